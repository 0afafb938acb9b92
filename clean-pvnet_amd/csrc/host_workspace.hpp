// host_workspace.hpp -- host side, part 1: errors, the problem and its workspace layout, per-device facts, tuning knobs.
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace); see that file
// for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py).
#pragma once

// Images of up to this many 2048-pixel tiles (480x640 = 150) subsample inside k_compact_hyp: one launch less on every
// call (-3 % at B = 64, -5 % at B = 1 on MI355X).  When subsampling does trigger, every block redoes the draws of the
// tiles before it, a cost that grows with the square of the tile count: at 190 tiles (540x720, BASELINE config 5, whose
// 31 k foreground pixels ARE subsampled) it already outweighs the launch (+2 %), so larger images keep k_tile_subsample.
constexpr int kFuseSubTiles = 160;
constexpr int kMaxTiles = 16000;     // tile prefix of an image in (dynamic) LDS: 64 KB => images up to ~32 Mpixel

// size of the per-device tables (num_cus, the stage hints, the side streams): a device of a larger ordinal is served
// without them
constexpr int kMaxDevices = 64;

thread_local char g_err[512] = "";

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return PVV_OK;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
    int T;
    size_t tiles, tile_list, tile_draw, tn, surv, coords, dirs, hyps, counts, sums, total;
    size_t lead;                                     // staged counting (count_prune.hpp): [B,K,8] leader counts; 0 = not reserved
    size_t ratio;                                    // [B,K] winner count / tn (k_select_refit -> k_finalize_v3 -> stage hint)
    size_t miss;                                     // staged counting: [B,K,hn] shared miss counters (count_filter_runs.hpp); 0 = not reserved
    size_t deferred;                                 // staged counting: [B] images whose rest-chunk rows the first count launch gathers; 0 = not reserved
};

bool use_bf16_count(const pvv_problem *p);
bool may_stage(const pvv_problem *p);

// Subsampling inside k_compact_hyp (no k_tile_subsample launch): only for images of <= kFuseSubTiles tiles and only when
// subsampling is unlikely -- max_num at least 1/16 of the image (30000 of 307200) -- and (make_front) only with the device RNG.
bool fuse_sub_shape(const pvv_problem *p, int T)
{
    return T <= kFuseSubTiles && (long long)p->max_num * 16 >= (long long)p->H * p->W;
}

// Does a call of this problem ever STORE per-pixel subsample draws (tile_draw: 4 B per pixel of the batch)?  Only the
// separate subsample pass reads them (k_tile_subsample; make_front: want_draws).  Whether that pass runs depends on pointer
// arguments the workspace query cannot see -- injected index pairs or draws switch the fused subsampling off -- unless the
// caller promises the device RNG (PVV_FLAG_DEVICE_RNG): then draws are stored only for images too large to fuse, and never
// when no mask of this shape can exceed max_num (the largest foreground_num: 255 per pixel, P:126).
bool may_store_draws(const pvv_problem *p, int T)
{
    // (the largest per-pixel weight: a byte mask's 255, or the fused argmax's class index seg_classes - 1 -- make_front's max_weight;
    // the workspace query cannot see which of the two the call will be, so the larger one decides: ADVICE r5)
    const long long max_weight = std::max(255ll, (long long)p->seg_classes - 1);
    if ((long long)p->max_num >= max_weight * p->H * p->W) return false;
    return !((p->flags & PVV_FLAG_DEVICE_RNG) && fuse_sub_shape(p, T));
}

// one set of leader words: [B,K,8] + the any_staged word
size_t lead_set_words(const pvv_problem *p) { return (size_t)p->B * p->K * 8 + 1; }

Layout make_layout(const pvv_problem *p)
{
    Layout L;
    const size_t HW = (size_t)p->H * p->W;
    L.T = (int)((HW + kTile - 1) / kTile);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
    L.tiles = take(sizeof(uint32_t) * (size_t)p->B * L.T);
    L.tile_list = take(sizeof(unsigned short) * (size_t)p->B * L.T * kTile);
    L.tile_draw = may_store_draws(p, L.T) ? take(sizeof(float) * (size_t)p->B * L.T * kTile) : 0;   // (0: not reserved)
    L.tn = take(sizeof(int) * (size_t)p->B);
    L.surv = take(sizeof(int) * (size_t)p->B * kSurvCap);
    L.coords = take(sizeof(float2) * (size_t)p->B * p->cap);
    L.dirs = take(sizeof(float2) * (size_t)p->B * p->K * p->cap);
    L.hyps = take(sizeof(float2) * (size_t)p->B * p->K * p->hn);
    L.counts = take(sizeof(int) * (size_t)p->B * p->K * p->hn);
    L.sums = take(sizeof(double) * (size_t)p->B * p->K * kRefitSplitMax * 5);
    L.ratio = take(sizeof(float) * (size_t)p->B * p->K);
    // (+ the any_staged word; TWO sets: the fused un_pnp call counts its v3 hypotheses and its estimate's as two staged passes)
    L.lead = may_stage(p) ? take(sizeof(int) * 2 * lead_set_words(p)) : 0;
    L.miss = may_stage(p) ? take(sizeof(int) * (size_t)p->B * p->K * p->hn) : 0;
    L.deferred = may_stage(p) ? take(sizeof(int) * (size_t)p->B) : 0;
    L.total = off;
    return L;
}

int validate(const pvv_problem *p)
{
    if (!p) return fail(PVV_E_ARG, "problem is NULL");
    if (p->B <= 0 || p->H <= 0 || p->W <= 0 || p->K <= 0 || p->hn <= 0)
        return fail(PVV_E_ARG, "B, H, W, K, hn must be positive");
    if (p->B > kMaxBatchLds) return fail(PVV_E_ARG, "B > 1024: split the batch");
    if (((long long)p->H * p->W + kTile - 1) / kTile > kMaxTiles) return fail(PVV_E_ARG, "H*W too large (more than 16000 tiles of 2048 pixels)");
    if ((long long)p->K * p->hn >= (1ll << 23)) return fail(PVV_E_ARG, "K*hn must be < 2^23");
    if (p->count_kernel < PVV_COUNT_AUTO || p->count_kernel > PVV_COUNT_STAGED_ESTIMATE) return fail(PVV_E_ARG, "unknown count_kernel");
    if (p->flags & ~(PVV_FLAG_DEVICE_RNG | PVV_FLAG_VERTEX_F16 | PVV_FLAG_VERTEX_BF16 | PVV_FLAG_SEG_F16 | PVV_FLAG_SEG_BF16))
        return fail(PVV_E_ARG, "unknown bits in flags");
    if ((p->flags & PVV_FLAG_VERTEX_F16) && (p->flags & PVV_FLAG_VERTEX_BF16))
        return fail(PVV_E_ARG, "flags: PVV_FLAG_VERTEX_F16 and PVV_FLAG_VERTEX_BF16 are exclusive");
    if ((p->flags & PVV_FLAG_SEG_F16) && (p->flags & PVV_FLAG_SEG_BF16))
        return fail(PVV_E_ARG, "flags: PVV_FLAG_SEG_F16 and PVV_FLAG_SEG_BF16 are exclusive");
    if (p->mask_elem_size != 1 && p->mask_elem_size != 2 && p->mask_elem_size != 4 &&
        p->mask_elem_size != 8)
        return fail(PVV_E_ARG, "mask_elem_size must be 1, 2, 4 or 8");
    if (p->cap <= 0 || (long long)p->cap > (long long)p->H * p->W)
        return fail(PVV_E_ARG, "cap must be in [1, H*W]");
    if ((long long)p->B * p->K * p->hn >= (1ll << 31) || (long long)p->B * p->K * p->cap >= (1ll << 40))
        return fail(PVV_E_ARG, "problem too large for one call");
    if (p->singular_policy < PVV_SINGULAR_REFERENCE || p->singular_policy > PVV_SINGULAR_IMAGE_ZERO)
        return fail(PVV_E_ARG, "unknown singular_policy");
    return PVV_OK;
}

int num_cus()
{
    // per device: one process may drive several GPUs (the bench and RCCL use one process per GPU, tests need not)
    static int cus[kMaxDevices] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    if (!cus[dev]) {
        hipDeviceProp_t prop;
        int n = 0;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        cus[dev] = n > 0 ? n : 256;
    }
    return cus[dev];
}

// the device the STREAM belongs to (a caller may launch on a stream of a device that is not current)
int stream_device(hipStream_t st)
{
    int dev = -1;
    if (st) {
        hipDevice_t d;
        if (hipStreamGetDevice(st, &d) == hipSuccess) dev = (int)d; else (void)hipGetLastError();
    }
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }     // (no sticky error on GPU-less hosts)
    return dev >= 0 && dev < kMaxDevices ? dev : -1;
}

// tuning knobs exist only in experimental builds (tools/build_variant.sh -DPVV_TUNING): the shipped library reads no
// environment variable
int tuning_int(const char *name, int dflt)
{
#ifdef PVV_TUNING
    // read ONCE per knob (tools/variant_ab.py loads a copy of the library per setting and restores the environment after
    // its first launches)
    static const char *names[32];
    static int vals[32], n = 0;
    for (int i = 0; i < n; ++i) if (!strcmp(names[i], name)) return vals[i] == INT32_MIN ? dflt : vals[i];
    const char *e = getenv(name);
    if (n < 32) { names[n] = name; vals[n] = e && *e ? atoi(e) : INT32_MIN; ++n; }
    return e && *e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

long long *tuning_ptr(const char *name)
{
#ifdef PVV_TUNING
    const char *e = getenv(name);      // re-read on every call: the tuning scripts change it between calls
    return e && *e ? (long long *)strtoull(e, nullptr, 0) : nullptr;
#else
    (void)name;
    return nullptr;
#endif
}

// optional stage-boundary events (pvv_problem.ev_marks, a measurement aid): mark i is recorded on the call's stream
int mark(const pvv_problem *p, int i, hipStream_t st)
{
    if (!p->ev_marks || !p->ev_marks[i]) return PVV_OK;
    if (hipEventRecord((hipEvent_t)p->ev_marks[i], st) != hipSuccess) return fail(PVV_E_ARG, "ev_marks holds an invalid hipEvent_t");
    return PVV_OK;
}

int check_ptrs(const pvv_problem *p, const void *mask, const void *vertex, void *ws, size_t ws_bytes,
               Layout *L)
{
    if (int e = validate(p)) return e;
    if (!mask || !vertex || !ws) return fail(PVV_E_ARG, "mask, vertex and workspace must be non-NULL");
    if ((uintptr_t)ws % 256 != 0) return fail(PVV_E_ARG, "workspace must be 256-byte aligned");
    *L = make_layout(p);
    if (ws_bytes < L->total) return fail(PVV_E_WORKSPACE, "workspace too small");
    return PVV_OK;
}
