// host_front.hpp -- host side, part 4: scan, subsample, compaction and count pass of a call; the side stream; the v3 refit.
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace); see that file
// for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py).
#pragma once

// A runtime element kind (kElemF32 / kElemF16 / kElemBF16) as a compile-time constant: fn(std::integral_constant<int, kElem*>{}).
template <class F>
void with_elem(int kind, F &&fn)
{
    if (kind == kElemF16) fn(std::integral_constant<int, kElemF16>{});
    else if (kind == kElemBF16) fn(std::integral_constant<int, kElemBF16>{});
    else fn(std::integral_constant<int, kElemF32>{});
}

template <int ES, int MODE, int ST = kElemF32>
void launch_scan(const MaskArgs &m, const Layout &L, char *ws, int B, hipStream_t st)
{
    const long long total = (long long)L.T * B;
    uint32_t *tiles = (uint32_t *)(ws + L.tiles);
    unsigned short *lists = (unsigned short *)(ws + L.tile_list);
    float *draws = (float *)(ws + L.tile_draw);
    // the read-ahead needs a contiguous mask; a strided mask or the fused argmax keep one short-lived block per tile
    // (their loads are not issued ahead, and a persistent block would walk its tiles one load latency at a time); ST: the
    // fused argmax's seg element type
    if (!(m.contig && !m.seg)) {
        hipLaunchKernelGGL((k_tile_scan<ES, false, MODE, ST>), dim3((unsigned)total), dim3(kBlock), 0, st, m, tiles, lists, draws, (int)total);
        return;
    }
    // ONE tile per block.  Round 2 made this kernel persistent over the resident blocks (8 per CU, every block 4-5 tiles with
    // the next tile's loads ahead: 4.0 -> 4.4 TB/s on the cold int64 mask) when it issued ~400 instructions per wave and
    // tile; at ~300 (round 3) the dispatcher's overlap of short blocks wins again -- one-process A/B over 4 ... 80 blocks
    // per CU in the grid rule, monotone: -2.1 % per call at B = 64, -1.1 % at B = 16, -2.4 % at B = 128, +-0 at B = 1 and
    // on config 5 against the persistent grid.  (The kernel still walks gridDim-strided tiles with its read-ahead if it is
    // ever launched with fewer blocks: PVV_SCAN_PER_CU in tuning builds.)
    const int per_cu_t = tuning_int("PVV_SCAN_PER_CU", 0);
    long long per_block = 1;
    if (per_cu_t > 0) per_block = (total + (long long)per_cu_t * num_cus() - 1) / ((long long)per_cu_t * num_cus());
    const int grid = (int)((total + per_block - 1) / per_block);
    hipLaunchKernelGGL((k_tile_scan<ES, true, MODE>), dim3(grid), dim3(kBlock), 0, st, m, tiles, lists, draws, (int)total);
}

// What run_front launches as "the count pass" when it is not one pass over whole rows: the first of the fused un_pnp call's two
// passes (pvv_decode_keypoint_un_pnp); the caller launches the second one itself.
struct CountPlan {
    const pvv_problem *p = nullptr;         // the problem of that pass: p->hn columns of rows of cols.hstride
    CountPass staged = CountPass::Full;     // decide_staged() for it
    CountCols cols;
};

// How the scan reads a mask element (MaskArgs.mode).
enum class MaskRule : int {
    LowByte = 0,         // low byte != 0: ransac_voting_layer_v3 (P:125)
    EqualsOne = 1,       // == 1: the estimate (P:207)
};

// What a call hands to run_front.  stream_first / stream_rest: RNG stream of the hypotheses [0, hn_first) / [hn_first, hn) -- 1 for
// ransac_voting_layer_v3, 3 for the estimate, so that the two layers never share draws under one seed
struct FrontArgs {
    MaskRule rule = MaskRule::LowByte;
    const void *mask = nullptr;          // the mask, or
    const float *seg = nullptr;          // the seg logits the scan takes the argmax of (decode calls), with
    int64_t *mask_out = nullptr;         // the int64 mask they emit (may be nullptr)
    const float *vertex = nullptr;
    const int32_t *idxs = nullptr;       // injected index pairs of the hypotheses [0, hn_first) / [hn_first, hn), or nullptr
    const int32_t *idxs2 = nullptr;
    int hn_first = -1;                   // (-1: p->hn, one range)
    const float *selection = nullptr;    // injected subsample draws, or nullptr
    uint32_t stream_first = 1u, stream_rest = 3u;
    int32_t *tn_out = nullptr;
    CountsNeed need = CountsNeed::All;   // decide_staged's question
    const CountPlan *plan = nullptr;     // != nullptr: the count pass run_front launches (need is then not consulted)
    const float *mean = nullptr;         // the estimate: the keypoints its staged pass orders the chunks by
};

struct Front {
    MaskArgs m;
    VertexArgs v;
    HypArgs h;
    bool can_subsample;
    bool seg2;                // two-class seg in two contiguous planes: k_tile_scan_seg2 (4 pixels per load)
    int vt, st;               // element types (kElem*) of the vertex field and of the seg logits: PVV_FLAG_VERTEX_* / _SEG_*
    long long *mask_deferred; // != nullptr: the scan does not write the int64 mask; k_mask_from_lists does, on the side stream
};

Front make_front(const pvv_problem *p, const Layout &L, char *ws, const FrontArgs &a)
{
    Front f;
    MaskArgs &m = f.m;
    m.mask = a.mask;
    m.seg = a.seg;
    m.mask_out = (long long *)a.mask_out;
    m.gb = p->seg_stride[0]; m.gc = p->seg_stride[1]; m.gh = p->seg_stride[2]; m.gw = p->seg_stride[3];
    m.C = p->seg_classes;
    m.selection = a.selection;
    m.sb = p->mask_stride[0]; m.sh = p->mask_stride[1]; m.sw = p->mask_stride[2];
    m.es = p->mask_elem_size;
    m.contig = (m.sw == 1 && m.sh == p->W) ? 1 : 0;
    m.mode = (int)a.rule;
    m.W = p->W; m.HW = p->H * p->W; m.T = L.T;
    m.min_num = p->min_num; m.max_num = p->max_num; m.cap = p->cap;
    m.seed = p->seed;
    m.b0 = p->first_image;
    m.tn_user = a.tn_out;
    m.status = p->d_status;
    // Subsampling inside k_compact_hyp (no k_tile_subsample launch) only for images of <= kFuseSubTiles tiles, only when
    // subsampling is unlikely -- max_num at least 1/16 of the image (30000 of 307200) -- and only with the device RNG:
    // injected index pairs address rows of the SUBSAMPLED list, which the hypothesis blocks can read off the tile lists
    // only after k_tile_subsample has rewritten them.
    m.fuse_sub = (fuse_sub_shape(p, L.T) && !a.idxs && !a.idxs2) ? 1 : 0;
    // largest possible foreground_num: the sum of byte values (P:126), of class indices (fused argmax) or of ones (P:208)
    const long long max_weight = a.rule == MaskRule::EqualsOne ? 1 : (a.seg ? (p->seg_classes > 1 ? p->seg_classes - 1 : 1) : 255);
    f.can_subsample = (long long)p->max_num < max_weight * (long long)p->H * p->W;
    m.want_draws = (f.can_subsample && !m.fuse_sub) ? 1 : 0;     // fused subsampling evaluates its draws on demand (compaction.hpp)
    f.vt = (p->flags & PVV_FLAG_VERTEX_F16) ? kElemF16 : (p->flags & PVV_FLAG_VERTEX_BF16) ? kElemBF16 : kElemF32;
    f.st = (p->flags & PVV_FLAG_SEG_F16) ? kElemF16 : (p->flags & PVV_FLAG_SEG_BF16) ? kElemBF16 : kElemF32;
    const int seg_es = f.st == kElemF32 ? 4 : 2, vertex_es = f.vt == kElemF32 ? 4 : 2;
    // decode_keypoint's real layout (resnet18.py:69,93): a two-class seg in two contiguous planes, every 4 pixels one aligned
    // load (16 bytes of f32, 8 of f16 / bf16)
    f.seg2 = a.seg && p->seg_classes == 2 && m.gw == 1 && m.gh == p->W && (((long long)p->H * p->W) & 3) == 0 && (m.gb & 3) == 0 &&
             (m.gc & 3) == 0 && ((uintptr_t)a.seg % (4 * seg_es)) == 0;
    // ... whose int64 mask (8 B per pixel, as much as the scan reads) can be written from the tile lists beside the rest of
    // the call instead of by the scan, when the lists stay complete (k_tile_subsample would rewrite them) and the batch is
    // large enough for the two cross-stream events to pay (measured: B = 64 480x640, scan 70.5 -> ~27 us)
    f.mask_deferred = nullptr;
    if (f.seg2 && a.mask_out && !(f.can_subsample && !m.fuse_sub) && (long long)p->B * p->H * p->W >= (1ll << 21) &&
        ((uintptr_t)a.mask_out & 15) == 0)
        f.mask_deferred = (long long *)a.mask_out;
    VertexArgs &v = f.v;
    v.vertex = a.vertex;
    v.sb = p->vertex_stride[0]; v.sh = p->vertex_stride[1]; v.sw = p->vertex_stride[2];
    v.sk = p->vertex_stride[3]; v.sc = p->vertex_stride[4];
    v.K = p->K;
    v.vec2 = (v.sc == 1 && !(v.sb & 1) && !(v.sh & 1) && !(v.sw & 1) && !(v.sk & 1) &&
              ((uintptr_t)a.vertex % (2 * vertex_es) == 0)) ? 1 : 0;
    HypArgs &h = f.h;
    h.idxs = a.idxs; h.idxs2 = a.idxs2;
    h.hn = p->hn; h.hn_first = a.hn_first < 0 ? p->hn : a.hn_first;
    h.stream = a.stream_first; h.stream2 = a.stream_rest;
    h.hyps = (float2 *)(ws + L.hyps);
    h.counts = (int *)(ws + L.counts);
    h.draws_out = p->d_draws_out;
    h.blocks = (int)(((long long)p->K * p->hn + kBlock - 1) / kBlock);
    h.surv = (int *)(ws + L.surv);
    h.lead = L.lead ? (int *)(ws + L.lead) : nullptr;
    h.miss = L.miss ? (int *)(ws + L.miss) : nullptr;
    h.defer_mask = 0u; h.deferred = nullptr;                       // (run_front: a call whose first count pass is v3 in stages)
    return f;
}

int run_scan(const pvv_problem *p, const Front &f, char *ws, const Layout &L, hipStream_t st, bool write_mask)
{
    if (f.seg2) {
        MaskArgs m = f.m;
        if (!write_mask) m.mask_out = nullptr;
        const unsigned total = (unsigned)((long long)L.T * p->B);
        uint32_t *tiles = (uint32_t *)(ws + L.tiles);
        unsigned short *lists = (unsigned short *)(ws + L.tile_list);
        float *draws = (float *)(ws + L.tile_draw);
        auto go2 = [&](auto et) {
            constexpr int ST = decltype(et)::value;
            if (write_mask) hipLaunchKernelGGL((k_tile_scan_seg2<true, ST>), dim3(total), dim3(kBlock), 0, st, m, tiles, lists, draws);
            else hipLaunchKernelGGL((k_tile_scan_seg2<false, ST>), dim3(total), dim3(kBlock), 0, st, m, tiles, lists, draws);
        };
        with_elem(f.st, go2);
        return check_launch("k_tile_scan_seg2");
    }
    if (f.m.seg && f.st != kElemF32) {
        // 2-byte logits, generic layout: the argmax reads seg only (never the mask) and only the decode calls (mode 0) pass
        // one, so one instantiation per element type
        with_elem(f.st, [&](auto et) { launch_scan<8, 0, decltype(et)::value>(f.m, L, ws, p->B, st); });
        return check_launch("k_tile_scan");
    }
    // (the mask's interpretation -- low byte for v3, == 1 for the estimate -- is a template parameter of the scan)
    auto go = [&](auto es) {
        constexpr int ES = decltype(es)::value;
        if (f.m.mode == (int)MaskRule::LowByte) launch_scan<ES, 0>(f.m, L, ws, p->B, st); else launch_scan<ES, 1>(f.m, L, ws, p->B, st);
    };
    switch (f.m.es) {
    case 1: go(std::integral_constant<int, 1>{}); break;
    case 2: go(std::integral_constant<int, 2>{}); break;
    case 4: go(std::integral_constant<int, 4>{}); break;
    default: go(std::integral_constant<int, 8>{}); break;
    }
    return check_launch("k_tile_scan");
}

// ---------------------------------------------------------------------------------------------
// The side stream: one per device, created on first use, for work of a call that nothing in the call waits for -- today
// the deferred int64 mask of decode_keypoint (k_mask_from_lists).  Fork: an event recorded on the caller's stream behind
// the scan, the side stream waits for it; join: an event recorded behind the side kernel, the caller's stream waits for
// it at the end of run_front -- by then the kernel has long finished, it ran beside the compaction and the count pass.
// hipStreamWaitEvent takes the event's state at the time of the call, so the events are reused (a ring of 8 pairs).
// Not used while the caller's stream is capturing (no stream or event is created under capture) or when the stream
// belongs to a device that is not current.
// ---------------------------------------------------------------------------------------------
// Both streams are on ONE device: the events between them need no system-scope fence (host / other devices do not look at
// what they order), only the agent-scope release every kernel ends with.
#ifdef PVV_SIDE_EVENT_SYSTEM_FENCE                                    // (tuning builds: A/B of the event flags)
constexpr unsigned kSideEventFlags = hipEventDisableTiming;
#else
constexpr unsigned kSideEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
#endif
struct SideStream {
    hipStream_t st = nullptr;
    hipEvent_t fork[8] = {}, join[8] = {};
    int next = 0;
    bool tried = false, ok = false;
};
SideStream g_side[kMaxDevices];
std::mutex g_side_mu;

// can work of a call on `st` be forked to the side stream?  (creates it on first use)
SideStream *side_get(hipStream_t st)
{
    int cur = -1;
    const int dev = stream_device(st);
    if (dev < 0 || hipGetDevice(&cur) != hipSuccess || cur != dev) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    std::lock_guard<std::mutex> lock(g_side_mu);
    SideStream *g = &g_side[dev];
    if (!g->tried) {
        g->tried = true;
        bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; ok && i < 8; ++i)
            ok = hipEventCreateWithFlags(&g->fork[i], kSideEventFlags) == hipSuccess &&
                 hipEventCreateWithFlags(&g->join[i], kSideEventFlags) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        g->ok = ok;
    }
    return g->ok ? g : nullptr;
}

// Fork: `side` waits for everything enqueued on `st` so far.  Call with g_side_mu held (SideFork below): the ring slot, the
// fork record and the side stream's wait are one step, and so are the kernel launched on the side stream and its join record --
// two threads forking at once would otherwise interleave records and launches on the one side stream.
bool side_fork_locked(SideStream *g, hipStream_t st, hipStream_t *side, hipEvent_t *join)
{
    const int i = g->next;
    g->next = (i + 1) & 7;
    if (hipEventRecord(g->fork[i], st) != hipSuccess || hipStreamWaitEvent(g->st, g->fork[i], 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    *side = g->st;
    *join = g->join[i];
    return true;
}

// Joins the side stream back into the caller's stream on EVERY way out of run_front once work has been forked (an
// error return between fork and join used to leave the side kernel unordered with `stream` while the caller already held
// an error code).  The join event of a ring slot may be re-recorded by a later fork before this wait is issued: both
// records are on the one in-order side stream, so waiting for the later one still covers this call's kernel.
struct SideJoin {
    hipStream_t st = nullptr;
    hipEvent_t join = nullptr;
    bool armed = false;
    int finish()                                                   // explicit join on the success path: its failure is an error
    {
        if (!armed) return PVV_OK;
        armed = false;
        return hipStreamWaitEvent(st, join, 0) == hipSuccess ? PVV_OK : fail(PVV_E_ARG, "side stream: hipStreamWaitEvent failed");
    }
    ~SideJoin()
    {
        if (armed && hipStreamWaitEvent(st, join, 0) != hipSuccess) (void)hipGetLastError();   // (the call is failing already)
    }
};

// mask scan + (subsample) + compaction and hypotheses + counting, shared by both layers.
int run_front(const pvv_problem *p, const Layout &L, char *ws, hipStream_t st, const FrontArgs &a)
{
    if ((p->flags & PVV_FLAG_DEVICE_RNG) && (a.idxs || a.idxs2 || a.selection))
        return fail(PVV_E_ARG, "PVV_FLAG_DEVICE_RNG promises d_idxs = d_idxs_est = d_selection = NULL");
    Front f = make_front(p, L, ws, a);
    if (f.m.want_draws && L.tile_draw == 0) return fail(PVV_E_WORKSPACE, "workspace holds no draw storage for this call");   // (cannot happen: may_store_draws)
    // whether the count pass runs in stages is decided HERE, once: a call that will not stage neither zeroes nor reads the
    // miss counters and leader words (k_compact_hyp would otherwise clear B*K*hn words for nothing on every AUTO call)
    // (a plan: some pass of the call stages -- the caller decided -- so the words are zeroed for all columns)
    const CountPlan *plan = a.plan;
    const CountPass pass = plan ? plan->staged : decide_staged(p, L, st, a.need);
    if (!plan && pass == CountPass::Full) { f.h.miss = nullptr; f.h.lead = nullptr; }
    // ... and so is the chunk schedule of a v3 pass in stages, because k_compact_hyp then leaves the rows the first count launch
    // does not read to that launch's gather blocks (HypArgs.defer_mask; count_bf16.hpp).  Every other pass -- full, exact, the
    // estimate in stages, a v3 pass on the 48-per-CU grid (count_grid_short), the fused un_pnp call -- has all its rows gathered up front, as has
    // pvv_rerun_count_kernel, whose rows are there already.
    CountCols cols = plan ? plan->cols : CountCols();
    if (!plan) cols.mean = a.mean;
    GatherArgs ga{};
    // (not the fused un_pnp call -- a plan --: its compaction launch is mostly hypothesis blocks, nine times v3's, and a second count
    // pass follows; deferring there measured +1 % per call, profiles/deferred_rows_ab.json)
    if (!plan && pass == CountPass::StagedV3 && L.deferred != 0 && count_grid_short(p) && tuning_int("PVV_DEFER_ROWS", 1) != 0) {
        cols.first = stage_schedule(p, st, pass);
        f.h.defer_mask = cols.first;
        f.h.deferred = (int *)(ws + L.deferred);
        ga.vt = f.vt; ga.deferred = f.h.deferred; ga.dirs = (float2 *)(ws + L.dirs); ga.v = f.v;
        cols.gather = &ga;
    }
    if (int e = mark(p, PVV_MARK_BEGIN, st)) return e;
    SideJoin sj;
    // no side stream to be had (the caller's stream is being captured, ...): the scan writes the mask itself
    SideStream *sg = (f.mask_deferred && tuning_int("PVV_MASK_DEFER", 1) != 0) ? side_get(st) : nullptr;
    const bool defer_mask = sg != nullptr;
    if (int e = run_scan(p, f, ws, L, st, !defer_mask)) return e;
    if (!f.m.fuse_sub && f.can_subsample) {
        hipLaunchKernelGGL(k_tile_subsample, dim3(L.T, p->B), dim3(kBlock), 0, st, f.m, (uint32_t *)(ws + L.tiles),
                           (unsigned short *)(ws + L.tile_list), (const float *)(ws + L.tile_draw));
        if (int e = check_launch("k_tile_subsample")) return e;
    }
    if (int e = mark(p, PVV_MARK_SCAN, st)) return e;
    auto compact = [&](auto et) {
        constexpr int VT = decltype(et)::value;
        auto kernel = f.h.defer_mask != 0u ? k_compact_hyp<VT, true> : k_compact_hyp<VT, false>;
        hipLaunchKernelGGL(kernel, dim3(L.T + f.h.blocks, p->B), dim3(kBlock), sizeof(int) * (size_t)L.T, st, f.m, f.v,
                           f.h, (const uint32_t *)(ws + L.tiles), (const unsigned short *)(ws + L.tile_list),
                           (const float *)(ws + L.tile_draw), (int *)(ws + L.tn), (float2 *)(ws + L.coords),
                           (float2 *)(ws + L.dirs));
    };
    with_elem(f.vt, compact);
    if (int e = check_launch("k_compact_hyp")) return e;
    if (int e = mark(p, PVV_MARK_COMPACT, st)) return e;
    if (defer_mask) {
        // forked BEHIND the compaction (measured: forked behind the scan, the 157 MB of stores cost the latency-bound
        // compaction +14 us at B = 64 and the count pass +9; the count pass alone is 130 us of mostly VALU work)
        std::lock_guard<std::mutex> lock(g_side_mu);                // fork, launch and join record: one step (see side_fork_locked)
        hipStream_t side = nullptr;
        hipEvent_t join = nullptr;
        const bool forked = side_fork_locked(sg, st, &side, &join);
        const hipStream_t ms = forked ? side : st;                  // the fork failed: the same kernel, in line
        const long long total = (long long)L.T * p->B;
        const int grid = (int)std::min<long long>(total, (long long)tuning_int("PVV_MASK_GRID_PER_CU", 2) * num_cus());
        hipLaunchKernelGGL(k_mask_from_lists, dim3(grid), dim3(kBlock), 0, ms, (const uint32_t *)(ws + L.tiles),
                           (const unsigned short *)(ws + L.tile_list), f.mask_deferred, L.T, p->H * p->W, (int)total);
        const int le = check_launch("k_mask_from_lists");
        if (forked) {
            // whatever happened to the launch, the side stream now holds this call's fork: join it back on every exit
            if (hipEventRecord(join, side) == hipSuccess) { sj.st = st; sj.join = join; sj.armed = true; }
            else {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(side);                   // no event to wait for: drain the side stream instead
                if (!le) return fail(PVV_E_ARG, "side stream: hipEventRecord failed");
            }
        }
        if (le) return le;
    }
    if (int e = launch_count_any(plan ? plan->p : p, L, ws, st, pass, cols)) return e;
    if (int e = sj.finish()) return e;
    return mark(p, PVV_MARK_COUNT, st);
}

// What finish_v3 delivers.  hstride: row length of hyps / counts in the workspace (= p->hn unless the row also holds the
// hypotheses of a fused estimate, pvv_decode_keypoint_un_pnp)
struct V3Out {
    float *kpt = nullptr;            // [B,K,2]
    int32_t *win_counts = nullptr;   // [B,K], or nullptr
    int hstride = 0;                 // (0: p->hn)
};

int finish_v3(const pvv_problem *p, const Layout &L, char *ws, hipStream_t st, const V3Out &out)
{
    const int hstride = out.hstride > 0 ? out.hstride : p->hn;
    // blocks per (keypoint, image): the largest power of two that keeps the grid within ~6 blocks per CU (measured on
    // MI355X: 2 at B*K = 576, 8 for a single image)
    int nsplit = kRefitSplitMax;
    while (nsplit > 1 && (long long)p->B * p->K * nsplit > 6ll * num_cus()) nsplit >>= 1;
    nsplit = tuning_int("PVV_REFIT_SPLIT", nsplit);
    // the re-vote's prefilter is the count kernel's second-level test: used where that kernel is valid and the grid is
    // large enough to be VALU-bound (measured: -1.3 % per call at B = 64, +-0 at B = 8, +1.2 % at B = 1)
    const Bf16Consts fc = bf16_consts(p->inlier_thresh);
    const bool band = use_bf16_count(p) && (long long)p->B * p->K >= 128;
    auto launch_refit = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(p->K * nsplit, p->B), dim3(kBlock), 0, st,
                           (const int *)(ws + L.tn), (const float2 *)(ws + L.coords),
                           (const float2 *)(ws + L.dirs), (const float2 *)(ws + L.hyps),
                           (const int *)(ws + L.counts), (double *)(ws + L.sums), out.win_counts, p->K, p->hn, hstride,
                           p->cap, p->inlier_thresh, nsplit, (float *)(ws + L.ratio), fc);
    };
    if (band) launch_refit(k_select_refit<true>); else launch_refit(k_select_refit<false>);
    if (int e = check_launch("k_select_refit")) return e;
    if (int e = mark(p, PVV_MARK_SELECT, st)) return e;
    // the stage hint is only ever consulted by AUTO for problems that may stage: other calls do not write it (a store to
    // host-visible memory at the end of a 3 us kernel: the reference's own eval batch is B = 1)
    float *hint = (p->count_kernel == PVV_COUNT_AUTO && may_stage(p)) ? stage_hint_claim(p, st) : nullptr;
    hipLaunchKernelGGL(k_finalize_v3, dim3(p->B), dim3(64), 0, st, (const int *)(ws + L.tn),
                       (const double *)(ws + L.sums), (float2 *)out.kpt, p->K, p->singular_policy, nsplit,
                       (const float *)(ws + L.ratio), hint, kMaxBatchLds);
    if (int e = check_launch("k_finalize_v3")) return e;
    return mark(p, PVV_MARK_END, st);
}
