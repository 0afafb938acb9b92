// pvnet_vote.hip -- RANSAC voting hot path of clean-pvnet as native HIP for gfx950 (MI355X).
//
// Written for CDNA4 only: 64-lane wavefronts are assumed everywhere (ballot masks are 64 bit,
// lane broadcasts use v_readlane), there is no CUDA path and no CPU fallback.
//
// Arithmetic contract (see oracle/vote_oracle.c): the inlier decision and the hypothesis
// intersection are IEEE binary32 with one rounding per source-level operation and NO fused
// multiply-add, so inlier counts are bit-exact against the oracle.  This file must be built
// with -ffp-contract=off; the pragma below enforces it even if the flag is forgotten.
//
// Reference behaviour restated (paths relative to /root/reference):
//   K = lib/csrc/ransac_voting/src/ransac_voting_kernel.cu
//   P = lib/csrc/ransac_voting/ransac_voting_gpu.py
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "pvnet_vote.h"

#pragma clang fp contract(off)

#define PVV_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

// (the tile constants the kernel parts are written against; the host-only ones are in host_workspace.hpp)
constexpr int kBlock = 256;          // 4 wavefronts
constexpr int kTileSteps = 8;
constexpr int kTile = kBlock * kTileSteps;  // pixels per compaction tile
constexpr int kPixPerWave = 64;      // pixels one wave walks per work item of the exact count kernel

#include "vote_common.hpp"
#include "compaction.hpp"
#include "count_exact.hpp"
#include "count_tile.hpp"
#include "count_bf16.hpp"
#include "count_filter_runs.hpp"
#include "count_prune.hpp"
#include "refit.hpp"
#include "covariance.hpp"
#include "legacy_kernels.hpp"

// host side, in dependency order
#include "host_workspace.hpp"
#include "host_stage.hpp"
#include "host_count.hpp"
#include "host_front.hpp"

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
PVV_EXPORT int pvv_abi_version(void) { return PVV_ABI_VERSION; }
PVV_EXPORT const char *pvv_last_error(void) { return g_err; }

// ABI v8: give back what the library created behind the caller's back (see the header).  Everything is released even when
// a call fails; the first error is reported.
PVV_EXPORT int pvv_shutdown(void)
{
    int rc = PVV_OK;
    auto note = [&](hipError_t e, const char *what) {
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (rc == PVV_OK) { snprintf(g_err, sizeof(g_err), "pvv_shutdown: %s: %s", what, hipGetErrorString(e)); rc = (int)e; }
        }
    };
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    if (!have_cur) (void)hipGetLastError();
    {
        std::lock_guard<std::mutex> lock(g_side_mu);
        for (int dev = 0; dev < kMaxDevices; ++dev) {
            SideStream *g = &g_side[dev];
            if (g->tried) {
                if (have_cur && hipSetDevice(dev) != hipSuccess) (void)hipGetLastError();
                if (g->st) { note(hipStreamSynchronize(g->st), "hipStreamSynchronize(side stream)"); note(hipStreamDestroy(g->st), "hipStreamDestroy"); }
                for (int i = 0; i < 8; ++i) {
                    if (g->fork[i]) note(hipEventDestroy(g->fork[i]), "hipEventDestroy");
                    if (g->join[i]) note(hipEventDestroy(g->join[i]), "hipEventDestroy");
                }
            }
            *g = SideStream();
        }
    }
    {
        std::lock_guard<std::mutex> lock(g_hint_mu);
        for (int dev = 0; dev < kMaxDevices; ++dev) {
            StageHint *g = &g_hint[dev];
            if (g->ratio) note(hipHostFree(g->ratio), "hipHostFree(stage hint)");
            *g = StageHint();
        }
    }
    if (have_cur && hipSetDevice(cur) != hipSuccess) (void)hipGetLastError();
    return rc;
}

PVV_EXPORT int pvv_stage_hint_query(float *mean_ratio, float *threshold, const pvv_problem *p, void *stream)
{
    float m = stage_hint_mean(p, (hipStream_t)stream);
    if (threshold) *threshold = -1.f;
    if (p) {
        const double work = stage_work(p, (hipStream_t)stream, &m);
        // (a problem whose evaluations stay below the bound is never staged by AUTO: reported as a threshold no ratio reaches)
        if (threshold) *threshold = work >= kStageMinWork ? stage_hint_threshold(p, work) : 2.f;
    }
    if (mean_ratio) *mean_ratio = m;
    return m >= 0.f ? 1 : 0;
}

PVV_EXPORT int32_t pvv_default_cap(int32_t H, int32_t W, int32_t max_num)
{
    long long hw = (long long)H * W;
    if (max_num < 0) max_num = 0;
    long long cap = (long long)max_num + (long long)(8.0 * std::sqrt((double)max_num)) + 64;
    return (int32_t)(cap < hw ? cap : hw);
}

PVV_EXPORT size_t pvv_workspace_bytes(const pvv_problem *p)
{
    if (validate(p)) return 0;
    return make_layout(p).total;
}

PVV_EXPORT int pvv_workspace_layout(const pvv_problem *p, pvv_workspace_offsets *out)
{
    if (int e = validate(p)) return e;
    if (!out) return fail(PVV_E_ARG, "out is NULL");
    const Layout L = make_layout(p);
    out->tn = L.tn; out->coords = L.coords; out->dirs = L.dirs; out->hyps = L.hyps; out->counts = L.counts;
    out->deferred = L.deferred; out->total = L.total;
    return PVV_OK;
}

// ransac_voting_layer_v3 behind its two exports, which have checked their arguments and say in `a` where the mask comes from
static int run_v3(const pvv_problem *p, const Layout &L, FrontArgs &a, const float *d_vertex, const int32_t *d_idxs,
                  const float *d_selection, void *d_workspace, float *d_out, int32_t *d_win_counts, int32_t *d_tn, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    a.vertex = d_vertex; a.idxs = d_idxs; a.selection = d_selection;
    a.tn_out = d_tn;
    a.need = CountsNeed::ArgMax;
    if (int e = run_front(p, L, ws, st, a)) return e;
    V3Out out;
    out.kpt = d_out; out.win_counts = d_win_counts;
    return finish_v3(p, L, ws, st, out);
}

PVV_EXPORT int pvv_ransac_voting_v3(const pvv_problem *p, const void *d_mask, const float *d_vertex,
                                    const int32_t *d_idxs, const float *d_selection,
                                    void *d_workspace, size_t workspace_bytes, float *d_out,
                                    int32_t *d_win_counts, int32_t *d_tn, void *stream)
{
    Layout L;
    if (int e = check_ptrs(p, d_mask, d_vertex, d_workspace, workspace_bytes, &L)) return e;
    if (!d_out) return fail(PVV_E_ARG, "d_out is NULL");
    FrontArgs a;
    a.mask = d_mask;
    return run_v3(p, L, a, d_vertex, d_idxs, d_selection, d_workspace, d_out, d_win_counts, d_tn, stream);
}

PVV_EXPORT int pvv_decode_keypoint_v3(const pvv_problem *p, const float *d_seg, const float *d_vertex,
                                      const int32_t *d_idxs, const float *d_selection, void *d_workspace,
                                      size_t workspace_bytes, int64_t *d_mask_out, float *d_out,
                                      int32_t *d_win_counts, int32_t *d_tn, void *stream)
{
    Layout L;
    if (p && p->mask_elem_size == 0) return fail(PVV_E_ARG, "set mask_elem_size = 8 (the int64 mask this call emits)");
    if (int e = check_ptrs(p, d_seg, d_vertex, d_workspace, workspace_bytes, &L)) return e;
    if (!d_out) return fail(PVV_E_ARG, "d_out is NULL");
    if (p->seg_classes < 1 || p->seg_classes > 256) return fail(PVV_E_ARG, "seg_classes must be in [1, 256]");
    FrontArgs a;
    a.seg = d_seg; a.mask_out = d_mask_out;
    return run_v3(p, L, a, d_vertex, d_idxs, d_selection, d_workspace, d_out, d_win_counts, d_tn, stream);
}

// k_covariance over columns [hoff, hoff + hn) of count rows hstride wide, about d_mean; d_hyp / d_counts: copies out, or nullptr
static int launch_covariance(const pvv_problem *p, const Layout &L, char *ws, hipStream_t st, const float *d_mean, float *d_cov,
                             float *d_hyp, int32_t *d_counts, float *d_weights, int hn, int hstride, int hoff)
{
    hipLaunchKernelGGL(k_covariance, dim3(p->K, p->B), dim3(kBlock), 0, st, (const int *)(ws + L.tn), (const float2 *)(ws + L.hyps),
                       (const int *)(ws + L.counts), (const float2 *)d_mean, d_cov, (float2 *)d_hyp, d_counts, d_weights, p->K, hn, hstride, hoff);
    return check_launch("k_covariance");
}

PVV_EXPORT int pvv_estimate_voting_distribution(const pvv_problem *p, const void *d_mask,
                                                const float *d_vertex, const int32_t *d_idxs,
                                                const float *d_selection, const float *d_mean,
                                                void *d_workspace, size_t workspace_bytes,
                                                float *d_cov, float *d_hyp, int32_t *d_counts,
                                                int32_t *d_tn, float *d_weights, void *stream)
{
    Layout L;
    if (int e = check_ptrs(p, d_mask, d_vertex, d_workspace, workspace_bytes, &L)) return e;
    if (!d_mean || !d_cov) return fail(PVV_E_ARG, "d_mean / d_cov is NULL");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    // the counts are an output (d_counts): every one of them is needed; otherwise the pass may drop what cannot carry weight
    FrontArgs a;
    a.rule = MaskRule::EqualsOne;
    a.mask = d_mask; a.vertex = d_vertex;
    a.idxs = d_idxs; a.selection = d_selection;
    a.stream_first = 3u;
    a.tn_out = d_tn;
    a.need = d_counts ? CountsNeed::All : CountsNeed::EstimateWindow;
    a.mean = d_mean;
    if (int e = run_front(p, L, ws, st, a)) return e;
    if (int e = launch_covariance(p, L, ws, st, d_mean, d_cov, d_hyp, d_counts, d_weights, p->hn, /*hstride=*/p->hn, /*hoff=*/0)) return e;
    return mark(p, PVV_MARK_END, st);
}

PVV_EXPORT int pvv_estimate_counts_in_stages(const pvv_problem *p)
{
    if (int e = validate(p)) return e < 0 ? e : -e;
    if (!may_stage(p)) return 0;
    return (p->count_kernel == PVV_COUNT_STAGED_ESTIMATE || (p->count_kernel == PVV_COUNT_AUTO && est_stage_auto(p, /*st=*/nullptr))) ? 1 : 0;
}

// resnet18.py:65-72 with cfg.test.un_pnp as ONE pass (see the header): the row of every (image, keypoint) holds the hn
// hypotheses of ransac_voting_layer_v3 followed by the hn_est of estimate_voting_distribution_with_mean.
static pvv_problem un_pnp_problem(const pvv_problem *p, int32_t hn_est)
{
    pvv_problem q = *p;
    q.hn = p->hn + hn_est;
    return q;
}

PVV_EXPORT size_t pvv_workspace_bytes_un_pnp(const pvv_problem *p, int32_t hn_est)
{
    if (validate(p) || hn_est <= 0) return 0;
    const pvv_problem q = un_pnp_problem(p, hn_est);
    if (validate(&q)) return 0;
    return make_layout(&q).total;
}

PVV_EXPORT int pvv_decode_keypoint_un_pnp(const pvv_problem *p, int32_t hn_est, const float *d_seg,
                                          const float *d_vertex, const int32_t *d_idxs, const int32_t *d_idxs_est,
                                          const float *d_selection, void *d_workspace, size_t workspace_bytes,
                                          int64_t *d_mask_out, float *d_kpt, float *d_cov, float *d_weights,
                                          int32_t *d_win_counts, int32_t *d_tn, void *stream)
{
    if (int e = validate(p)) return e;
    if (hn_est <= 0) return fail(PVV_E_ARG, "hn_est must be positive");
    if (p->mask_elem_size == 0) return fail(PVV_E_ARG, "set mask_elem_size = 8 (the int64 mask this call emits)");
    // v3 takes `mask != 0` as foreground, the estimate `mask == 1` (P:125 vs P:207): one compaction serves both only
    // when the argmax cannot produce anything but 0 and 1
    if (p->seg_classes != 2) return fail(PVV_E_ARG, "the fused un_pnp pass needs seg_classes == 2 (PVNet's seg_dim)");
    const pvv_problem q = un_pnp_problem(p, hn_est);
    Layout L;
    if (int e = check_ptrs(&q, d_seg, d_vertex, d_workspace, workspace_bytes, &L)) return e;
    if (!d_kpt || !d_cov) return fail(PVV_E_ARG, "d_kpt / d_cov is NULL");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    // Round 5: when the estimate alone would count in stages (decide_staged: large batches, AUTO; or forced) the rows are counted
    // as TWO passes over the one compaction -- columns [0, hn) as ransac_voting_layer_v3 would (full or in stages, the same rule
    // and the same stage hint as the layer's own call), then, behind the refit that delivers the mean, columns [hn, hn + hn_est)
    // against the estimate's bound.  Same results as the one full pass over all columns, bit for bit; what the two separate calls
    // cost more -- a second mask scan and a second compaction -- stays saved.
    pvv_problem pe = *p, p1 = *p;
    pe.hn = hn_est;
    const CountPass est_pass = decide_staged(&pe, L, st, CountsNeed::EstimateWindow);
    FrontArgs a;
    a.seg = d_seg; a.mask_out = d_mask_out; a.vertex = d_vertex;
    a.idxs = d_idxs; a.idxs2 = d_idxs_est; a.hn_first = p->hn;
    a.selection = d_selection;
    a.tn_out = d_tn;
    a.need = CountsNeed::All;
    CountPlan plan;
    if (est_pass != CountPass::Full) {
        const size_t set_bytes = sizeof(int) * lead_set_words(p);
        // the second pass's leader words (k_compact_hyp zeroes the first set): cleared up front, off the kernels' chain
        if (hipMemsetAsync(ws + L.lead + set_bytes, 0, set_bytes, st) != hipSuccess) return fail(PVV_E_ARG, "hipMemsetAsync(leader words) failed");
        // the caller's event pair spans BOTH count passes (and the refit between them): begin is recorded by the first pass only,
        // end by the second only -- a consumer never sees the estimate's pass alone
        p1.ev_count_end = nullptr;
        pe.ev_count_begin = nullptr;
        plan.p = &p1;
        plan.staged = decide_staged(p, L, st, CountsNeed::ArgMax);
        plan.cols.col0 = 0; plan.cols.hstride = q.hn; plan.cols.lead_set = 0;
        a.plan = &plan;
    }
    if (int e = run_front(&q, L, ws, st, a)) return e;
    V3Out out;
    out.kpt = d_kpt; out.win_counts = d_win_counts; out.hstride = q.hn;
    if (int e = finish_v3(p, L, ws, st, out)) return e;                                 // mean = winner refit over the first hn
    if (est_pass != CountPass::Full) {
        CountCols ec;
        ec.col0 = p->hn; ec.hstride = q.hn; ec.lead_set = 1; ec.mean = d_kpt;
        if (int e = launch_count_any(&pe, L, ws, st, est_pass, ec)) return e;
    }
    return launch_covariance(p, L, ws, st, d_kpt, d_cov, /*d_hyp=*/nullptr, /*d_counts=*/nullptr, d_weights, (int)hn_est, /*hstride=*/q.hn, /*hoff=*/p->hn);
}

PVV_EXPORT int pvv_rerun_count_kernel(const pvv_problem *p, void *d_workspace, size_t workspace_bytes,
                                      int zero_counts, void *stream)
{
    // Re-runs the count pass on the state a previous call left in the workspace.  That call may have been the estimate or
    // the fused un_pnp pass, which need EVERY count: so the pass is re-run in stages only when the caller says so
    // explicitly (PVV_COUNT_STAGED -- the state must then be a v3 call's), never under AUTO.  A staged pass
    // compares PARTIAL counts and therefore needs cleared counters.
    if (p && p->count_kernel == PVV_COUNT_STAGED && !zero_counts)
        return fail(PVV_E_ARG, "a staged count pass needs zero_counts = 1");
    const CountsNeed need = (p && p->count_kernel == PVV_COUNT_STAGED) ? CountsNeed::ArgMax : CountsNeed::All;
    if (int e = validate(p)) return e;
    if (!d_workspace) return fail(PVV_E_ARG, "workspace is NULL");
    Layout L = make_layout(p);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    if (zero_counts) {
        hipError_t e = hipMemsetAsync(ws + L.counts, 0, sizeof(int) * (size_t)p->B * p->K * p->hn, st);
        if (e == hipSuccess && L.lead) e = hipMemsetAsync(ws + L.lead, 0, sizeof(int) * lead_set_words(p), st);
        if (e == hipSuccess && L.miss) e = hipMemsetAsync(ws + L.miss, 0, sizeof(int) * (size_t)p->B * p->K * p->hn, st);
        if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    }
    return launch_count_any(p, L, ws, st, decide_staged(p, L, st, need), CountCols());
}

// ---- streaming-read probe (bench aid; SURVEY 8(d): what a read-once stream reaches on this box) ------------------
namespace {
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(kBlock) void k_stream_read(const u32x4 *__restrict__ src, size_t n16, uint32_t *__restrict__ sink)
{
    // persistent grid, every lane four independent 16-byte loads per trip (64 B in flight per lane), non-temporal: the
    // data is read once
    uint32_t acc = 0;
    const size_t stride = (size_t)gridDim.x * kBlock;
    size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const u32x4 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
        const u32x4 c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
        acc += (a.x ^ a.y ^ a.z ^ a.w) + (b.x ^ b.y ^ b.z ^ b.w) + (c.x ^ c.y ^ c.z ^ c.w) + (d.x ^ d.y ^ d.z ^ d.w);
    }
    for (; i < n16; i += stride) {
        const u32x4 a = __builtin_nontemporal_load(src + i);
        acc += a.x ^ a.y ^ a.z ^ a.w;
    }
    acc = wave_sum(acc);
    if (lane_id() == 0 && acc == 0x9e3779b9u) atomicAdd(sink, acc);   // practically never: the sum only has to be observable
}
}  // namespace

PVV_EXPORT int pvv_stream_read_probe(const void *d_buf, size_t bytes, uint32_t *d_sink, void *stream)
{
    if (!d_buf || !d_sink || bytes < 16 || (bytes & 15) || ((uintptr_t)d_buf & 15)) return fail(PVV_E_ARG, "probe: 16-byte aligned buffer and size");
    hipLaunchKernelGGL(k_stream_read, dim3(num_cus() * 8), dim3(kBlock), 0, (hipStream_t)stream, (const u32x4 *)d_buf, bytes / 16, d_sink);
    return check_launch("k_stream_read");
}

// ---- legacy module surface ---------------------------------------------------------------
static int check_legacy(const void *a, const void *b, const void *c, const void *d, int tn, int vn,
                        int hn)
{
    if (!a || !b || !c || !d) return fail(PVV_E_ARG, "NULL device pointer");
    if (tn < 0 || vn <= 0 || hn < 0) return fail(PVV_E_ARG, "tn, hn must be >= 0 and vn > 0");
    if ((long long)hn * vn >= (1ll << 29) || (long long)tn * vn >= (1ll << 29) ||
        (long long)hn * vn * (long long)(tn > 0 ? tn : 1) >= (1ll << 40))
        return fail(PVV_E_ARG, "problem too large");
    return PVV_OK;
}

typedef void (*legacy_gen_kernel)(const float *, const float *, const int32_t *, float *, int, int, int);

static int legacy_generate(legacy_gen_kernel kernel, const char *name, const float *d_direct, const float *d_coords,
                           const int32_t *d_idxs, float *d_hypo_pts, int tn, int vn, int hn, void *stream)
{
    if (int e = check_legacy(d_direct, d_coords, d_idxs, d_hypo_pts, tn, vn, hn)) return e;
    if (hn == 0) return PVV_OK;
    hipLaunchKernelGGL(kernel, dim3((hn * vn + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, d_direct, d_coords, d_idxs, d_hypo_pts, tn, vn, hn);
    return check_launch(name);
}

PVV_EXPORT int pvv_generate_hypothesis(const float *d_direct, const float *d_coords,
                                       const int32_t *d_idxs, float *d_hypo_pts, int tn, int vn,
                                       int hn, void *stream)
{
    return legacy_generate(k_legacy_gen, "k_legacy_gen", d_direct, d_coords, d_idxs, d_hypo_pts, tn, vn, hn, stream);
}

PVV_EXPORT int pvv_generate_hypothesis_vanishing_point(const float *d_direct, const float *d_coords,
                                                       const int32_t *d_idxs, float *d_hypo_pts,
                                                       int tn, int vn, int hn, void *stream)
{
    return legacy_generate(k_legacy_gen_vp, "k_legacy_gen_vp", d_direct, d_coords, d_idxs, d_hypo_pts, tn, vn, hn, stream);
}

static void legacy_vote_shape(int tn, int vn, int hn, dim3 *grid, int *h_per_block)
{
    // enough blocks to fill 256 CUs, few enough that each thread amortises its pixel load
    int tiles = (tn + kBlock - 1) / kBlock;
    int hz = 1;
    while ((long long)tiles * vn * hz < 4096 && hz < hn) hz <<= 1;
    if (hz > hn) hz = hn;
    if (hz > 65535) hz = 65535;
    *h_per_block = (hn + hz - 1) / hz;
    *grid = dim3(tiles, vn, (hn + *h_per_block - 1) / *h_per_block);
}

typedef void (*legacy_vote_kernel)(const float *, const float *, const float *, uint8_t *, int, int, int, int, float);

static int legacy_vote(legacy_vote_kernel kernel, const char *name, const float *d_direct, const float *d_coords,
                       const float *d_hypo_pts, uint8_t *d_inliers, int tn, int vn, int hn, float inlier_thresh, void *stream)
{
    if (int e = check_legacy(d_direct, d_coords, d_hypo_pts, d_inliers, tn, vn, hn)) return e;
    if (vn > 65535) return fail(PVV_E_ARG, "vn > 65535");
    if (hn == 0 || tn == 0) return PVV_OK;
    dim3 grid; int hpb;
    legacy_vote_shape(tn, vn, hn, &grid, &hpb);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, d_direct, d_coords,
                       d_hypo_pts, d_inliers, tn, vn, hn, hpb, inlier_thresh);
    return check_launch(name);
}

PVV_EXPORT int pvv_voting_for_hypothesis(const float *d_direct, const float *d_coords,
                                         const float *d_hypo_pts, uint8_t *d_inliers, int tn, int vn,
                                         int hn, float inlier_thresh, void *stream)
{
    return legacy_vote(k_legacy_vote, "k_legacy_vote", d_direct, d_coords, d_hypo_pts, d_inliers, tn, vn, hn, inlier_thresh, stream);
}

PVV_EXPORT int pvv_voting_for_hypothesis_vanishing_point(const float *d_direct, const float *d_coords,
                                                         const float *d_hypo_pts, uint8_t *d_inliers,
                                                         int tn, int vn, int hn, float inlier_thresh,
                                                         void *stream)
{
    return legacy_vote(k_legacy_vote_vp, "k_legacy_vote_vp", d_direct, d_coords, d_hypo_pts, d_inliers, tn, vn, hn, inlier_thresh,
                       stream);
}

PVV_EXPORT int pvv_count_inliers(const float *d_direct, const float *d_coords, const float *d_hypo_pts,
                                 int32_t *d_counts, int tn, int vn, int hn, float inlier_thresh,
                                 void *stream)
{
    if (int e = check_legacy(d_direct, d_coords, d_hypo_pts, d_counts, tn, vn, hn)) return e;
    if (hn == 0) return PVV_OK;
    hipStream_t st = (hipStream_t)stream;
    hipError_t me = hipMemsetAsync(d_counts, 0, sizeof(int) * (size_t)hn * vn, st);
    if (me != hipSuccess) return fail((int)me, hipGetErrorString(me));
    if (tn == 0) return PVV_OK;
    CountArgs a;
    a.coords = (const float2 *)d_coords;
    a.dirs = (const float2 *)d_direct;
    a.hyps = (const float2 *)d_hypo_pts;
    a.counts = d_counts;
    a.tn_arr = nullptr;
    a.c_b = 0;
    a.d_b = 0; a.d_v = 1; a.d_p = vn;      // direct[ti,vi]
    a.h_b = 0; a.h_v = 1; a.h_h = vn;      // hypo[hi,vi], counts[hi,vi]
    a.tn_fixed = tn;
    a.B = 1; a.K = vn; a.hn = hn;
    a.thresh = inlier_thresh;
    return launch_count(a, st);
}

// crop.hpp, augment.hpp, ct_augment.hpp and tless_augment.hpp include what they share (warp.hpp, train.hpp, ct_augment.hpp): their
// place in this list carries no meaning.

// ---- detector decode, crops and the way back (ABI v8, additive) --------------------------
#include "crop.hpp"

// ---- DCNv2 modulated deformable convolution, forward (ABI v8, additive) -------------------
#include "dcn.hpp"

// ---- model metadata: farthest point sampling, bounds, diameter (ABI v8, additive) ----------
#include "model.hpp"

// ---- training: vote targets and the PVNet loss, forward and backward (ABI v8, additive) -----
#include "train.hpp"

// ---- detector training: heat-map targets and the detector loss, forward and backward (ABI v8, additive) -----
#include "ct_train.hpp"

// ---- DCNv2 modulated deformable convolution, backward (ABI v8, additive) -------------------
#include "dcn_train.hpp"

// ---- training augmentation: rotate, crop, resize, blur, colour jitter, normalise (ABI v8, additive) -----
#include "augment.hpp"

// ---- detector augmentation: cut-and-paste, warp, colour steps, boxes on the output map (ABI v8, additive) -----
#include "ct_augment.hpp"

// ---- T-LESS PVNet augmentation: rotated cut-outs, occlusion, the crop around the target (ABI v8, additive) -----
#include "tless_augment.hpp"

// ---- colour renders: shaded images, instance labels and depth of a batch of scenes (ABI v8, additive) -----
#include "render.hpp"

// ---- detector evaluation: COCO box AP, map, match and accumulate (ABI v8, additive) -----
#include "det_eval.hpp"

// ---- optimizer step: clipped Adam / RAdam / SGD for all parameter tensors in one launch (ABI v8, additive) -----
#include "optim.hpp"

// ---- PVNet output head: upsample, cat, conv3x3, BatchNorm, LeakyReLU, conv1x1 in one launch (ABI v8, additive) -----
// head_tile.hpp: the 8 x 32 tile the three kernels share; then the two modes pvv_head_forward (head.hpp) branches into:
// the stage mode -- PVNet's decoder stages, the channels in chunks --, the bfloat16 matrix-core mode, and the stage's
// bfloat16 mode (after head_bf16.hpp: it takes head_pack8 and the operand layout from there)
#include "head_tile.hpp"
#include "head_stage.hpp"
#include "head_bf16.hpp"
#include "head_stage_bf16.hpp"
#include "head.hpp"
