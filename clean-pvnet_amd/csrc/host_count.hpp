// host_count.hpp -- host side, part 3: launch policy of the count pass (exact, matrix-core full, matrix-core in stages).
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace); see that file
// for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py).
#pragma once

int launch_count(const CountArgs &a, hipStream_t st)
{
    const int grid = num_cus() * 8;
    if (a.hn <= 64)
        hipLaunchKernelGGL(k_count_inliers<1>, dim3(grid), dim3(kBlock), 0, st, a);
    else if (a.hn <= 128)
        hipLaunchKernelGGL(k_count_inliers<2>, dim3(grid), dim3(kBlock), 0, st, a);
    else if (a.hn <= 256)
        hipLaunchKernelGGL(k_count_inliers<4>, dim3(grid), dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL(k_count_inliers<8>, dim3(grid), dim3(kBlock), 0, st, a);
    return check_launch("k_count_inliers");
}

Bf16Consts bf16_consts(float thresh)
{
    const double T = (double)thresh, s2 = 1.0 - T * T, kappa = T / std::sqrt(s2);
    const double u = 0x1p-24;
    Bf16Consts fc;
    // (round 3: the unit normals come from v_rsq_f32, components within 4u instead of the 3u of sqrt + divide: 32 -> 33,
    // 34 -> 35 in the first level, 6 -> 8 in the second)
    fc.beta = (float)(1.25 * (33.0 * (1.0 + kappa) + 8.0 / s2) * u / T);
    fc.eps_c = (float)(1.25 * (1.0 + kappa) * 35.0 * u);
    fc.eps0 = (float)(1.5e-6 * (1.0 + kappa));
    fc.kappa = (float)kappa;
    // second level: d exact-path's own, nh/B computed in f32 (<= 4u / 5u relative), one fma each => 8u(1+kappa)|d|
    fc.beta2 = (float)(1.25 * (8.0 * (1.0 + kappa) + 8.0 / s2) * u / T);
#ifdef PVV_TUNING
    // timing experiments only (tools/build_variant.sh -DPVV_TUNING); != 1 voids the exactness guarantee
    static const char *dbg = getenv("PVV_DEBUG_BAND_SCALE");
    if (dbg && *dbg) {
        const float k = (float)atof(dbg);
        fc.beta *= k; fc.eps_c *= k; fc.eps0 *= k;
    }
#endif
    return fc;
}

// The hypotheses a count pass covers when they are a column range of longer rows: the fused un_pnp call keeps rows of
// hn + hn_est hypotheses (one compaction, one hypothesis launch) and counts [0, hn) as ransac_voting_layer_v3's and [hn, hn + hn_est)
// as the estimate's, each full or in stages as it would be alone.  p->hn is then the number of columns counted, hstride the row.
struct CountCols {
    int col0 = 0;        // first column
    int hstride = 0;     // row length (0: p->hn, whole rows)
    int lead_set = 0;    // which of the workspace's two sets of leader words the pass uses
    const float *mean = nullptr;   // the estimate in stages: [B,K,2] keypoints (device) its second launch orders the chunks by, or nullptr
    // a staged pass whose schedule was chosen ahead of the front kernels (run_front: k_compact_hyp deferred rows against it)
    uint32_t first = 0;                 // the first launch's residues; 0: launch_count_bf16 chooses (stage_schedule)
    const GatherArgs *gather = nullptr; // != nullptr: rows were deferred, the first launch gathers them (G is set by launch_staged)
};

struct StagedLaunch {
    const pvv_problem *p;
    char *ws;
    const Layout *L;
    hipStream_t st;
    Bf16Consts fc;
    long long *dbg;
    int per_cu_first, per_cu_filter, target_first, target_filter;
    CountPass pass;      // StagedEstimate: the estimate's bound (StageArgs.sub_tenth)
    CountCols cols;
};

// Gather blocks added to the first count launch when rows were deferred, per CU.  The host does not know tn, so the number is
// fixed.  A unit (512 rows x K gathers) is three dependent round trips and config 3 at B = 64 has 576 of them; one-process A/B of
// whole calls there, 1 / 2 / 4 per CU: 0.1884 / 0.1883 / 0.1884 ms against the parent's 0.1916; at B = 32 0.1213 / 0.1211 / 0.1210
// against 0.1212 (profiles/deferred_rows_ab.json).  One: a batch whose images all turn out subsampled or small pays a table build
// per gather block for nothing.
constexpr int kGatherBlocksPerCu = 1;

// the three launches of a staged count pass for one chunk schedule (FIRST = the residues mod 8 the first launch counts)
template <uint32_t FIRST>
int launch_staged(const StagedLaunch &a)
{
    const pvv_problem *p = a.p;
    const Layout &L = *a.L;
    char *ws = a.ws;
    hipStream_t st = a.st;
    const Bf16Consts fc = a.fc;
    const float2 *coords = (const float2 *)(ws + L.coords), *dirs = (const float2 *)(ws + L.dirs);
    const float2 *hyps = (const float2 *)(ws + L.hyps) + a.cols.col0;
    int *counts = (int *)(ws + L.counts) + a.cols.col0;
    const int *tn = (const int *)(ws + L.tn);
    int *lead = (int *)(ws + L.lead) + (size_t)a.cols.lead_set * lead_set_words(p);
    StageArgs sa;
    sa.lead = nullptr;
    sa.any_staged = lead + (size_t)p->B * p->K * 8;
    sa.miss = (int *)(ws + L.miss) + a.cols.col0;
    sa.sub_tenth = a.pass == CountPass::StagedEstimate ? 1 : 0;
    sa.hstride = a.cols.hstride;
    sa.mean = (sa.sub_tenth && tuning_int("PVV_PROX", 1) != 0) ? (const float2 *)a.cols.mean : nullptr;
#ifdef PVV_STAMPS
    sa.dbg = tuning_ptr("PVV_DBG_PTR_FILTER");                    // phase census of the second launch (tools/census_filter.py)
#endif
    GatherArgs ga{};
    if (a.cols.gather) {
        ga = *a.cols.gather;
        ga.G = tuning_int("PVV_GATHER_PER_CU", kGatherBlocksPerCu) * num_cus();
    }
    if (ga.G > 0)
        hipLaunchKernelGGL((k_count_bf16<kCountFirst, FIRST, true>), dim3(a.per_cu_first * num_cus() + ga.G), dim3(kBlock), 0, st, coords, dirs, hyps, counts, tn,
                           p->B, p->K, p->hn, p->cap, p->inlier_thresh, fc, a.target_first, a.dbg, sa, ga);
    else
        hipLaunchKernelGGL((k_count_bf16<kCountFirst, FIRST>), dim3(a.per_cu_first * num_cus()), dim3(kBlock), 0, st, coords, dirs, hyps, counts, tn,
                           p->B, p->K, p->hn, p->cap, p->inlier_thresh, fc, a.target_first, a.dbg, sa, ga);
    if (int e = check_launch("k_count_bf16<first>")) return e;
    if (int e = mark(p, PVV_MARK_STAGE0, st)) return e;
    LeadArgs la;
    la.tn_arr = tn; la.coords = coords; la.dirs = dirs; la.hyps = hyps; la.counts = counts; la.lead = lead;
    la.K = p->K; la.hn = p->hn; la.cap = p->cap;
    la.hstride = a.cols.hstride > 0 ? a.cols.hstride : p->hn;
    la.kappa = fc.kappa; la.beta = 2.f * fc.beta2; la.eps = 2.f * fc.eps0;
    la.any_staged = sa.any_staged;
    // shares per (image, keypoint): the largest power of two <= 16 that keeps the grid within one generation of blocks
    // (8 per CU)
    la.nsplit = 16;
    while (la.nsplit > 1 && (long long)p->B * p->K * la.nsplit > 8ll * num_cus()) la.nsplit >>= 1;
    la.nsplit = tuning_int("PVV_LEAD_SPLIT", la.nsplit);
    hipLaunchKernelGGL(k_lead<FIRST>, dim3(p->K * la.nsplit, p->B), dim3(kBlock), 0, st, la);
    if (int e = check_launch("k_lead")) return e;
    if (int e = mark(p, PVV_MARK_PRUNE0, st)) return e;
    sa.lead = lead;
    // round 4: the second launch's items own a RUN of an (image, keypoint)'s remaining chunks and keep eliminating inside it
    // (count_filter_runs.hpp); one generation of blocks, the run length adapts the item count to it.  (Round 3's
    // one-chunk items stay reachable in tuning builds: PVV_FILTER_OLD=1.)
    // With runs of ONE chunk the new items only add their elimination step to round 3's (+2 % per call at config 3, B = 16 / 24):
    // when the images the last call of this shape reported (the stage hint: AUTO only) predict that, round 3's kernel runs.
    const long long rest = p->count_kernel == PVV_COUNT_AUTO ? stage_hint_rest_chunks(p, st, stage_rest_of(FIRST)) : -1;
    // (Only up to 512 hypotheses: with several hypothesis groups a run-owning item walks the survivors of all of them in ONE pass,
    // round 3's items one group each -- config 5 at B = 2, runs of one chunk: round 3's kernel +2.3 % per call.)
    const bool runs = rest < 0 || rest * p->K >= 2ll * a.target_filter || p->hn > 512;
    if (tuning_int("PVV_FILTER_OLD", runs ? 0 : 1) == 0) {
        hipLaunchKernelGGL(k_count_filter_runs<FIRST>, dim3(tuning_int("PVV_GRID_PER_CU_FILTER", 5) * num_cus()), dim3(kBlock), sizeof(int) * (size_t)p->B, st, coords, dirs,
                           hyps, counts, tn, p->B, p->K, p->hn, p->cap, p->inlier_thresh, fc, a.target_filter, tuning_int("PVV_RUN_R", 0), sa);
        return check_launch("k_count_filter_runs");
    }
    hipLaunchKernelGGL((k_count_bf16<kCountFilter, FIRST>), dim3(a.per_cu_filter * num_cus()), dim3(kBlock), 0, st, coords, dirs, hyps, counts, tn,
                       p->B, p->K, p->hn, p->cap, p->inlier_thresh, fc, a.target_filter, a.dbg, sa, GatherArgs{});
    return check_launch("k_count_bf16<filter>");
}

// Is the count grid of the short kind (5 or 15 blocks per CU, whose blocks beyond one resident generation mostly pass through),
// not the 48-per-CU grid of long, uneven items in which every block works?  Rows are deferred only for the short kind: the gather
// blocks live on the slots the first generation frees early, and a grid in which every block works has none to spare (config 5 at
// B = 16, where moreover every image is subsampled and nothing would be deferred: +0.3 % per call when it carried them).
bool count_grid_short(const pvv_problem *p) { return p->hn < 2048 || p->B <= 8; }

// The chunk schedule of a staged pass: the residues mod kStageM its first launch counts.
// The first stage is a QUARTER of the chunks, or an EIGHTH when the problem is so large that the second launch's runs are long
// (measured, one-process A/B of whole calls: -5 % at config 3 / B = 96, -4 % at B = 128, -9 % on config 5 / B = 16, -5 % at its
// B = 8; +2.5 % at config 3 / B = 64, +4.8 % on config 5 / B = 4 with unequal keypoints).  "Long" is a property of the RUNS, not of
// the hypothesis count: x = K * sum(tn) / 512 chunks per block slot of the second launch -- 5.4 at config 3 / B = 64, 8.1 at 96,
// 6.2 / 3.1 on config 5 at B = 8 / 4 -- and the eighth pays from x = 5.8 on.  (Until round 5 the bound was on the work
// K * hn * sum(tn), which told the same for 512 hypotheses and sent config 5's 2048 to the eighth from B = 2 on: the one case
// of tools/auto_regret.py above 1.03.)
// (the ESTIMATE keeps the quarter at every size: its second launch walks the chunks nearest to the keypoint first, and an
// eighth is 1.5 % slower at B = 64, 2-3 % at B = 6-8, +-1 % on config 5 -- profiles/r05_experiments.txt (15))
// It reads the stage hint, which the device may rewrite at any time: a call asks ONCE -- run_front ahead of k_compact_hyp when rows
// are deferred against the schedule (CountCols.first), launch_count_bf16 otherwise.
uint32_t stage_schedule(const pvv_problem *p, hipStream_t st, CountPass pass)
{
    const double sum_tn = (p->count_kernel == PVV_COUNT_AUTO ? stage_work(p, st) : stage_proxy_work(p)) * kStageProxyFg / ((double)p->K * p->hn);
    const double chunks_per_slot = (double)p->K * sum_tn / (4.0 * kBfPixPerWave) / (5.0 * num_cus());
    const bool eighth = tuning_int("PVV_STAGE_EIGHTH", (pass != CountPass::StagedEstimate && chunks_per_slot >= 5.8) ? 1 : 0) != 0;
    return eighth ? kStageFirstEighth : kStageFirst;
}

int launch_count_bf16(const pvv_problem *p, const Layout &L, char *ws, hipStream_t st, CountPass pass, const CountCols &cc)
{
    // persistent blocks per CU (5 are resident): every block builds the item table once, so few blocks are better when
    // items are short (hn <= 512: one hypothesis group per item), more when they are long and uneven; several
    // generations of blocks also stagger the latency-bound prologues against the VALU-bound loops (exactly 5 per CU
    // runs them in lockstep: +11 %).  Measured on MI355X: 15 vs 24 per CU = -2 % at cfg3 (B = 64) and -20 % at B = 1;
    // 48 vs 24 = -1 % at cfg5 (2048 hypotheses).  A single atomic work queue instead of the static round-robin was
    // 12-150 % slower: device-scope atomics on one address serialise at ~20 ns each; an effective grid that gives every
    // block the same NUMBER of items was 6 % slower too -- its stride (32 images' worth of items) lines the near-empty
    // last chunks of all images up in the same blocks.
    const int per_cu_t = tuning_int("PVV_GRID_PER_CU", 0);
    // Item size: the kernel splits (chunk, keypoint) pairs into runs / groups of hypothesis tiles until there are at least
    // 5 items per CU (round-2 sweep, tools/sweep_count.py: against 2 per CU -12 % at B = 8, -8 % at B = 4, -20 % for the
    // 4096-hypothesis estimate at B <= 8, +-0 from B = 24 on).
    const int items_per_cu = tuning_int("PVV_ITEMS_PER_CU", 5);
    // Grid: up to ~2000 items one generation of blocks (the 5 resident ones per CU, a few of them take two items) -- a
    // block without an item still costs ~1 us (it has to read tn[] to find that out), and three generations of them kept
    // the kernel alive 2 us after the last working block at B = 1; 15 per CU lose 6 % at B = 16 and win 8 % at B = 24.
    // The host does not know tn: up to B = 8 it launches the one generation, beyond that 15 per CU (48 for >= 2048
    // hypotheses: long, uneven items) and the KERNEL falls back to one generation when it finds few items (count_bf16.hpp).
    // (Round 4: when the stage hint knows the tn of the last call of this shape, "few items" is decided on them instead of on B --
    // eight dense 256x256 crops are 3240 (chunk, keypoint) pairs, as many as 34 LINEMOD frames: 15 per CU -3.4 % per call there.)
    bool few = p->B <= 8;
    if (p->count_kernel == PVV_COUNT_AUTO) {
        double sum_tn = -1.0;
        if (stage_hint_mean(p, st, /*max_tn=*/nullptr, &sum_tn) >= 0.f && sum_tn >= 0.0)
            few = sum_tn / (4 * kBfPixPerWave) * p->K * ((p->hn + 511) / 512) <= 2000.0;
    }
    // (not few at B <= 8 -- only the hint can say so --: 15 per CU whatever hn; config 5 at B = 2, staged: 48 per CU +2 %)
    const int per_cu = per_cu_t > 0 ? per_cu_t : (few ? 5 : (count_grid_short(p) ? 15 : 48));
    const float2 *coords = (const float2 *)(ws + L.coords), *dirs = (const float2 *)(ws + L.dirs);
    const float2 *hyps = (const float2 *)(ws + L.hyps) + cc.col0;
    int *counts = (int *)(ws + L.counts) + cc.col0;
    const int *tn = (const int *)(ws + L.tn);
    const Bf16Consts fc = bf16_consts(p->inlier_thresh);
    const int target = tuning_int("PVV_TARGET_ITEMS", items_per_cu * num_cus());
    const int target_first = tuning_int("PVV_TARGET_ITEMS_FIRST", target), target_filter = tuning_int("PVV_TARGET_ITEMS_FILTER", target);
    // the second launch's items are short (a few matrix-core tiles behind the same prologue): one generation of blocks
    // walks them as fast as three (-0.6 % per call at B = 64, -1.8 % at B = 32) and an EMPTY second launch -- a batch of
    // small masks -- costs a third (-1.5 % on config 4 at B = 32)
    const int per_cu_first = tuning_int("PVV_GRID_PER_CU_FIRST", per_cu);
    const int per_cu_filter = tuning_int("PVV_GRID_PER_CU_FILTER", p->hn < 2048 ? 5 : per_cu);
    long long *dbg = tuning_ptr("PVV_DBG_PTR");
    if (pass == CountPass::Full) {
        StageArgs full{};
        full.hstride = cc.hstride;
        hipLaunchKernelGGL(k_count_bf16<kCountFull>, dim3(per_cu * num_cus()), dim3(kBlock), 0, st, coords, dirs, hyps, counts, tn,
                           p->B, p->K, p->hn, p->cap, p->inlier_thresh, fc, target, dbg, full, GatherArgs{});
        return check_launch("k_count_bf16");
    }
    // ransac_voting_layer_v3, staged: count a spread part of the chunks for every hypothesis, bound the winner's count from
    // below through two leaders (k_lead), then the rest only for the hypotheses that can still reach that bound.  Which chunks
    // the first launch counts: stage_schedule.
    StagedLaunch sl;
    sl.p = p; sl.ws = ws; sl.L = &L; sl.st = st; sl.fc = fc; sl.dbg = dbg;
    sl.per_cu_first = per_cu_first; sl.per_cu_filter = per_cu_filter; sl.target_first = target_first; sl.target_filter = target_filter;
    sl.pass = pass;
    sl.cols = cc;
    const uint32_t first = cc.first ? cc.first : stage_schedule(p, st, pass);
    return first == kStageFirstEighth ? launch_staged<kStageFirstEighth>(sl) : launch_staged<kStageFirst>(sl);
}

CountArgs planar_count_args(const pvv_problem *p, const Layout &L, char *ws)
{
    CountArgs a;
    a.coords = (const float2 *)(ws + L.coords);
    a.dirs = (const float2 *)(ws + L.dirs);
    a.hyps = (const float2 *)(ws + L.hyps);
    a.counts = (int *)(ws + L.counts);
    a.tn_arr = (const int *)(ws + L.tn);
    a.c_b = p->cap;
    a.d_b = (long long)p->K * p->cap; a.d_v = p->cap; a.d_p = 1;
    a.h_b = (long long)p->K * p->hn; a.h_v = p->hn; a.h_h = 1;
    a.tn_fixed = 0;
    a.B = p->B; a.K = p->K; a.hn = p->hn;
    a.thresh = p->inlier_thresh;
    return a;
}

int launch_count_any(const pvv_problem *p, const Layout &L, char *ws, hipStream_t st, CountPass pass, const CountCols &cc)
{
    if (p->ev_count_begin && hipEventRecord((hipEvent_t)p->ev_count_begin, st) != hipSuccess)
        return fail(PVV_E_ARG, "ev_count_begin is not a valid hipEvent_t");
    if (!use_bf16_count(p) && (cc.col0 || cc.hstride)) return fail(PVV_E_ARG, "internal: a column range needs the bf16 count kernel");
    const int e = use_bf16_count(p) ? launch_count_bf16(p, L, ws, st, pass, cc) : launch_count(planar_count_args(p, L, ws), st);
    if (e) return e;
    if (p->ev_count_end && hipEventRecord((hipEvent_t)p->ev_count_end, st) != hipSuccess)
        return fail(PVV_E_ARG, "ev_count_end is not a valid hipEvent_t");
    return PVV_OK;
}
