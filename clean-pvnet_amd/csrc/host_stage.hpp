// host_stage.hpp -- host side, part 2: which count kernel, the stage hint, and whether a pass counts in stages.
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace); see that file
// for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py).
#pragma once

// The matrix-core prefilter needs 0 < T < 1 with a sane kappa and pixel coordinates well inside the range where the
// block extents of its guard band are exact; outside [0.5, 0.99995], for huge images, and when the caller asks for it
// (pvv_problem.count_kernel = PVV_COUNT_EXACT: the tests' cross-check) the exact kernel counts.
bool use_bf16_count(const pvv_problem *p)
{
    return p->count_kernel != PVV_COUNT_EXACT && p->inlier_thresh >= 0.5f && p->inlier_thresh <= 0.99995f &&
           p->H <= 16384 && p->W <= 16384;
}

// Staged counting with exact elimination (count_bf16.hpp / count_prune.hpp) is something only ransac_voting_layer_v3
// can use (it keeps the arg-max; the estimate weighs every hypothesis).  may_stage: the workspace reserves the leader
// words (a property of the problem alone, so that pvv_workspace_bytes needs no extra argument); a v3 call whose problem
// may stage takes the staged path.  PVV_COUNT_STAGED forces it wherever the matrix-core kernel is valid, PVV_COUNT_FULL
// forbids it, AUTO stages when the batch is large enough for the two extra launches (k_lead + the second count launch)
// to pay.  The host knows neither tn nor the winners' inlier ratios, so the rule is a proxy for the evaluations of a full
// pass, B*K*hn*H*W >= 2e10 -- measured on MI355X (tools/staged_ab.py): 480x640, K = 9, 512 hypotheses breaks even at
// B = 16 (2.3e10), +4 % at B = 32, +24 % at B = 64; 540x720, K = 17, 2048 hypotheses at B = 16 (2.2e11) +86 % -- and the
// DEVICE refines it per image: images of fewer than 8 chunks (tn <= 3584) are counted completely by the first launch, and
// when no image of the batch is staged the two later launches leave at their first instruction (config 4's sparse masks
// at B = 32: the call then costs ~5 us more than the full pass, the price of not knowing tn on the host).
// Round 4, later: that proxy is calibrated on LINEMOD-like frames (2 % foreground).  T-LESS votes on detector crops (128x128 / 256x256,
// a third of the pixels foreground, B = #detections): 16 crops of 256x256 are 1.7e9 evaluations -- the benchmark's 64
// frames are 1.8e9 -- behind a proxy of 4.8e9, and staging them is worth +34 % per call (profiles/r04_experiments.txt (17)).  So the
// decision now uses the evaluations themselves whenever the stage hint knows the last call's tn (work_equivalent: K*hn*sum(tn) scaled
// to the proxy's units, x 50 = 1 / 0.02), the proxy only before any call has reported; and may_stage -- what reserves the leader words
// and lets a call leave its hint -- asks whether the problem COULD reach the bound: B*K*hn*min(H*W, cap) evaluations at most.
constexpr double kStageMinWork = 2e10;
constexpr double kStageProxyFg = 0.02;      // tn / (H*W) of the frames the proxy and the threshold table were measured on
bool may_stage(const pvv_problem *p)
{
    if (!use_bf16_count(p) || p->count_kernel == PVV_COUNT_FULL) return false;
    if (p->count_kernel == PVV_COUNT_STAGED || p->count_kernel == PVV_COUNT_STAGED_ESTIMATE) return true;
    // cap bounds tn: with fewer than 8 chunks of rows reserved per image nothing can ever be staged (the reference's default
    // call, max_num = 100: 244 rows)
    const double rows = std::min((double)p->H * p->W, (double)p->cap);
    return p->hn >= 128 && p->cap >= kStageMinChunks * 4 * kBfPixPerWave &&
           (double)p->B * p->K * p->hn * rows >= kStageMinWork * kStageProxyFg;
}
double stage_proxy_work(const pvv_problem *p) { return (double)p->B * p->K * p->hn * p->H * p->W; }

// ---------------------------------------------------------------------------------------------
// The stage hint.  Whether staged counting pays depends on how clean the vector field is -- on the winners' inlier ratio
// rho, which the host cannot know before the call: measured on MI355X (tools/staged_ab.py --outlier .., profiles/DESIGN_rounds_1-4.md 4.6),
// 480x640, K = 9, 512 hypotheses at B = 64: +26 % at rho = 0.995, +5 % at 0.95, +-0 at 0.90, -4 % at 0.80 (a quarter of
// the pixels then eliminates nothing and the call pays for the two extra launches); at B = 16 the break-even is rho ~
// 0.97; 540x720, K = 17, 2048 hypotheses gains down to rho = 0.8 and below.  But consecutive calls see similar data (a
// video, a dataset, one network), and every call -- staged or not -- ends with the exact winner counts.  So
// k_finalize_v3 leaves each image's mean winner ratio in a small host-visible array (one per device, pinned, written by
// the GPU with plain stores), and AUTO stages a call only if the ratios the LAST completed calls left there reach a
// threshold that depends on the problem's size.  The hint lags by the calls still in flight and mixes calls when several
// streams interleave (a hint left by another problem SHAPE -- H, W, K, hn; the batch size may vary -- is ignored); it only ever selects between two exact paths.  No data yet (first call, or first
// call under stream capture, where no memory can be pinned): stage.  PVV_COUNT_STAGED / PVV_COUNT_FULL ignore it.
// ---------------------------------------------------------------------------------------------
struct StageHint {
    float *ratio = nullptr;   // 2 x kMaxBatchLds floats, hipHostMalloc: [b] winner ratio (< -1.5 = never written, -1 = skipped
                              // image), [kMaxBatchLds + b] the image's tn
    int n = 0;                // images of the last call that was given the buffer
    int shape[5] = {0, 0, 0, 0, 0};   // B, H, W, K, hn of that call: a hint left by another problem shape is ignored.
                                      // The BATCH SIZE is not part of the shape that must match: a detector hands over a different number
                                      // of crops with every frame; sums over the last call's images are scaled to this call's B
    bool tried = false;
};
StageHint g_hint[kMaxDevices];
std::mutex g_hint_mu;        // guards every field of g_hint[] (the GPU writes only the pinned ratio[] words)

// the device's hint slot, with its pinned array allocated on first use (never while the stream is capturing).  Call with
// g_hint_mu held.
StageHint *stage_hint_locked(hipStream_t st, bool allocate)
{
    const int dev = stream_device(st);
    if (dev < 0) return nullptr;
    StageHint *g = &g_hint[dev];
    if (!g->tried && allocate) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (cs != hipStreamCaptureStatusNone) return nullptr;            // pinning memory is not allowed while capturing
        g->tried = true;
        void *q = nullptr;
        if (hipHostMalloc(&q, sizeof(float) * 2 * kMaxBatchLds, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
        g->ratio = (float *)q;
        if (g->ratio) for (int i = 0; i < 2 * kMaxBatchLds; ++i) g->ratio[i] = -2.f;
    }
    return g->ratio ? g : nullptr;
}

bool hint_same_shape(const StageHint *g, const pvv_problem *p, bool any_hn = false)
{
    return g->shape[1] == p->H && g->shape[2] == p->W && g->shape[3] == p->K && (any_hn || g->shape[4] == p->hn);
}

// A v3 call is about to leave its winners' ratios in the device's slot: record whose they are and hand out the array.
float *stage_hint_claim(const pvv_problem *p, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_hint_mu);
    StageHint *g = stage_hint_locked(st, true);
    if (!g) return nullptr;
    const int shape[5] = {p->B, p->H, p->W, p->K, p->hn};
    if (!hint_same_shape(g, p)) {
        // another problem shape: what the array holds says nothing about this one -- until this call reports, no data
        for (int i = 0; i < p->B; ++i) g->ratio[i] = -2.f;
    } else {
        // more images than the last call had: the new slots hold nothing of this shape until this call reports
        for (int i = g->n; i < p->B; ++i) g->ratio[i] = -2.f;
    }
    memcpy(g->shape, shape, sizeof(shape));
    g->n = p->B;
    return g->ratio;
}

// mean winner ratio of the images the last calls OF THIS SHAPE reported (< 0: no data) and the largest tn among them
// (any_hn: the hint of a v3 call on the same fields with ANOTHER hypothesis count counts too -- the estimate's question)
float stage_hint_mean(const pvv_problem *p, hipStream_t st, float *max_tn = nullptr, double *sum_tn = nullptr, bool any_hn = false)
{
    if (max_tn) *max_tn = -1.f;
    if (sum_tn) *sum_tn = -1.0;
    std::lock_guard<std::mutex> lock(g_hint_mu);
    StageHint *g = stage_hint_locked(st, false);
    if (!g || g->n <= 0) return -1.f;
    if (p && !hint_same_shape(g, p, any_hn)) return -1.f;
    double sum = 0, stn = 0;
    int cnt = 0;
    float mt = 0.f;
    const volatile float *r = g->ratio;
    for (int i = 0; i < g->n; ++i) {
        const float v = r[i];
        if (v < -1.5f) return -1.f;                                       // an image of the last call has not reported yet
        if (v >= 0.f) { sum += v; ++cnt; }
        mt = std::max(mt, (float)r[kMaxBatchLds + i]);
        stn += std::max(0.f, (float)r[kMaxBatchLds + i]);
    }
    if (max_tn) *max_tn = mt;
    if (sum_tn && cnt) *sum_tn = p ? stn * (double)p->B / (double)g->n : stn;   // (scaled to this call's batch size)
    return cnt ? (float)(sum / cnt) : -1.f;
}

// Chunks the SECOND launch of a staged pass would walk, summed over the images the last call of this shape reported (-1: no
// data): the host's preview of the run length k_count_filter_runs will pick (count_filter_runs.hpp).
long long stage_hint_rest_chunks(const pvv_problem *p, hipStream_t st, uint32_t rest_mask)
{
    std::lock_guard<std::mutex> lock(g_hint_mu);
    StageHint *g = stage_hint_locked(st, false);
    if (!g || g->n <= 0) return -1;
    if (!hint_same_shape(g, p)) return -1;
    const volatile float *r = g->ratio;
    long long total = 0;
    constexpr int PC = 4 * kBfPixPerWave;
    for (int i = 0; i < g->n; ++i) {
        if (r[i] < -1.5f) return -1;                                      // an image of the last call has not reported yet
        const int nch = ((int)r[kMaxBatchLds + i] + PC - 1) / PC;
        if (nch >= kStageMinChunks)
            total += (nch / kStageM) * __builtin_popcount(rest_mask) + __builtin_popcount(rest_mask & ((1u << (nch % kStageM)) - 1u));
    }
    return total * p->B / g->n;                                           // (scaled to this call's batch size)
}

// The break-even winner ratio, from one-process A/B measurements of whole calls on MI355X with the round-4 second launch
// (k_count_filter_runs; tools/staged_ab.py --outlier ..., profiles/r04_staged_ab_outliers.json, profiles/DESIGN_rounds_1-4.md 4.7): 480x640, K = 9,
// 512 hypotheses breaks even at rho = 0.990 for B = 16, 0.966 for 24, 0.957 for 32, 0.91 for 48, 0.765 for 64 and below 0.6
// for 128 (round 3's kernel: 0.976 / 0.941 / 0.906 at B = 16 / 32 / 64); 540x720, K = 17, 2048 hypotheses at B = 16 gains at
// every ratio measured (+10 % at 0.71).  Interpolated in x = log2(B*K*hn*H*W / 2.26e10); more hypotheses per keypoint
// lower it further.
float stage_hint_threshold(const pvv_problem *p, double work)
{
    static const double xs[6] = {0.0, 0.585, 1.0, 1.585, 2.0, 3.0}, ys[6] = {0.990, 0.966, 0.957, 0.910, 0.765, 0.50};
    const double x = std::log2(std::max(work, 1.0) / 2.26e10);
    double thr;
    if (x <= xs[0]) thr = ys[0] + (ys[1] - ys[0]) / (xs[1] - xs[0]) * (x - xs[0]);
    else if (x >= xs[5]) thr = ys[5];
    else {
        int i = 0;
        while (x > xs[i + 1]) ++i;
        thr = ys[i] + (ys[i + 1] - ys[i]) * (x - xs[i]) / (xs[i + 1] - xs[i]);
    }
    thr -= 0.1 * std::log2(std::max(p->hn, 512) / 512.0);
    return (float)std::min(0.995, std::max(0.5, thr));
}

// The evaluations of a full pass in the proxy's units (B*K*hn*H*W of a frame with 2 % foreground): K*hn*sum(tn) / 0.02 when the last
// call of this shape has reported its images' tn, the proxy itself otherwise.  *mean / *max_tn: the hint's (see stage_hint_mean).
double stage_work(const pvv_problem *p, hipStream_t st, float *mean = nullptr, float *max_tn = nullptr)
{
    double sum_tn = -1.0;
    float mt = -1.f;
    const float m = stage_hint_mean(p, st, &mt, &sum_tn);
    if (mean) *mean = m;
    if (max_tn) *max_tn = mt;
    if (m < 0.f || sum_tn < 0.0) return stage_proxy_work(p);
    return (double)p->K * p->hn * sum_tn / kStageProxyFg;
}

bool stage_hint_allows(const pvv_problem *p, hipStream_t st)
{
    if (p->count_kernel != PVV_COUNT_AUTO) return true;
    float max_tn = -1.f, m = -1.f;
    const double work = stage_work(p, st, &m, &max_tn);
    if (work < kStageMinWork) return false;                               // too few evaluations for the two extra launches to pay
    if (m < 0.f) return true;                                             // no data yet: by the proxy alone
    // (images of fewer than kStageMinChunks chunks are counted completely by the first launch: when the last calls held
    // no larger one -- config 4's sparse masks -- the two later launches would only be launched to leave again)
    return m >= stage_hint_threshold(p, work) && max_tn > (float)((kStageMinChunks - 1) * 4 * kBfPixPerWave);
}

// The ESTIMATE in stages: estimate_voting_distribution_with_mean weighs every hypothesis whose ratio lies within 0.1 of the best
// (P:262-264), so its count pass may drop what provably falls below that window (stage_bound, count_tile.hpp) when nobody asked
// for the counts themselves.  Covariances and PnP weights are bit-identical to the full pass (tests/test_gpu_staged.py); a third of
// the hypothesis-tile work goes away.  Round 4 measured it exact and NOT faster (1.437 vs 1.402 ms at B = 64, 4096 hypotheses) and
// kept AUTO away from it -- with a second launch that, unnoticed, ran four blocks per CU instead of five (count_filter_runs.hpp:
// its LDS was one allocation granule too large).  With five (round 5, tools/estimate_ab.py, 480x640, K = 9, 4096 hypotheses,
// staged vs full): 1.2385 vs 1.3992 ms at B = 64 (+13 %; +12 % with 9.5 % outlier pixels), 0.657 vs 0.709 at B = 32, 0.369 vs 0.377
// at B = 16, 0.205 vs 0.218 at B = 8, 0.075 vs 0.053 at B = 1; 540x720, K = 17, 2048 hypotheses at B = 16: 1.438 vs 1.532; B = 24 / 48:
// +10 % / +13 %; 2048 hypotheses at B = 64 +8.5 %, 1024 at B = 64 +2 %, at B = 16 -10 %.  On fields with STRUCTURED errors (a third
// of the object voting for a wrong point plus keypoints of very different quality: synth wrong_region / kp_outlier) the gain shrinks
// to +3 % at B = 64 and turns into -6 % at B = 16, -2 % at B = 8 (profiles/r05_experiments.txt (8)).  So AUTO staged an estimate
// only from kEstStageMinWork = 2e11 evaluations-equivalent on (B*K*hn*H*W: 18 LINEMOD frames at 4096 hypotheses, 540x720 / K = 17 /
// 2048 at B = 16) and >= 1024 hypotheses; PVV_COUNT_STAGED_ESTIMATE forces it at every size (the tests' cross-check of the
// bound), PVV_COUNT_FULL forbids it, and PVV_COUNT_STAGED means v3 alone.
// With the chunks of a run walked NEAREST to the keypoint first (count_filter_runs.hpp: a hypothesis' misses sit around the
// keypoint) the staged pass is another 5-7 % faster and wins from 6 LINEMOD frames on: staged / full on clean fields 0.93 at
// B = 6, 0.94 at 8, 0.91 at 12, 0.85 at 24, 0.83-0.85 at 48-64 (1.10 at B = 4); 540x720 / K = 17 / 2048 hypotheses 0.80 at B = 4, 0.76 at
// 8; 9.5 % outlier pixels 0.95-0.96 at 8-16; 30 % outliers 1.00 / 0.99 / 0.88 at 8 / 16 / 64; structured errors 1.05 / 1.07 / 1.00 /
// 0.96 at 8 / 16 / 24 / 64 (profiles/r05_experiments.txt (15)).  What separates those fields is what the v3 call that precedes every
// estimate (resnet18.py:71-72) has just reported: the winners' ratios and the images' tn -- the stage hint of the shape (H, W, K),
// whatever its hn.  With a hint the bound is on the REAL work K * hn * sum(tn) / 0.02: 6e10 for ratios >= 0.95, 9e10 from 0.85 on,
// kEstStageMinWork below; without one the proxy against kEstStageMinWork, as before.
constexpr double kEstStageMinWork = 2e11;
bool est_stage_auto(const pvv_problem *p, hipStream_t st)
{
    if (p->hn < 1024) return false;
    double sum_tn = -1.0;
    float max_tn = -1.f;
    const float rho = stage_hint_mean(p, st, &max_tn, &sum_tn, /*any_hn=*/true);
    if (rho < 0.f || sum_tn < 0.0) return stage_proxy_work(p) >= kEstStageMinWork;
    // (as in stage_hint_allows: when the last calls held no image of kStageMinChunks chunks, the first launch counts everything and
    // k_lead + the second launch would only be launched to leave again)
    if (!(max_tn > (float)((kStageMinChunks - 1) * 4 * kBfPixPerWave))) return false;
    const double work = (double)p->K * p->hn * sum_tn / kStageProxyFg;
    return work >= (rho >= 0.95f ? 6e10 : (rho >= 0.85f ? 9e10 : kEstStageMinWork));
}

// What the caller needs of the counts.
enum class CountsNeed : int {
    All = 0,             // every count (the estimate when its counts are an output, the fused un_pnp pass)
    ArgMax = 1,          // ransac_voting_layer_v3 proper, which keeps the arg-max and may count in stages
    EstimateWindow = 2,  // the estimate without a counts output, which may count in stages against its own bound
};
// How the count pass runs.
enum class CountPass : int {
    Full = 0,
    StagedV3 = 1,        // v3 in stages
    StagedEstimate = 2,  // the estimate in stages
};

// Decided ONCE per call, before the front kernels are launched:
// k_compact_hyp zeroes the miss counters and leader words only for a call that will stage.
CountPass decide_staged(const pvv_problem *p, const Layout &L, hipStream_t st, CountsNeed need)
{
    if (!may_stage(p) || L.lead == 0) return CountPass::Full;
    if (need == CountsNeed::ArgMax && stage_hint_allows(p, st)) return CountPass::StagedV3;
    if (need == CountsNeed::EstimateWindow &&
        (p->count_kernel == PVV_COUNT_STAGED_ESTIMATE || (p->count_kernel == PVV_COUNT_AUTO && est_stage_auto(p, st))))
        return CountPass::StagedEstimate;
    return CountPass::Full;
}
