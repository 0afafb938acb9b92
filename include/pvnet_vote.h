/*
 * pvnet_vote.h -- C ABI of libpvnet_vote.so: clean-pvnet's RANSAC voting hot
 * path as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Every pointer named d_* is a DEVICE pointer (HBM) owned by the caller; the
 * library allocates no device memory, synchronises nothing and launches
 * everything on the `stream` it is given (a hipStream_t passed as void*;
 * NULL = the null stream).  What it does own -- per device, created on first
 * use: 8 KB of pinned host memory (the stage hint) and one side stream with
 * 16 events (the deferred mask of the fused decode) -- pvv_shutdown() gives
 * back.  All entry points return 0 on success and a non-zero code on
 * failure (PVV_E_*; > 0 values are hipError_t from a failed launch);
 * pvv_last_error() returns a thread-local human readable message.  There is
 * no CPU fallback anywhere in this library.
 *
 * Citations are into /root/reference (zju3dv/clean-pvnet):
 *   K = lib/csrc/ransac_voting/src/ransac_voting_kernel.cu
 *   C = lib/csrc/ransac_voting/src/ransac_voting.cpp
 *   P = lib/csrc/ransac_voting/ransac_voting_gpu.py
 */
#ifndef PVNET_VOTE_H_
#define PVNET_VOTE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVV_OK 0
#define PVV_E_ARG (-1)       /* bad shape / size / NULL pointer              */
#define PVV_E_WORKSPACE (-2) /* workspace smaller than pvv_workspace_bytes() */

/* ABI version of this header; pvv_abi_version() must return the same.  (The detector decode, the crops and the way back --
 * pvv_ct_*, pvv_crop_boxes, pvv_uncrop_* at the end of this header -- were added under v8: nothing that existed changed, so
 * the version did not; a host asks for them with dlsym.) */
#define PVV_ABI_VERSION 8

int pvv_abi_version(void);
const char *pvv_last_error(void);

/* ABI v8.  Library lifecycle: releases everything the library created behind the caller's back -- per device the pinned
 * host array of the stage hint (see pvv_stage_hint_query) and the side stream with its events (ABI v7) -- and forgets
 * every hint, so that the next call starts like the first one of a fresh process (it re-creates what it needs).  The
 * side streams are synchronised first; the caller must have no pvv_* call in flight on another thread and should have
 * synchronised the streams it launched on (a kernel still running may write its hint into the array this frees).  Call
 * it before unloading the library or resetting the device, or between workloads to make timing independent of call
 * history.  Returns 0, or the first hipError_t met (everything is released regardless). */
int pvv_shutdown(void);

/* ------------------------------------------------------------------------
 * Legacy extension-module surface: the four functions the reference's
 * pybind module `ransac_voting` exports (C:102-107).  Layouts exactly as the
 * reference: direct [tn,vn,2] f32, coords [tn,2] f32 (x,y), idxs [hn,vn,2]
 * i32, hypo_pts [hn,vn,2|3] f32, inliers [hn,vn,tn] u8 -- all contiguous.
 * ---------------------------------------------------------------------- */

/* Replaces generate_hypothesis (C:20-31 -> K:51-86 -> kernel K:11-49).
 * d_hypo_pts is fully written: (0,0) for degenerate pairs, as at::zeros + the
 * kernel's early return give in the reference (K:42-43,75). */
int pvv_generate_hypothesis(const float *d_direct, const float *d_coords,
                            const int32_t *d_idxs, float *d_hypo_pts, int tn,
                            int vn, int hn, void *stream);

/* Replaces voting_for_hypothesis (C:41-55 -> K:129-167 -> kernel K:88-126).
 * In/out d_inliers: only ever written with 1; the caller pre-zeroes (P:155). */
int pvv_voting_for_hypothesis(const float *d_direct, const float *d_coords,
                              const float *d_hypo_pts, uint8_t *d_inliers,
                              int tn, int vn, int hn, float inlier_thresh,
                              void *stream);

/* Replaces generate_hypothesis_vanishing_point (C:64-75 -> K:231-266 -> K:170-229). */
int pvv_generate_hypothesis_vanishing_point(const float *d_direct,
                                            const float *d_coords,
                                            const int32_t *d_idxs,
                                            float *d_hypo_pts, int tn, int vn,
                                            int hn, void *stream);

/* Replaces voting_for_hypothesis_vanishing_point (C:85-99 -> K:313-351 -> K:268-310). */
int pvv_voting_for_hypothesis_vanishing_point(const float *d_direct,
                                              const float *d_coords,
                                              const float *d_hypo_pts,
                                              uint8_t *d_inliers, int tn,
                                              int vn, int hn,
                                              float inlier_thresh,
                                              void *stream);

/* Fused voting_for_hypothesis + torch.sum(inlier, 2) (P:155-159) on the
 * reference layouts: d_counts [hn,vn] i32, fully written.  No [hn,vn,tn]
 * scratch exists. */
int pvv_count_inliers(const float *d_direct, const float *d_coords,
                      const float *d_hypo_pts, int32_t *d_counts, int tn,
                      int vn, int hn, float inlier_thresh, void *stream);

/* ------------------------------------------------------------------------
 * Batched, sync-free voting layers (replace the per-image Python loops of
 * P:112-199 and P:202-274).  One call = the whole batch, no host read-back.
 * ---------------------------------------------------------------------- */

typedef struct pvv_problem {
    int32_t B, H, W, K;      /* images, rows, cols, keypoints (vn)            */
    int32_t hn;              /* hypotheses per keypoint evaluated in this call */
    int32_t mask_elem_size;  /* bytes per mask element: 1,2,4,8 (bool/intN)   */
    int32_t min_num;         /* P:129 / P:211                                  */
    int32_t max_num;         /* P:135 / P:219                                  */
    int32_t cap;             /* rows reserved per image for compacted pixels;
                                use pvv_default_cap()                          */
    int32_t singular_policy; /* PVV_SINGULAR_*; v3 only                        */
    float inlier_thresh;     /* P:112 / P:202                                  */
    int64_t mask_stride[3];  /* element strides of mask   [B,H,W]              */
    int64_t vertex_stride[5];/* element strides of vertex [B,H,W,K,2] (any view,
                                e.g. the planar permute of resnet18.py:66-68)  */
    uint64_t seed;           /* counter-based RNG key, used when d_idxs /
                                d_selection are NULL                           */
    /* pvv_decode_keypoint_v3 only (ignored elsewhere): the segmentation logits */
    int32_t seg_classes;     /* C of seg [B,C,H,W] (2 for PVNet, config.py:108-112) */
    int32_t first_image;     /* index of image 0 of this call in the caller's larger batch: the device RNG is keyed
                                by (seed, first_image + b), so a batch split over several calls draws the same
                                numbers as one call.  0 for a whole batch (was reserved_, keep 0 if unsure) */
    int64_t seg_stride[4];   /* element strides of seg [B,C,H,W] (a channel slice
                                of the network output, resnet18.py:93)          */
    /* ---- ABI v5 ---- */
    int32_t count_kernel;    /* PVV_COUNT_*: which inlier-count kernel runs; 0 (AUTO) unless cross-checking */
    int32_t flags;           /* PVV_FLAG_* bits (ABI v8; was reserved0: 0 keeps the v7 behaviour) */
    int32_t *d_draws_out;    /* optional DEVICE buffer [B,K,hn,2] i32 (NULL = off): the pixel (y*W + x) each
                                hypothesis' index pair resolved to, -1 where none (image skipped).  Lets a test
                                replay the device RNG's draws through the oracle; for the fused un_pnp call hn is
                                p->hn + hn_est */
    void *ev_count_begin;    /* optional hipEvent_t pair (NULL = off), recorded on `stream` immediately before and   */
    void *ev_count_end;      /* after the inlier-count launch of THIS call: the dominant kernel's duration as it runs
                                inside the pipeline (a measurement aid).  pvv_decode_keypoint_un_pnp counting its rows as
                                two passes records begin before the first and end after the second: the pair then spans
                                v3's count pass, the refit and the estimate's count pass; its PVV_MARK_END (ev_marks) is
                                recorded behind the refit, i.e. BEFORE the estimate's pass */
    /* ---- ABI v6 ---- */
    int32_t *d_status;       /* optional DEVICE buffer [B] i32 (NULL = off): PVV_STATUS_* bits per image, written with tn.
                                The one condition a caller cannot see otherwise is PVV_STATUS_TRUNCATED: the subsample of
                                P:135-138 came out longer than the `cap` rows reserved (beyond 8 sigma with
                                pvv_default_cap) and was cut */
    void **ev_marks;         /* optional HOST array of PVV_N_MARKS hipEvent_t (NULL = off; NULL entries are skipped):
                                recorded on `stream` at the stage boundaries of THIS call (PVV_MARK_*), so that every
                                kernel's duration can be read as it runs inside the pipeline (bench.py's per-kernel
                                rooflines).  A measurement aid: the records cost ~1 us each */
} pvv_problem;

/* pvv_problem.flags (ABI v8) */
#define PVV_FLAG_DEVICE_RNG 1    /* the caller promises d_idxs = d_idxs_est = d_selection = NULL for the call this problem
                                    describes (the device RNG draws everything).  Only then is it known BEFORE the call that
                                    no per-pixel subsample draw is ever stored (small images subsample inside the compaction
                                    kernel and evaluate draws on demand), and pvv_workspace_bytes() leaves the 4 B x H x W per
                                    image of draw storage out: -27 % at 480x640, B = 64.  A call that sets the flag and
                                    passes one of those pointers fails with PVV_E_ARG */
/* 2-byte input fields (ABI v8, additive).  With a vertex bit, d_vertex points to [B,H,W,K,2] float16 / bfloat16 elements
 * (it keeps its `const float *` type: cast), vertex_stride stays in ELEMENTS; the seg bits say the same of d_seg and are
 * read by pvv_decode_keypoint_v3 and pvv_decode_keypoint_un_pnp only.  The kernels widen each element to float32 as they
 * load it -- exact, order-, NaN-, inf- and subnormal-preserving -- so every output is bit-identical to the same call on the
 * float32 copy of the field, and stays float32; nothing is copied and the workspace is the same size.  Setting both bits of
 * one pair fails with PVV_E_ARG.  A library that predates these bits rejects them ("unknown bits in flags" from
 * pvv_workspace_bytes): the feature test for C hosts. */
#define PVV_FLAG_VERTEX_F16 2
#define PVV_FLAG_VERTEX_BF16 4
#define PVV_FLAG_SEG_F16 8
#define PVV_FLAG_SEG_BF16 16

/* pvv_problem.d_status bits */
#define PVV_STATUS_SKIPPED 1     /* foreground_num < min_num: the image's keypoints are zeros (P:129-132 / P:211-216) */
#define PVV_STATUS_SUBSAMPLED 2  /* foreground_num > max_num: pixels were kept with probability max_num/foreground_num  */
#define PVV_STATUS_TRUNCATED 4   /* more rows than `cap`: the list was cut at cap rows (results are those of the cut list) */

/* pvv_problem.ev_marks indices: the event is recorded AFTER the named stage has been enqueued */
#define PVV_MARK_BEGIN 0    /* before the first kernel of the call                                    */
#define PVV_MARK_SCAN 1     /* k_tile_scan (+ k_tile_subsample)                                       */
#define PVV_MARK_COMPACT 2  /* k_compact_hyp                                                          */
#define PVV_MARK_COUNT 3    /* the whole inlier-count pass (both launches and k_lead when staged)     */
#define PVV_MARK_SELECT 4   /* k_select_refit (v3)                                                    */
#define PVV_MARK_END 5      /* k_finalize_v3 / k_covariance: the call is complete                     */
#define PVV_MARK_STAGE0 6   /* staged count only: the first k_count_bf16 launch                       */
#define PVV_MARK_PRUNE0 7   /* staged count only: k_lead                                                 */
#define PVV_N_MARKS 8

/* pvv_problem.count_kernel.  AUTO: the split-bf16 matrix-core prefilter with its guard band wherever it is valid
 * (0.5 <= inlier_thresh <= 0.99995, H and W <= 16384), the exact kernel elsewhere.  EXACT: the reference's own
 * arithmetic (sqrt, divide) for every evaluation -- identical counts, ~9x slower; what the tests cross-check AUTO
 * against.  (Round 1 selected this with an environment variable; the library now reads no environment.) */
#define PVV_COUNT_AUTO 0
#define PVV_COUNT_EXACT 1
/* ABI v7 (round 4) -- no signature changed, three behaviours did:
 *  - the staged count's second launch owns RUNS of an (image, keypoint)'s remaining chunks and eliminates cooperatively
 *    through per-hypothesis miss counters (count_filter_runs.hpp): the workspace reserves them, pvv_workspace_bytes() grew;
 *  - pvv_rerun_count_kernel re-runs the pass in stages only for an explicit PVV_COUNT_STAGED (see there);
 *  - pvv_decode_keypoint_v3 / pvv_decode_keypoint_un_pnp on a two-class seg in two contiguous planes may write d_mask_out
 *    from a second, library-owned HIP stream (one per device, created on first use) that is forked from and joined back
 *    into `stream` inside the call: for the caller everything stays ordered on `stream`.  Not used while `stream` is being
 *    captured into a graph.  (v8: joined back on EVERY exit path, errors included.  There is ONE side stream per device: calls
 *    from several caller streams or threads fork onto it one after the other -- fork, launch and join record are one critical
 *    section -- so the deferred masks of concurrent calls serialise among themselves, and a call's join may wait for a mask
 *    kernel another call queued before it; the voting kernels of different streams stay independent.) */

/* ABI v6.  ransac_voting_layer_v3 keeps only the arg-max of the counts (P:160-167), so pvv_ransac_voting_v3 /
 * pvv_decode_keypoint_v3 may count in STAGES: every hypothesis over a spread quarter of the pixels, then only the
 * hypotheses that can still reach a lower bound of a leader's full count over the rest (k_lead, count_prune.hpp).  Winner,
 * first-index
 * tie rule, winner count and refit are bit-identical to the full pass; what differs is that the counters of eliminated
 * hypotheses hold partial counts (they are not an output of v3).  AUTO stages when the batch is large enough for the
 * two extra launches to pay; FULL = the matrix-core kernel over everything, never staged; STAGED = staged wherever the
 * matrix-core kernel is valid (what the tests force at every size).  The estimate weighs the hypotheses within 0.1 of the best
 * ratio and, since ABI v8, counts in stages against that bound where it pays (AUTO: est_stage_auto -- the stage hint of the v3
 * call that precedes every estimate, from ~6 LINEMOD frames on; pvv_estimate_counts_in_stages tells; never when its counts are
 * an output).  The fused un_pnp call (pvv_decode_keypoint_un_pnp) follows the same rule: where the estimate alone would stage,
 * its rows are counted as TWO passes -- v3's columns, then the estimate's against its bound -- otherwise as one full pass. */
#define PVV_COUNT_FULL 2
#define PVV_COUNT_STAGED 3
/* ABI v8: PVV_COUNT_STAGED stages ransac_voting_layer_v3 only (its v6 meaning; under v7 it also staged an estimate whose
 * counts are not an output).  The estimate counted in stages against its own bound (every hypothesis whose ratio can still
 * come within 0.1 of the best, P:262-264) is exact and, since round 5, faster than the full pass from ~6 LINEMOD frames on
 * (staged / full 0.83-0.85 at B = 24-64, >= 1.0 below 6 frames: DESIGN.md 4.2), which is where AUTO takes it; this value FORCES it
 * at every size: what the tests use to cross-check the bound.  For v3 calls it behaves like PVV_COUNT_STAGED. */
#define PVV_COUNT_STAGED_ESTIMATE 4

/* b_inv (P:97-109) falls back to the identity for the WHOLE image when the
 * batched solve raises; REFERENCE reproduces that (x = ATb for every keypoint
 * of an image that has a singular keypoint), ZERO confines the damage to the
 * singular keypoint, which becomes (0,0). */
#define PVV_SINGULAR_REFERENCE 0
#define PVV_SINGULAR_ZERO 1
/* ransac_voting_layer (v1, P:86-91): torch.inverse raises for the whole image
 * -> every keypoint of that image becomes (0,0). */
#define PVV_SINGULAR_IMAGE_ZERO 2

/* Rows to reserve per image: H*W when max_num >= H*W, otherwise max_num plus
 * 8 sigma of the binomial subsample of P:135-138 (a longer list is truncated). */
int32_t pvv_default_cap(int32_t H, int32_t W, int32_t max_num);

/* Bytes of device scratch the layer calls below need for `p`; the scratch must be
 * 256-byte aligned (any hipMalloc / torch allocation is). */
size_t pvv_workspace_bytes(const pvv_problem *p);

/* ABI v8, additive (ask with dlsym).  Where a layer call on `p` leaves its state inside the workspace, in bytes from its start --
 * read-only knowledge for tests and tools that read the compacted rows back; nothing here is an input of any call.
 *   tn [B] i32 | coords [B,cap] f32x2 | dirs [B,K,cap] f32x2 (planar per keypoint) | hyps [B,K,hn] f32x2 | counts [B,K,hn] i32
 *   deferred [B] i32, 0 = not reserved: the images whose rows outside the first count launch's chunks that launch gathered itself
 *   (a v3 call counted in stages; every row below tn is there once the call has completed, whoever gathered it).
 * Returns PVV_OK, or what pvv_workspace_bytes() would have failed with. */
typedef struct pvv_workspace_offsets {
    size_t tn, coords, dirs, hyps, counts, deferred, total;
} pvv_workspace_offsets;
int pvv_workspace_layout(const pvv_problem *p, pvv_workspace_offsets *out);

/* ransac_voting_layer_v3 (P:112-199).
 *   d_mask      [B,H,W] integer/bool mask, foreground = low byte != 0 (P:125)
 *   d_vertex    [B,H,W,K,2] f32 through p->vertex_stride (f16 / bf16 with PVV_FLAG_VERTEX_F16 / _BF16)
 *   d_idxs      [B,hn,K,2] i32 injected index pairs of P:145, or NULL (device RNG)
 *   d_selection [B,H,W] f32 injected U(0,1) draws of P:136, or NULL (device RNG)
 *   d_out       [B,K,2] f32 keypoint means
 *   d_win_counts[B,K] i32 inlier count of each winner (optional, may be NULL)
 *   d_tn        [B] i32 foreground pixels used per image (optional)
 * The confidence loop of P:150-174 cannot change the result (idxs are drawn
 * once, P:145) and is not executed. */
int pvv_ransac_voting_v3(const pvv_problem *p, const void *d_mask,
                         const float *d_vertex, const int32_t *d_idxs,
                         const float *d_selection, void *d_workspace,
                         size_t workspace_bytes, float *d_out,
                         int32_t *d_win_counts, int32_t *d_tn, void *stream);

/* Resnet18.decode_keypoint (lib/networks/pvnet/resnet18.py:65-76) with the
 * argmax fused into the mask scan: mask = argmax(seg, 1) (first maximum; a NaN
 * logit wins, as torch.argmax) is computed while the foreground is counted, so
 * the int64 mask is written once and never read back.
 *   d_seg       [B,C,H,W] f32 class logits through p->seg_stride (f16 / bf16 with PVV_FLAG_SEG_F16 / _BF16)
 *   d_mask_out  [B,H,W] i64, contiguous: the `mask` entry of the output dict
 *               (resnet18.py:72,76); may be NULL when the caller does not need it
 * everything else as pvv_ransac_voting_v3 (foreground = class != 0). */
int pvv_decode_keypoint_v3(const pvv_problem *p, const float *d_seg,
                           const float *d_vertex, const int32_t *d_idxs,
                           const float *d_selection, void *d_workspace,
                           size_t workspace_bytes, int64_t *d_mask_out,
                           float *d_out, int32_t *d_win_counts, int32_t *d_tn,
                           void *stream);

/* estimate_voting_distribution_with_mean (P:202-274); p->hn is the TOTAL
 * number of hypotheses (round_num * round_hyp_num, P:231-249).
 *   d_mask      foreground = element == 1 (P:207)
 *   d_idxs      [B,hn,K,2] i32 (the rounds of P:235 concatenated) or NULL
 *   d_mean      [B,K,2] f32
 *   d_cov       [B,K,2,2] f32
 *   d_hyp       [B,K,hn,2] f32 all hypotheses (optional, may be NULL)
 *   d_counts    [B,K,hn] i32 their inlier counts (optional)
 *   d_weights   [B,K,3] f32 (wxx,wxy,wyy) of inv(sqrtm(cov)) (optional): the
 *               per-keypoint weights the evaluators hand to uncertainty_pnp
 *               (lib/evaluators/linemod/pvnet.py:118-130), zeros where
 *               cov[0][0] < 1e-6, any entry is NaN, or cov is not positive definite */
int pvv_estimate_voting_distribution(const pvv_problem *p, const void *d_mask,
                                     const float *d_vertex,
                                     const int32_t *d_idxs,
                                     const float *d_selection,
                                     const float *d_mean, void *d_workspace,
                                     size_t workspace_bytes, float *d_cov,
                                     float *d_hyp, int32_t *d_counts,
                                     int32_t *d_tn, float *d_weights,
                                     void *stream);

/* Resnet18.decode_keypoint with cfg.test.un_pnp (resnet18.py:65-72) as ONE pass:
 *     mask   = argmax(seg, 1)
 *     mean   = ransac_voting_layer_v3(mask, vertex, p->hn, inlier_thresh)        (resnet18.py:71)
 *     kpt, var = estimate_voting_distribution_with_mean(mask, vertex, mean)       (resnet18.py:72, P:202-274)
 * The two layers scan and compact the same mask, so here the mask is scanned once, the foreground compacted once,
 * and ONE hypothesis launch + ONE inlier-count launch cover the p->hn hypotheses of the v3 layer and the hn_est
 * (= ceil(min_hyp_num / round_hyp_num) * round_hyp_num, 4096 by default) of the estimate; the refit reads the
 * first p->hn counts of a row, the covariance the rest.  Results are bit-identical to pvv_decode_keypoint_v3
 * followed by pvv_estimate_voting_distribution on the same draws.
 * Where the estimate alone would count in stages (pvv_estimate_counts_in_stages(p with hn = hn_est): large batches under
 * PVV_COUNT_AUTO, or PVV_COUNT_STAGED_ESTIMATE) the rows are counted as TWO passes over the one compaction instead: the
 * columns [0, p->hn) exactly as pvv_ransac_voting_v3 would count them (in full or in stages, the same rule and stage hint),
 * then, behind the refit, the columns [p->hn, p->hn + hn_est) against the estimate's bound.  Same results, bit for bit.
 * Requires p->seg_classes == 2 (PVNet's seg_dim, config.py:108-112): v3 votes with `mask != 0`, the estimate with
 * `mask == 1` (P:125 vs P:207), which coincide only for a two-class argmax -- PVV_E_ARG otherwise (make the two
 * calls then).  min_num / max_num of p apply to both layers, as in the reference's call (defaults of both).
 *   d_idxs      [B,p->hn,K,2] i32 or NULL      d_idxs_est  [B,hn_est,K,2] i32 or NULL   (device RNG where NULL)
 *   d_kpt       [B,K,2] f32 = mean             d_cov       [B,K,2,2] f32
 *   d_weights   [B,K,3] f32 (wxx,wxy,wyy) of inv(sqrtm(cov)) or NULL (evaluators/linemod/pvnet.py:118-128)
 * workspace: pvv_workspace_bytes_un_pnp(p, hn_est). */
size_t pvv_workspace_bytes_un_pnp(const pvv_problem *p, int32_t hn_est);

/* ABI v8: 1 when pvv_estimate_voting_distribution would count this problem IN STAGES (d_counts == NULL; PVV_COUNT_STAGED_ESTIMATE,
 * or PVV_COUNT_AUTO: from ~2e11 evaluations-equivalent B*K*hn*H*W on -- 18 LINEMOD frames at 4096 hypotheses -- or, once a v3 call
 * on fields of the same H, W, K has reported its winners' ratios and tn on the current device (the stage hint; resnet18.py:71-72
 * runs v3 right before every estimate), from 6e10 of REAL work K*hn*sum(tn)/0.02 on clean fields (6 LINEMOD frames), 9e10 for
 * ratios >= 0.85), 0 when it counts in full, < 0 for an invalid problem.
 * pvv_decode_keypoint_un_pnp applies the same rule to its estimate columns (see there), so a host no longer has to choose
 * between the fused call and the two calls; the query stays for hosts that want to know which pass will run. */
int pvv_estimate_counts_in_stages(const pvv_problem *p);
int pvv_decode_keypoint_un_pnp(const pvv_problem *p, int32_t hn_est, const float *d_seg,
                               const float *d_vertex, const int32_t *d_idxs,
                               const int32_t *d_idxs_est, const float *d_selection,
                               void *d_workspace, size_t workspace_bytes,
                               int64_t *d_mask_out, float *d_kpt, float *d_cov,
                               float *d_weights, int32_t *d_win_counts, int32_t *d_tn,
                               void *stream);

/* Bench aid: SURVEY 8(d)'s "achievable number from a streaming-read microbenchmark on the box".  Reads `bytes` (a
 * multiple of 16) of d_buf once with 16-byte loads per lane from a persistent grid and writes a 4-byte checksum to
 * d_sink (so the loads cannot be elided); bracket it with events on `stream`.  Nothing of the voting path uses it. */
int pvv_stream_read_probe(const void *d_buf, size_t bytes, uint32_t *d_sink, void *stream);

/* The stage hint (ABI v6).  Whether staged counting pays depends on how clean the vector field is -- on the winners'
 * inlier ratio, which nobody knows before the call -- but consecutive calls see similar data, and every v3 call ends with
 * the exact winner counts.  The library therefore keeps, per device, the mean winner ratio (winner count / tn) of every
 * image of the last completed v3 calls in a small pinned array the GPU writes, and PVV_COUNT_AUTO stages a call only if
 * that mean reaches a threshold that depends on the problem's size (host_stage.hpp, stage_hint_threshold; DESIGN.md
 * 4.6-4.7).  The same array carries every image's tn, so the size that decides is the call's real work -- K * hn * sum(tn)
 * evaluations as the last call of this shape reported them (dense detector crops stage at a batch size where sparse full
 * frames do not; "shape" = H, W, K, hn: the batch size may change from call to call, the sums are scaled to it) -- and
 * B*K*hn*H*W, a proxy calibrated on frames with 2 % foreground, only while no call has reported.  The
 * hint lags by the calls in flight and only selects between two exact paths; with no data yet the proxy alone decides;
 * PVV_COUNT_STAGED / PVV_COUNT_FULL ignore it.  This query is for tests, benches and the curious: returns 1 and
 * the mean when data is there (0 and -1 otherwise), and the threshold of `p` (p may be NULL: -1; 2 = a problem with too
 * little work to be staged at all). */
int pvv_stage_hint_query(float *mean_ratio, float *threshold, const pvv_problem *p, void *stream);

/* Bench / profiling aid: re-runs ONLY the inlier-count kernel of the last
 * layer call recorded in `d_workspace` (same problem), so its duration can be
 * bracketed with HIP events on `stream`.  zero_counts != 0 first clears the
 * counters (a separate memset node) so the result stays valid; with 0 nothing
 * but the kernel is enqueued and the counters keep accumulating.  The pass is
 * re-run IN STAGES (both launches and k_lead) only when count_kernel is
 * PVV_COUNT_STAGED explicitly -- the workspace must then hold a v3 call's
 * state and zero_counts must be 1 (the elimination compares partial counts);
 * under AUTO the full kernel runs: the workspace may be the estimate's or the
 * fused un_pnp pass's, which need every count.  `p` must describe the call
 * that filled the workspace INCLUDING `cap` (the offsets depend on it). */
int pvv_rerun_count_kernel(const pvv_problem *p, void *d_workspace,
                           size_t workspace_bytes, int zero_counts,
                           void *stream);

/* ------------------------------------------------------------------------
 * Detector decode, crops and the way back (ABI v8, additive): what the detector -> crop -> PVNet caller of the reference
 * does on the host around the voting layer.  Citations:
 *   D = lib/utils/ct/ct_decode.py     U = lib/utils/data_utils.py     R = lib/networks/ct_pvnet/res.py
 *   T = lib/utils/tless/tless_test_utils.py                           E = lib/evaluators/tless_test/pvnet.py
 * All arithmetic is in the stated order without fused multiply-add; tests/crop_twin.py is the same in numpy, bit for bit.
 * Parity of the two warps with cv2.warpAffine is unpinned (no OpenCV where this was built): the contract is the product's own.
 * ---------------------------------------------------------------------- */
#define PVV_CT_MAX_K 256
#define PVV_CROP_WORKSPACE_PER_BOX 96 /* bytes of 8-byte aligned device scratch pvv_crop_boxes needs per box */

/* Replaces decode_ct_hm with ae = None (D:52-75: nms D:6-12, the two-level topk D:33-49, the rows D:60-69) followed, when
 * `clip` is set, by clip_to_image with the heat map's own H, W (U:373-377 as called in lib/networks/ct/dla.py:20-26).
 *   d_ct_hm     [B,C,H,W] f32, after the sigmoid: finite, >= 0           d_wh  [B,2,H,W] f32
 *   d_ct        [B,K,2] f32 (x, y)      d_detection [B,K,6] f32 (x0, y0, x1, y1, value, class)      d_count [B] i32
 * A peak is a pixel not smaller than any of its 8 neighbours inside its class plane; a candidate is a peak > 0; the rows are the
 * K candidates of an image by descending value, the lower c*H*W + y*W + x first among equals; d_count = min(K, candidates) and
 * the rows from there on are zeros (the reference's depend on torch.topk's tie order among zeros).  1 <= K <= PVV_CT_MAX_K,
 * K <= H*W, C*H*W < 2^31.  Three launches whatever the data; the workspace is 256-byte aligned. */
size_t pvv_ct_workspace_bytes(int B, int C, int H, int W, int K);
int pvv_ct_decode(const float *d_ct_hm, const float *d_wh, int B, int C, int H, int W, int K, int clip, void *d_workspace,
                  size_t workspace_bytes, float *d_ct, float *d_detection, int32_t *d_count, void *stream);

/* Replaces _crop / pvnet_transform (R:14-32, T:57-79) for N boxes: centre and scale (R:16-17), the closed form of
 * get_affine_transform(center, scale, 0, [ow, oh]) (U:123-156), an 8-bit bilinear warp in fixed point with constant border 0
 * in place of cv2.warpAffine(INTER_LINEAR) (R:23), the box blanking of the test loader when has_box_ratio (magnify_box,
 * T:49-54, 65-69) and the normalisation to planar float32 (R:25-27).
 *   d_img [B,H,W,3] u8     d_boxes [N,4] f64 (x0,y0,x1,y1) in image pixels     d_image_index [N] i32
 *   h_mean, h_std: HOST arrays of 3 floats
 *   d_inp [N,3,oh,ow] f32  d_center [N,2] f32  d_scale [N] f32  d_trans [N,2,3] f64 (image -> crop)  d_valid [N] u8
 * A box with a non-finite entry, a float32 scale <= 0 or an image index outside [0, B) is invalid: valid 0, centre, scale
 * and trans zero, the crop normalised zeros. */
int pvv_crop_boxes(const uint8_t *d_img, int B, int H, int W, const double *d_boxes, const int32_t *d_image_index, int N, int ow,
                   int oh, double scale_ratio, int has_box_ratio, double box_ratio, const float *h_mean, const float *h_std,
                   void *d_workspace, size_t workspace_bytes, float *d_inp, float *d_center, float *d_scale, double *d_trans,
                   uint8_t *d_valid, void *stream);

/* Replaces affine_transform(kpt_2d, get_affine_transform(..., inv=1)) (E:233-234): d_trans [N,2,3] f64 as pvv_crop_boxes wrote
 * it is inverted (the operation order of OpenCV's invertAffineTransform; a zero map inverts to zeros) and applied in binary64.
 *   d_kpt_2d [N,K,2] f32, or f64 when kpt_is_f64        d_out [N,K,2] f64 */
int pvv_uncrop_keypoints(const void *d_kpt_2d, int kpt_is_f64, const double *d_trans, int N, int K, double *d_out, void *stream);

/* Replaces cv2.warpAffine(seg, trans_inv, (Wc, Hc), INTER_NEAREST) (E:243-245): d_trans (canvas -> crop) is the
 * destination -> source map, nearest neighbour in fixed point with 10 fractional bits, 0 outside the crop.
 *   d_mask [N,h,w] of mask_elem_size 1 or 8 bytes (the low byte is read)        d_out [N,Hc,Wc] u8 */
int pvv_uncrop_mask(const void *d_mask, int mask_elem_size, int h, int w, const double *d_trans, int N, int Hc, int Wc,
                    uint8_t *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Modulated deformable convolution (DCNv2), forward only (ABI v8, additive): the op every DeformConv of the detector
 * (lib/networks/ct/dla_dcn.py:346-358) runs through lib/networks/dcn_v2.py.  Citations:
 *   I = lib/csrc/dcn_v2/src/cuda/dcn_v2_im2col_cuda.cu        C = lib/csrc/dcn_v2/src/cuda/dcn_v2_cuda.cu
 * Replaces dcn_v2_cuda_forward (C:86-163: the bias broadcast C:97-125, modulated_deformable_im2col_cuda C:133-141 and the
 * batched SGEMM C:143-160) with the column element of I:25-54, 143-189.  Everything is float32:
 *   d_input [B,C,H,W]   d_weight [M,C,kh,kw]   d_bias [M] or NULL (zeros)   d_out [B,M,Ho,Wo]
 *   d_offset: image b at d_offset + b * offset_image_stride, [2*dg*kh*kw, Ho, Wo] contiguous
 *   d_mask:   image b at d_mask   + b * mask_image_stride,   [dg*kh*kw, Ho, Wo] contiguous    (strides in elements, so both
 *             may be views of one tensor)
 *   Ho = (H + 2*pad_h - (dil_h*(kh-1)+1)) / stride_h + 1 in integer division, Wo alike; dg >= 1 divides C.
 *
 * Columns, in this order and without fused multiply-add.  For output pixel (y, x), channel c of deformable group
 * g = c / (C/dg) and tap (i, j), t = i*kw + j:
 *   h = float(y*stride_h - pad_h + i*dil_h) + offset[b, g*2*kh*kw + 2t, y, x]          (I:155, 177)
 *   w = float(x*stride_w - pad_w + j*dil_w) + offset[b, g*2*kh*kw + 2t + 1, y, x]      (I:156, 178)
 *   not (h > -1 && w > -1 && h < H && w < W)  =>  val = 0   (a NaN offset too)         (I:176, 180)
 *   otherwise h0 = floor(h), lh = h - h0, hh = 1 - lh, and w0, lw, hw alike; v1..v4 = input[b, c] at (h0, w0), (h0, w0+1),
 *   (h0+1, w0), (h0+1, w0+1), each 0 unless its row and column pass h0 >= 0, w0 >= 0, h0+1 <= H-1, w0+1 <= W-1;
 *   val = (((hh*hw)*v1 + (hh*lw)*v2) + (lh*hw)*v3) + (lh*lw)*v4                        (I:28-52)
 *   col[k, p] = val * mask[b, g*kh*kw + t, y, x],   k = c*kh*kw + t,   p = y*Wo + x    (I:189)
 * Output: out[b, o, p] = the float32 fmaf chain over k in ascending order from the bias,
 *   acc = bias[o];   for k = 0 .. C*kh*kw - 1:  acc = fmaf(weight[o, k], col[k, p], acc)
 * one rounding per step, no split over k, no second accumulator.  Zero terms (0 * 0) may be added to fill an instruction;
 * they change at most the sign of a zero, so results compare as bit patterns with -0 mapped to +0.  The reference sums the
 * same terms in its BLAS's unspecified order.  tests/dcn_twin.py is this contract in numpy, bit for bit.
 * ---------------------------------------------------------------------- */

/* One fused launch; no column tensor is written.  Per-image element counts must stay below 2^31, B <= 65535. */
int pvv_dcn_forward(const float *d_input, const float *d_weight, const float *d_bias, const float *d_offset,
                    long long offset_image_stride, const float *d_mask, long long mask_image_stride, int B, int C, int H, int W,
                    int M, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                    int deformable_groups, float *d_out, void *stream);

/* The columns alone, for tests: d_col [B, C*kh*kw, Ho*Wo] (fewer than 2^31 elements), one thread per element through the same
 * device function as pvv_dcn_forward. */
int pvv_dcn_columns(const float *d_input, const float *d_offset, long long offset_image_stride, const float *d_mask,
                    long long mask_image_stride, int B, int C, int H, int W, int kh, int kw, int stride_h, int stride_w, int pad_h,
                    int pad_w, int dil_h, int dil_w, int deformable_groups, float *d_col, void *stream);

/* ------------------------------------------------------------------------
 * Modulated deformable convolution (DCNv2), backward (ABI v8, additive): the five gradients of pvv_dcn_forward, the same
 * bits on every run -- no float atomic anywhere.  I and C as in the forward's section.  Replaces dcn_v2_cuda_backward
 * (C:206-335): modulated_deformable_col2im_coord_cuda (I:256-327 with the coordinate weight of I:82-123),
 * modulated_deformable_col2im_cuda (I:197-254 with the gradient weight of I:56-80), the two SGEMMs (C:289-297, C:311-319 on
 * the columns of C:300-307) and the bias SGEMV (C:322-329).  Float32 tensors and strides as in pvv_dcn_forward;
 * d_grad_out [B,M,Ho,Wo] contiguous.  K = C*kh*kw, k = c*kh*kw + t, P = Ho*Wo, p = y*Wo + x, Cg = C/dg; h, w, the window test,
 * h0, w0, the neighbours v1..v4 (0 outside the plane) and the blend weights w1..w4 = hh*hw, hh*lw, lh*hw, lh*lw are the
 * forward's.  No fused multiply-add except where `fmaf` is written; everything float32 unless it says binary64.
 *
 *  1. gcol[b,k,p]: acc = +0; for o = 0 .. M-1: acc = fmaf(weight[o,k], grad_out[b,o,p], acc)       (v_mfma_f32_32x32x2_f32)
 *  2. Per (b, g, t, p), over the channels c = g*Cg .. g*Cg + Cg - 1 ascending, from +0, with gc = gcol[b, c*kh*kw + t, p] and
 *     m = mask[b, g*kh*kw + t, p], and only where the sample lies inside the window (otherwise all three stay exactly +0):
 *       grad_mask   += gc * val,            val = ((w1*v1 + w2*v2) + w3*v3) + w4*v4
 *       grad_off_h  += (ch * gc) * m,       ch = (((0 + (-wl)*v1) + (-wh)*v2) + wl*v3) + wh*v4,   wl = float(w0+1) - w, wh = w - float(w0)
 *       grad_off_w  += (cw * gc) * m,       cw = (((0 + (-hl)*v1) + hl*v2) + (-hh)*v3) + hh*v4,   hl = float(h0+1) - h, hh = h - float(h0)
 *     max_b = the largest |gc * m| of image b over every (k, p), inside the window or not (compared as bit patterns of the
 *     absolute value, so a NaN counts as not finite).
 *  3. grad_input.  max_b not finite: every element of image b is NaN.  max_b = 0: every element is +0.  Otherwise 2^e_b is the
 *     smallest power of two >= max_b, and each neighbour i inside the plane of each sample inside the window contributes
 *       n = rint(binary64(w_i * (gc * m)) * 2^(40 - e_b))      (exact scaling, ties to even, |n| <= 2^40)
 *     to the int64 sum of its element; grad_input = float32(binary64(sum) * 2^(e_b - 40)).  Integer sums do not depend on
 *     their order.  Refused unless kh*kw*P <= 2^22, so that a sum cannot overflow.
 *  4. grad_weight.  Image b's pixels are cut into slabs of PVV_DCN_SLAB; per (b, slab, o, k): acc = +0; for p ascending in the
 *     slab: acc = fmaf(grad_out[b,o,p], col[b,k,p], acc), col the forward's column element (sampled again on the chip).
 *     grad_weight[o,k] = float32 of the binary64 sum of these over (b, slab) ascending, from +0.
 *  5. grad_bias[o]: per image, binary64 lane sums s[l] = sum over p = l, l+256, ... ascending from +0, folded as
 *     s[i] += s[i+w] for w = 128, 64, .., 1; the images' s[0] are added ascending from +0; float32 once.
 * Zero terms (0 * 0) may be added to fill an instruction in 1 and 4: from +0 they change nothing.
 * tests/dcn_train_twin.py is this contract in numpy.
 *
 * Workspace (caller-allocated, 256-byte aligned; nothing is kept between calls; every part 256-byte aligned): binary64 [M,K]
 * and [M] accumulators and 65536 max words, then for `chunk` images at a time gcol f32 [chunk,K,P], the grad_weight partials
 * f32 [chunk, ceil(P/PVV_DCN_SLAB), M, K] and the sums i64 [chunk,C,H,W].  The images go through in chunks; no [B,K,P]
 * tensor exists and the result does not depend on the chunk size.  Nothing is read back; no host synchronisation.
 * ---------------------------------------------------------------------- */
#define PVV_DCN_SLAB 512

/* Host-only; stands for the `ones` and `columns` allocations of C:206-335 (C:247-248).  Bytes for chunks of `chunk_images` images (clamped to [1, B]); <= 0: as many images as fit 256 MiB of per-image
 * parts, one at least.  Negative (PVV_E_ARG) with pvv_last_error set when the sizes are refused. */
long long pvv_dcn_backward_workspace_bytes(int B, int C, int H, int W, int M, int kh, int kw, int stride_h, int stride_w, int pad_h,
                                           int pad_w, int dil_h, int dil_w, int deformable_groups, int chunk_images);

/* Replaces C:206-335 with I:56-123 (the gradient and coordinate weights) and I:197-327 (col2im, col2im_coord).
 * Any of the five outputs may be NULL: its launches are skipped.  d_grad_input [B,C,H,W], d_grad_offset [B,2*dg*kh*kw,Ho,Wo],
 * d_grad_mask [B,dg*kh*kw,Ho,Wo], d_grad_weight [M,C,kh,kw], d_grad_bias [M], all contiguous.  The chunk is the largest that
 * `workspace_bytes` holds; PVV_E_WORKSPACE when it does not hold one image. */
int pvv_dcn_backward(const float *d_input, const float *d_weight, const float *d_offset, long long offset_image_stride,
                     const float *d_mask, long long mask_image_stride, const float *d_grad_out, int B, int C, int H, int W, int M,
                     int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, int deformable_groups,
                     float *d_grad_input, float *d_grad_offset, float *d_grad_mask, float *d_grad_weight, float *d_grad_bias,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * PVNet output head, forward only (ABI v8, additive): the tail of Resnet18.forward (lib/networks/pvnet/resnet18.py:53-59,
 * 90-94) for inference, BatchNorm in eval mode, in one launch with no full-resolution intermediate in memory:
 *   fm = up2storaw(fm)                      UpsamplingBilinear2d(scale_factor=2), [B,C2,h,w] -> [B,C2,H,W]
 *   x  = convraw(cat([fm, x], 1))           Conv3x3(C2+C0 -> M1, padding 1, no bias), BatchNorm2d, LeakyReLU, Conv1x1(M1 -> M2, bias)
 * Inputs, float32:
 *   d_fm: image b at d_fm + b * fm_image_stride, [C2,h,w] contiguous      d_x: image b at d_x + b * x_image_stride, [C0,H,W]
 *   (strides in elements: both may be channel slices of larger tensors; d_x may be NULL when C0 = 0);  H = 2h, W = 2w
 *   d_weight1 [M1, C2+C0, 3, 3], fm's channels first as the cat puts them   d_scale, d_shift [M1]: the folded BatchNorm
 *   d_weight2 [M2, M1]   d_bias2 [M2]        1 <= M1, M2 <= PVV_HEAD_MAX_M,  C2 >= 1,  C0 >= 0
 * Output d_out [B,M2,H,W] contiguous, float32 / float16 / bfloat16 by out_kind.
 *
 * In this order, float32 throughout, no fused multiply-add except where fmaf is written:
 *  Upsample (torch's align_corners=True source index, ATen/native/UpSample.h and the CUDA bilinear kernel), per axis:
 *    r = (n_in > 1 && n_out > 1) ? (float)(n_in-1) / (float)(n_out-1) : 0;   src = r * (float)dst;   i0 = (int)src (never
 *    above n_in-1);   i1 = i0 + (i0 < n_in-1);   l1 = src - (float)i0;   l0 = 1 - l1
 *    u = hl0*(wl0*v00 + wl1*v01) + hl1*(wl0*v10 + wl1*v11),   v_ab = fm[b, c, hi_a, wi_b]
 *    each operation rounded once in the order written; a zero weight still multiplies its sample (a NaN reaches u).
 *  Padding: z = cat([u, x]) has a ring of zeros around it -- not an extrapolated upsample.
 *  Conv1: acc = +0;  for k = c*9 + dy*3 + dx ascending (c over fm's channels, then x's):
 *    acc = fmaf(weight1[o, k], z[b, c, y+dy-1, x+dx-1], acc)            one accumulator, one rounding per step
 *  BatchNorm and activation:  t = fmaf(acc, scale[o], shift[o]);   a = t > 0 ? t : t * negative_slope
 *  Conv2: acc = bias2[o];  for m = 0 .. M1-1 ascending: acc = fmaf(weight2[o, m], a[m], acc)
 *  Store: float32, or rounded to nearest even to float16 / bfloat16 (overflow to Inf).
 * Zero terms (0 * 0) may be added to fill an instruction (a K or M1 that is odd); they change at most the sign of a zero, so
 * results compare as bit patterns with -0 mapped to +0.  The fold of the BatchNorm is host work in binary64:
 *   scale = gamma / sqrt(var + eps),  shift = beta - mean * scale (from the unrounded scale), each rounded once to float32.
 * tests/head_twin.py is this contract in numpy, bit for bit.  Bit parity with torch's own device upsample kernel and with
 * MIOpen's convolution is not claimed: both are free to contract and to reorder.
 * ---------------------------------------------------------------------- */
#define PVV_HEAD_OUT_F32 0
#define PVV_HEAD_OUT_F16 1
#define PVV_HEAD_OUT_BF16 2
#define PVV_HEAD_MAX_M 64

/* One fused launch; no workspace, nothing read back.  Per-image element counts must stay below 2^31, B <= 65535, and the
 * halo of C2+C0 channels must fit a CU's 160 KiB of LDS (about 90 channels).  With PVV_HEAD_STAGE in `out_kind` ("PVNet
 * decoder stage" below) the call stops after the activation, takes any number of channels and M1 up to 128. */
int pvv_head_forward(const float *d_fm, long long fm_image_stride, const float *d_x, long long x_image_stride,
                     const float *d_weight1, const float *d_scale, const float *d_shift, const float *d_weight2,
                     const float *d_bias2, int B, int C2, int C0, int h, int w, int H, int W, int M1, int M2,
                     float negative_slope, int out_kind, void *d_out, void *stream);

/* The upsample alone, for tests: d_u [B,C2,H,W] float32 (at most 2^28 elements), one thread per element through the same
 * device function as pvv_head_forward. */
int pvv_head_upsample(const float *d_fm, long long fm_image_stride, int B, int C2, int h, int w, int H, int W, float *d_u,
                      void *stream);

/* The bfloat16 matrix-core compute mode of the same function (ABI v8, additive, opt-in): PVV_HEAD_COMPUTE_BF16 or-ed into
 * pvv_head_forward's `out_kind`, whose low byte stays the output dtype code -- PVV_HEAD_OUT_BF16 | PVV_HEAD_COMPUTE_BF16 computes
 * and stores in bfloat16.  No symbol is added and no signature changes; without the flag the call is what it was.  Any other bit
 * above the low byte is refused together with an unknown dtype code.  Arguments, limits and refusals are otherwise the same.  One
 * launch, no workspace, no atomics (reruns give the same bytes), nothing read back.  The operands are stated bit for bit:
 *  1. u is the float32 upsample above, unchanged; z = cat([u, x]) inside its ring of zeros, fm's channels first.
 *  2. Conv1's operands are z and weight1.  bf16(v) is float32 v rounded to nearest even to bfloat16 (a NaN keeps its upper bits
 *     and gets the quiet bit); every operand v enters as bf16(v).
 *  3. acc1 is a float32 sum, from +0, of the exact products (v_mfma_f32_32x32x16_bf16).  The ORDER of the sum is not part of
 *     the contract, nor are zero terms added for channel padding.
 *  4. t = fmaf(acc1, scale[o], shift[o]);  a = t > 0 ? t : t * negative_slope, float32 as above.
 *  5. Conv2's operands are a and weight2, rounded as in 2; acc2 is a float32 sum, in any order, of bias2[o] (float32,
 *     not rounded) and the products.
 *  6. Store: float32, or rounded to nearest even to float16 / bfloat16.
 * Because the order is free a result is held to a bound, not to bits: tests/head_bf16_twin.py evaluates 1-6 in binary64 on the
 * bit-exact operands (step 4 rounded to float32) and gives bound_acc, the reach of any float32 summation order, and
 * bound_mode, the distance from the float32 contract's function.  Where every partial sum is exact (the twin's exact-sum
 * cases) the result is pinned bit for bit.  Non-finite values: a NaN operand gives NaN; the NaN outputs and the +-Inf outputs are
 * the twin's.  -0 compares as +0.
 * A split mode (hi = bf16(v), lo = bf16(v - hi), the products hi*hi + hi*lo + lo*hi: near float32) is stated by the twin as
 * "bfloat16x3" but is NOT offered: built on this kernel it measured slower than the float32 launch; the
 * flag 0x200 is kept free for it. */
#define PVV_HEAD_COMPUTE_BF16 0x100

/* PVNet decoder stage: the stage mode of the same function (ABI v8, additive): PVV_HEAD_STAGE or-ed into pvv_head_forward's
 * `out_kind`, whose low byte stays the output dtype code.  No symbol is added and no signature changes; without the flag the
 * call is what it was, every refusal included.  A stage is one of the three steps of Resnet18.forward before the head
 * (lib/networks/pvnet/resnet18.py:31-51, 81-89), for inference, BatchNorm in eval mode, in one launch:
 *   fm = conv8s(cat([xfc, x8s], 1))                  PVV_HEAD_STAGE | PVV_HEAD_SAME_RES: no upsample, 256+128 -> 128
 *   fm = conv4s(cat([up8sto4s(fm), x4s], 1))         PVV_HEAD_STAGE: 128+64 -> 64
 *   fm = conv2s(cat([up4sto2s(fm), x2s], 1))         PVV_HEAD_STAGE: 64+64 -> 32
 * each Conv3x3(C2+C0 -> M1, padding 1, no bias), BatchNorm2d, LeakyReLU: the head without its Conv1x1.  The call stops after
 * the activation: d_out = a, [B,M1,H,W] contiguous, float32 / float16 / bfloat16 by the low byte.  d_weight2, d_bias2 and M2
 * are not read and may be NULL / anything.  The contract is the head's, word for word, up to a:
 *   u = the float32 align_corners=True source index and blend above, one rounding per operation in the order written; under
 *     PVV_HEAD_SAME_RES d_fm is already [C2,H,W] (h = H, w = W) and u = fm.
 *   z = cat([u, x]) inside a ring of zeros, d_fm's channels first; d_x is the skip tensor at output resolution, image b at
 *     d_x + b * x_image_stride, and may be NULL when C0 = 0.
 *   acc = +0;  for k = c*9 + dy*3 + dx ascending over all C = C2 + C0 channels:  acc = fmaf(weight1[o, k], z.., acc)
 *   t = fmaf(acc, scale[o], shift[o]);   a = t > 0 ? t : t * negative_slope;   a is stored.
 * Zero terms (0 * 0) may be added anywhere to fill an instruction or a chunk; results compare as bit patterns with -0 as +0.
 * tests/decoder_twin.py is this contract in numpy, bit for bit.
 * Limits: 1 <= M1 <= PVV_HEAD_STAGE_MAX_M; any C2 >= 1 and C0 >= 0 -- no LDS limit on C2 + C0: the kernel takes the channels
 * in chunks --; per-image element counts below 2^31, B <= 65535; H = 2h and W = 2w, or H = h and W = w under
 * PVV_HEAD_SAME_RES.  Every refusal goes through pvv_last_error before any launch.  One launch on the caller's stream, no
 * workspace, no atomics, nothing read back.
 * PVV_HEAD_STAGE | PVV_HEAD_COMPUTE_BF16 and PVV_HEAD_SAME_RES without PVV_HEAD_STAGE are refused as unknown dtype codes: a
 * bfloat16 stage is not offered under that spelling (PVV_HEAD_STAGE_BF16 below is the stage's compute mode). */
#define PVV_HEAD_STAGE     0x400   /* stop after the activation: out = a, [B,M1,H,W]; d_weight2, d_bias2 and M2 are not read */
#define PVV_HEAD_SAME_RES  0x800   /* only with PVV_HEAD_STAGE: d_fm is already [C2,H,W] (h = H, w = W), no upsample */
#define PVV_HEAD_STAGE_MAX_M 128

/* PVNet decoder stage, compute mode (ABI v8, additive, opt-in): PVV_HEAD_STAGE_BF16 or-ed into `out_kind` beside
 * PVV_HEAD_STAGE, with or without PVV_HEAD_SAME_RES, the low byte still the output dtype code.  The flag is a bit of its own,
 * not PVV_HEAD_STAGE | PVV_HEAD_COMPUTE_BF16: that combination has been a pinned refusal since the stage mode exists, and a
 * caller that relies on the refusal must keep getting it; a new bit changes no answer any earlier call got.  It is valid only
 * beside PVV_HEAD_STAGE: alone, with PVV_HEAD_COMPUTE_BF16, with PVV_HEAD_SAME_RES but no PVV_HEAD_STAGE, or with any other
 * high bit it is refused with the unknown dtype codes.  No symbol is added and no signature changes.  Arguments, limits and
 * refusals are the stage's: M1 <= PVV_HEAD_STAGE_MAX_M, any C2 + C0, d_weight2, d_bias2 and M2 not read.  One launch on the
 * caller's stream, no workspace, no atomics (reruns give the same bytes), nothing read back; weight1 crosses the ABI as the
 * caller's float32 and is rounded inside the launch.  The head's bfloat16 contract above, cut after the activation -- the
 * operands are stated bit for bit:
 *  1. u is the float32 upsample above, unchanged, or u = fm under PVV_HEAD_SAME_RES; z = cat([u, x]) inside its ring of zeros,
 *     d_fm's channels first.
 *  2. z and weight1 each enter as bf16(v): rounded once to nearest even to bfloat16, a NaN quieted.
 *  3. acc is a float32 sum, from +0, of the exact products (v_mfma_f32_32x32x16_bf16).  The ORDER of the sum is not part of the
 *     contract, nor are zero terms added for channel padding.
 *  4. t = fmaf(acc, scale[o], shift[o]);  a = t > 0 ? t : t * negative_slope, float32.
 *  5. Store: a as float32, or rounded to nearest even to float16 / bfloat16.
 * A result is held to a bound, not to bits: tests/decoder_bf16_twin.py evaluates 1-5 in binary64 on the bit-exact operands (t
 * and a rounded to float32) and gives bound_acc, the reach of any float32 summation order, and bound_mode, the distance from
 * the float32 stage.  Where every partial sum is exact (the twin's exact-sum cases) the result is pinned bit for bit.  The NaN
 * outputs and the +-Inf outputs are the twin's.  -0 compares as +0. */
#define PVV_HEAD_STAGE_BF16 0x2000 /* only with PVV_HEAD_STAGE: z and weight1 rounded to bfloat16, the sum's order free */

/* ------------------------------------------------------------------------
 * Optimizer step: the clipped Adam / RAdam / SGD step of every parameter tensor in one launch (ABI v8, additive).  Citations:
 *   T = lib/train/trainers/trainer.py:42-45 (zero_grad, clip_grad_value_(..., 40), optimizer.step)
 *   O = lib/train/optimizer.py:12-27 (make_optimizer: every parameter is a param group of its own)
 *   R = lib/utils/optimizer/radam.py:29-95 (RAdam.step);  torch.optim.Adam (no amsgrad, L2 decay), torch.optim.SGD (momentum)
 * O makes torch's foreach / fused steps run once per tensor; here one launch reads p, g, m, v once and writes p, m, v once for all
 * of them.  Nothing synchronises, nothing is allocated and nothing is kept between calls.
 *
 * The table, built on the host per step and uploaded by the caller: n_tensors rows (pvv_optim_row, 80 bytes, 8-byte aligned)
 * and the chunk prefix, n_tensors + 1 int32: chunk_start[0] = 0, chunk_start[t+1] = chunk_start[t] + ceil(numel_t /
 * PVV_OPTIM_CHUNK), chunk_start[n_tensors] = n_chunks.  Block b works on chunk b - chunk_start[t] of the tensor t with
 * chunk_start[t] <= b < chunk_start[t+1], found by a binary search.  Every row has numel >= 1 (the caller skips empty tensors).
 * p, g, m, v are float32, dense, 4-byte aligned; a chunk whose four addresses are 16-byte aligned moves in 16-byte loads and
 * stores, any other and the last numel % 4 elements one element at a time.  No byte outside [0, numel) of a tensor is touched.
 *
 * The arithmetic contract: float32, one rounding per operation as written, no fused multiply-add, `/` and sqrt correctly rounded,
 * subnormals kept (tests/optim_twin.py is this contract in numpy; the device equals it byte for byte).  The scalars s[] are
 * computed on the host in binary64 by the reference's own expressions and rounded to float32 once; t is the tensor's step count
 * after this step, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t.
 *
 * Clip (PVV_OPTIM_CLIP, c = clip_value >= 0):  g = g < -c ? -c : (g > c ? c : g).  A NaN stays NaN, +-Inf becomes +-c.  The
 *   clamped value is used and not written back to g (clip_grad_value_ writes it: the one deviation from T).
 * PVV_OPTIM_ADAM   s = {wd, 1 - beta1, beta2, 1 - beta2, sqrt(bc2), eps, -(lr / bc1)}
 *   g = g + s0*p;  m = m + s1*(g - m);  v = v*s2 + s3*(g*g);  den = sqrt(v)/s4 + s5;  p = p + s6*(m/den)
 * PVV_OPTIM_RADAM  s = {beta1, 1 - beta1, beta2, 1 - beta2, eps, -wd*lr, -step_size*lr}, N_sma and step_size as R:68-80
 *   v = v*s2 + s3*(g*g);  m = m*s0 + s1*g;
 *   unless PVV_OPTIM_ROW_NO_UPDATE (step_size = -1 of degenerated_to_sgd = False):
 *     if PVV_OPTIM_ROW_DECAY (wd != 0):  p = p + s5*p
 *     if PVV_OPTIM_ROW_ADAPTIVE (N_sma >= 5):  p = p + s6*(m/(sqrt(v) + s4));  else  p = p + s6*m
 * PVV_OPTIM_SGD    s = {wd, momentum, -lr};  v is NULL and not touched
 *   g = g + s0*p;  m = PVV_OPTIM_ROW_FIRST ? g : m*s1 + g  (m is not read on a tensor's first step);  p = p + s2*m
 * PVV_OPTIM_ZERO_GRAD: +0 is stored to every element of g after it is read: the zero_grad() of the next iteration.
 * ---------------------------------------------------------------------- */
#define PVV_OPTIM_CHUNK 8192
#define PVV_OPTIM_ADAM 0
#define PVV_OPTIM_RADAM 1
#define PVV_OPTIM_SGD 2
#define PVV_OPTIM_CLIP 1
#define PVV_OPTIM_ZERO_GRAD 2
#define PVV_OPTIM_ROW_ADAPTIVE 1
#define PVV_OPTIM_ROW_DECAY 2
#define PVV_OPTIM_ROW_NO_UPDATE 4
#define PVV_OPTIM_ROW_FIRST 8

typedef struct pvv_optim_row {
    void *p, *g, *m, *v;        /* device pointers to numel float32 each; v NULL for PVV_OPTIM_SGD */
    long long numel;            /* >= 1 */
    int32_t flags;              /* PVV_OPTIM_ROW_* */
    int32_t reserved;           /* 0 */
    float s[8];                 /* the scalars of the kind, as above; the rest 0 */
} pvv_optim_row;

/* Host-only.  PVV_OPTIM_CHUNK of the built library. */
int pvv_optim_chunk(void);

/* One launch of n_chunks blocks.  d_rows [n_tensors] and d_chunk_start [n_tensors + 1] on the device, as above; `flags` is
 * PVV_OPTIM_CLIP | PVV_OPTIM_ZERO_GRAD or 0.  n_tensors = 0 launches nothing.  Refused with PVV_E_ARG: an unknown kind or flag,
 * n_chunks < n_tensors or >= 2^31, a negative or NaN clip_value with PVV_OPTIM_CLIP, a NULL or misaligned table.  The library
 * cannot check the table's contents: it lives on the device. */
int pvv_optim_step(int kind, const pvv_optim_row *d_rows, const int32_t *d_chunk_start, int n_tensors, long long n_chunks,
                   float clip_value, int flags, void *stream);

/* ------------------------------------------------------------------------
 * Model metadata (ABI v8, additive): from a mesh's vertices to what every later stage consumes -- the farthest-point
 * keypoints (`fps_3d`), the bounding box (`corner_3d`, `center_3d`) and the diameter.  Citations:
 *   F = lib/csrc/fps/src/farthest_point_sampling.cpp    M = lib/utils/vsd/misc.py:139-154 (calc_pts_diameter)
 *   H = tools/handle_custom_dataset.py:19-40 (sample_fps_points, get_model_corners), :94 (the centre)
 * A batch is padded: d_points [B,N,3], cloud b has n_b = d_n[b] points (int32 on the device, each in [1, N]; NULL: every cloud
 * has N).  The padding is never read.  Device pointers, caller-owned workspace (256-byte aligned, at least what the query
 * beside each entry point returns), the stream last; nothing is kept between calls.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= N <= PVV_MODEL_MAX_N, 1 <= B <= PVV_MODEL_MAX_B,
 * B * T <= 2^22 with T = ceil(N / PVV_MODEL_TILE) (the grids are (T, B)); the diameter also B * T * T <= 2^22 (its grid is
 * (T, T, B)); 1 <= sn <= 2^20 and B * sn < 2^31.
 *
 * FPS (F:40-105, 122-160; float32 throughout, in this order, no fused multiply-add):
 *   d2(p, q)    = ((p.x-q.x)*(p.x-q.x) + (p.y-q.y)*(p.y-q.y)) + (p.z-q.z)*(p.z-q.z)
 *   min_dist[i] = FLT_MAX;  chosen[i] = false
 *   pick()      = the lowest i with chosen[i] false and min_dist[i] maximal if that maximum is > 0, otherwise 0    (F:56-73)
 *   d_start == NULL (F:122-160): c = (hi + lo) * 0.5f per coordinate, hi / lo the coordinate-wise max / min of the cloud;
 *                                min_dist[i] = min(d2(p_i, c), FLT_MAX);  cur = pick()
 *   otherwise (F:76-105):        cur = d_start[b] (int32 on the device, in [0, n_b)), in place of F:93-94's rand() % pn
 *   repeat sn times:  chosen[cur] = true;  idx[k] = cur
 *                     if k < sn-1:  for every i not chosen: d = d2(p_i, p_cur); if d < min_dist[i]: min_dist[i] = d
 *                                   cur = pick()
 * "otherwise 0" is F:61-62: once every unchosen point coincides with a chosen one, index 0 repeats, chosen before or not, so
 * sn > n_b is legal.  Inputs are finite; with a non-finite coordinate the indices of that cloud are unspecified but stay in
 * [0, n_b).  PVV_FPS_ONE_BLOCK (N <= PVV_FPS_ONE_BLOCK_MAX) runs the sn rounds in one launch of one workgroup per cloud;
 * PVV_FPS_TILED runs one launch per round over (T, B) workgroups; both give the same indices.  PVV_FPS_AUTO takes ONE_BLOCK
 * where it applies.  No workgroup waits for another in either.
 *
 * Diameter (M:139-154): coordinates taken to binary64 exactly (float32 widened), d2 = (dx*dx + dy*dy) + dz*dz in binary64
 * without fused multiply-add, the result the correctly rounded sqrt of the maximum of d2 over all pairs, a point with itself
 * included (one point, or all equal: 0.0).  A maximum is exact in any order; for float64 input this is calc_pts_diameter's value
 * bit for bit.  Bounds (H:27-29): plain minima and maxima, in the type of the points.  tests/model_twin.py is this contract in numpy.
 * ---------------------------------------------------------------------- */
#define PVV_FPS_AUTO 0
#define PVV_FPS_ONE_BLOCK 1
#define PVV_FPS_TILED 2
#define PVV_FPS_ONE_BLOCK_MAX 8192 /* the largest N PVV_FPS_ONE_BLOCK takes */
#define PVV_MODEL_TILE 1024        /* points per workgroup of the tiled kernels */
#define PVV_MODEL_MAX_N (1 << 20)
#define PVV_MODEL_MAX_B 65535

/* Host-only.  Bytes pvv_fps needs for these sizes and this path; 0 with pvv_last_error set when they are refused. */
size_t pvv_fps_workspace_bytes(int B, int N, int sn, int path);

/* d_idx [B,sn] int32.  d_start == NULL: the centre start (farthest_point_sampling_init_center, F:186-204). */
int pvv_fps(const float *d_points, const int *d_n, const int *d_start, int B, int N, int sn, int path, void *workspace,
            size_t workspace_bytes, int *d_idx, void *stream);

/* Host-only.  Bytes pvv_model_bounds and pvv_model_diameter need; 0 with pvv_last_error set when the sizes are refused. */
size_t pvv_model_workspace_bytes(int B, int N);

/* d_points [B,N,3] float32, or float64 when is_f64; d_lo, d_hi [B,3] of the same type. */
int pvv_model_bounds(const void *d_points, int is_f64, const int *d_n, int B, int N, void *workspace, size_t workspace_bytes,
                     void *d_lo, void *d_hi, void *stream);

/* d_out [B] float64. */
int pvv_model_diameter(const void *d_points, int is_f64, const int *d_n, int B, int N, void *workspace, size_t workspace_bytes,
                       double *d_out, void *stream);

/* ------------------------------------------------------------------------
 * Training augmentation: PVNet's rotate / crop / resize and the loader's transforms for a batch (ABI v8, additive).  Citations:
 *   P = lib/datasets/linemod/pvnet.py:62-78 (augment; lib/datasets/custom/pvnet.py repeats it)
 *   A = lib/datasets/augmentation.py (rotate_instance :60-69, crop_or_padding_to_fixed_size_instance :126-167,
 *       crop_or_padding_to_fixed_size :170-196, crop_resize_instance_v1 :266-295)
 *   X = lib/datasets/transforms.py:29-99 (ToTensor, Normalize, ColorJitter, RandomBlur, make_transforms)
 * Device pointers, caller-owned workspace (8-byte aligned), the caller's stream last; nothing is read back, nothing
 * synchronises, nothing is allocated and nothing is kept between calls.  The kernels draw no random number and evaluate no
 * transcendental function: the caller hands over the drawn values per sample, cos and sin of the degree included.  No fused
 * multiply-add anywhere; every reduction is over integers, so no arrival order enters a result and reruns give the same
 * bytes.  tests/augment_twin.py is this contract in numpy; DESIGN.md section 18 states it in full.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= B <= 65535, sides in [1, 16384], out_size sides in [8, 16384], K <= 65535.
 *
 * pvv_pvnet_augment's params: B records of PVV_AUGMENT_PARAM_BYTES on the device, 8-byte aligned:
 *   binary64 cos, sin, ratio, u_h, u_w;  int32 th = int(oh * ratio), tw = int(ow * ratio)
 * pvv_pvnet_transform's params: B records of PVV_TRANSFORM_PARAM_BYTES on the device:
 *   int32 k (0, 3, 5, 7, 9);  int32 w[9] (the taps centred on w[4], summing to 256);  float32 f[3] (the factors of
 *   brightness, contrast, saturation);  int32 hue (what is added to PIL's 8-bit hue modulo 256: int(factor * 255) & 255);
 *   int32 order[4] (0 brightness, 1 contrast, 2 saturation, 3 hue in the drawn order, -1 for a step that is not applied)
 * ---------------------------------------------------------------------- */
#define PVV_AUGMENT_PARAM_BYTES 48
#define PVV_TRANSFORM_PARAM_BYTES 72

/* Host-only.  Bytes pvv_pvnet_augment needs: a record per sample and the rotated windows [B,max_th,max_tw,3], max_th and max_tw
 * the largest th and tw among the records; 0 with pvv_last_error set when a size is refused. */
size_t pvv_augment_workspace_bytes(int B, int max_th, int max_tw);

/* P:62-78.  d_img [B,H,W,3] uint8, d_mask [B,H,W] uint8 (foreground: != 0), d_kpt_2d [B,K,2] float32 or binary64.  Writes
 * d_out_img [B,oh,ow,3] uint8, d_out_mask [B,oh,ow] uint8, d_out_kpt [B,K,2] binary64, d_path [B] int32 (0 no foreground, 1 the
 * instance branch, 2 the rotated mask is empty: the steps of 0) and d_window [B,6] int32 (th, tw, hbeg, wbeg, pad_h, pad_w).
 * A fill and five launches: the moments, the rotated mask's box, the window with the keypoints, the rotated image inside each
 * window, the output pixels.  A record whose th or tw exceeds max_th or max_tw reads zeros beyond them, never out of bounds. */
int pvv_pvnet_augment(const uint8_t *d_img, const uint8_t *d_mask, const void *d_kpt_2d, int kpt_is_f64, int B, int H, int W, int K,
                      int oh, int ow, double overlap_ratio, const void *d_params, int max_th, int max_tw, void *d_workspace, size_t workspace_bytes,
                      uint8_t *d_out_img, uint8_t *d_out_mask, double *d_out_kpt, int32_t *d_path, int32_t *d_window, void *stream);

/* Host-only.  Bytes pvv_pvnet_transform needs when it is given params: one int64 per image and the blurred batch. */
size_t pvv_transform_workspace_bytes(int B, int h, int w);

/* X:81-90.  d_img [B,h,w,3] uint8 -> d_out [B,3,h,w] float32.  d_params NULL: ToTensor and Normalize only (no workspace
 * needed).  h_mean, h_std: 3 binary64 each on the host.  has_blur / has_contrast: whether any record asks for the step (its
 * launch is skipped otherwise).  With params the sides must be at least 8.  At most a fill and three launches. */
int pvv_pvnet_transform(const uint8_t *d_img, int B, int h, int w, const void *d_params, int has_blur, int has_contrast,
                        const double *h_mean, const double *h_std, void *d_workspace, size_t workspace_bytes, float *d_out,
                        void *stream);

/* ------------------------------------------------------------------------
 * Detector augmentation: the T-LESS detector's training batch from cut-outs and a background, and the detector's input
 * preparation at inference (ABI v8, additive).  Citations:
 *   U = lib/utils/tless/tless_utils.py (augment :18-63, cut_and_paste :86-97)
 *   C = lib/datasets/tless/ct.py:58-70 (Dataset.get_bbox);  C' = lib/datasets/tless_train/ct.py:75-76 (the nearest form)
 *   G = lib/utils/data_utils.py (get_affine_transform :123-156, grayscale :172-173, lighting_ .. contrast_ :176-199,
 *       color_aug :202-210)
 * Device pointers, caller-owned workspace (8-byte aligned), the caller's stream last; nothing is read back, nothing
 * synchronises, nothing is allocated and nothing is kept between calls.  The kernels draw no random number and evaluate no
 * transcendental function.  No fused multiply-add anywhere; the only floating-point sum (the grey mean) is binary64 in a
 * fixed tree, every other reduction is over integers: reruns give the same bytes.  Every source tap is tested against its
 * image in 64 bits before an address is formed.  tests/ct_augment_twin.py is this contract in numpy; DESIGN.md section 19
 * states it in full.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= B <= 65535, sides in [1, 16384], 1 <= N <= PVV_CT_AUGMENT_MAX_N.
 *
 * pvv_ct_augment's params: B records of PVV_CT_AUGMENT_PARAM_BYTES on the device, 8-byte aligned:
 *   binary64 inv_in[6] (the inverse of trans_input), inv_out[6] (of trans_output), light[3] (eigvec . (eigval * alpha));
 *   float32 a[3], oma[3] (alpha and 1 - alpha of the three colour steps in the drawn order, each rounded to float32);
 *   int32 order[3] (0 brightness, 1 contrast, 2 saturation in the drawn order), int32 padding
 * ---------------------------------------------------------------------- */
#define PVV_CT_AUGMENT_MAX_N 16
#define PVV_CT_AUGMENT_PARAM_BYTES 160
#define PVV_CT_BOXES_LINEAR 0
#define PVV_CT_BOXES_NEAREST 1

/* U:86-97 for every instance of a batch.  d_bg [B,H,W,3] uint8, d_inst_img [B,N,h,w,3] uint8, d_inst_mask [B,N,h,w] uint8
 * (the object: != 0), d_num [B] int32 (instances n >= num[b] are skipped), d_place_u [B,N,2] binary64 in [0, 1): the uniforms
 * of dst_y and dst_x.  Writes d_img [B,H,W,3] uint8, d_label [B,H,W] uint8 (0 background, n + 1 instance n) and d_place [B,N,6]
 * int32 (y_min, x_min, h, w, dst_y, dst_x; h = y_max - y_min, w = x_max - x_min as U:90 has them; a skipped instance -- beyond
 * num[b] or with an empty mask, where the reference raises -- is (0, 0, -1, -1, 0, 0)).  randint(lo, hi) = lo + floor(u * (hi - lo))
 * for hi > lo, lo otherwise (an instance larger than the canvas: its pixels outside the canvas are dropped).  Two launches:
 * the boxes with the placements, then one lane per canvas pixel that walks the instances from the last to the first and takes
 * the first whose mask covers it -- a gather: every pixel has one owner, no atomics. */
int pvv_ct_compose(const uint8_t *d_bg, const uint8_t *d_inst_img, const uint8_t *d_inst_mask, const int32_t *d_num,
                   const double *d_place_u, int B, int H, int W, int N, int h, int w, uint8_t *d_img, uint8_t *d_label,
                   int32_t *d_place, void *stream);

/* Host-only.  Bytes pvv_ct_augment needs: the box accumulators [B,N,4] int32, one binary64 grey partial per (image, 64 x 4
 * tile of the input) and the grey means; 0 with pvv_last_error set when a size is refused. */
size_t pvv_ct_augment_workspace_bytes(int B, int N, int ih, int iw);

/* U:46-63 and C:58-70 for a batch.  d_img [B,H,W,3] uint8 -> d_orig [B,ih,iw,3] uint8 (the 8-bit bilinear warp of
 * pvv_crop_boxes through inv_in, zero border) and d_inp [B,3,ih,iw] float32: with train != 0 the colour steps of G:202-210 on
 * float32(orig) / 255 (grey = (c0 * 0.114f + c1 * 0.587f) + c2 * 0.299f, its mean the binary64 fixed-tree sum divided by ih * iw
 * and rounded once to float32; all three steps use the grey and the mean of the image before any step; the lighting vector is
 * added in binary64 and rounded once), then (x - mean) / std in float32; with train == 0 the normalisation alone.  h_mean,
 * h_std: 3 float32 each on the host.  d_label [B,H,W] uint8 (NULL: no boxes, N and d_boxes are ignored) -> d_boxes [B,N,4]
 * int32 (x, y, x2, y2) on the oh x ow output map: an output pixel belongs to instance i iff, PVV_CT_BOXES_LINEAR, one of the
 * four taps of the 8-bit bilinear rule through inv_out with a non-zero weight carries label i + 1 (= warpAffine(float mask,
 * INTER_LINEAR) != 0) or, PVV_CT_BOXES_NEAREST, the tap of the nearest rule of pvv_uncrop_mask does; then
 * (xmin, ymin, min(xmax + 1, ow - 1), min(ymax + 1, oh - 1)) as boundingRect and C:67-68 give it, (0, 0, 0, 0) for an instance
 * without a pixel.  A fill and at most five launches. */
int pvv_ct_augment(const uint8_t *d_img, const uint8_t *d_label, int B, int H, int W, int N, int ih, int iw, int oh, int ow,
                   int train, int boxes_mode, const void *d_params, const float *h_mean, const float *h_std, void *d_workspace,
                   size_t workspace_bytes, uint8_t *d_orig, float *d_inp, int32_t *d_boxes, void *stream);

/* ------------------------------------------------------------------------
 * T-LESS PVNet augmentation: the T-LESS PVNet loader's training sample from a rotated target cut-out, rotated distractor
 * cut-outs and a background, and its crop around what is left of the target (ABI v8, additive).  Citations:
 *   T = lib/utils/tless/tless_train_utils.py (cut_and_paste :94-120, get_fused_image :123-136, rotate_image :153-172)
 *   U = lib/utils/tless/tless_utils.py:86-97 (cut_and_paste)
 *   D = lib/datasets/tless_train/pvnet.py (read_data :60-69, get_training_img :73-105, __getitem__ :113-116)
 *   V = lib/utils/tless/tless_pvnet_utils.py (magnify_box :13-18, augment :21-73)
 *   G = lib/utils/data_utils.py (affine_transform :159-162, color_aug :202-210)
 * The rules of "Detector augmentation" hold: device pointers, caller-owned workspace (8-byte aligned), the caller's stream last;
 * nothing is read back, nothing synchronises, nothing is allocated or kept; no random number and no transcendental function on
 * the device; no fused multiply-add; the grey mean is the only floating-point sum (binary64, fixed tree); every other reduction
 * is over integers; every source tap is tested against its image in 64 bits before an address is formed.
 * tests/tless_augment_twin.py is this contract in numpy; DESIGN.md section 22 states it in full.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= B <= 65535, sides in [1, 16384], 0 <= N <= PVV_TLESS_MAX_N, K <= 65535.
 *
 * A cut-out's record, PVV_TLESS_CUT_BYTES on the device, 8-byte aligned, built by the host in binary64 (T:154-165):
 *   binary64 M[6]   getRotationMatrix2D((w / 2, h / 2), angle, 1) with M[2] += bound_w / 2 - w / 2, M[5] += bound_h / 2 - h / 2
 *   binary64 inv[6] its inverse in invertAffineTransform's operation order
 *   int32 bound_h = int(h |cos| + w |sin|), bound_w = int(h |sin| + w |cos|), two int32 of padding
 * Both bounds are <= pvv_tless_rotate_side(h, w) = floor(sqrt(h^2 + w^2)).
 * ---------------------------------------------------------------------- */
#define PVV_TLESS_MAX_N 16
#define PVV_TLESS_CUT_BYTES 112

/* Host-only.  D, the side of the square plane a rotated h x w cut-out is stored in; 0 for sides outside [1, 16384]. */
int pvv_tless_rotate_side(int h, int w);

/* T:153-172 for P cut-outs: d_src [P,h,w,channels] uint8, channels 1 or 3, d_cuts P records -> d_out [P,D,D,channels]: inside
 * bound_w x bound_h the warp through inv with zero border -- nearest == 0: the 8-bit bilinear rule of pvv_crop_boxes (what the
 * reference's call does: its INTER_NEAREST stands in the position of dst, so the flags keep their default); nearest != 0: the
 * rule of pvv_uncrop_mask -- and zero outside.  One launch. */
int pvv_tless_rotate(const uint8_t *d_src, const void *d_cuts, int P, int h, int w, int channels, int D, int nearest,
                     uint8_t *d_out, void *stream);

/* Host-only.  Bytes pvv_tless_compose needs: the accumulators, a coverage byte per canvas pixel and the rotated masks of the
 * 1 + N cut-outs (one byte per pixel of their D x D planes); 0 with pvv_last_error set when a size is refused. */
size_t pvv_tless_compose_workspace_bytes(int B, int N, int H, int W, int ht, int wt, int ho, int wo);

/* D:73-105 for a batch.  d_bg [B,H,W,3], d_fused_bg [B,H,W,3] or NULL (= d_bg), d_img [B,ht,wt,3], d_mask [B,ht,wt],
 * d_other_img [B,N,ho,wo,3], d_other_mask [B,N,ho,wo], all uint8; d_kpt [B,K,2] binary64; d_num [B] int32 or NULL (= N):
 * distractors n >= num[b] are skipped; d_cuts [B,1+N] records, the target's first; d_place_u [B,1+N,2] binary64 in [0, 1), the
 * uniforms of dst_y and dst_x; d_flags [B,2] int32: target on top by draw (D:93), black fused background (T:95).
 * The masks are rotated as one-channel images (T:115, D:65); a rotated cut-out covers where its rotated mask != 0, its box and
 * placement are U:87-93 with randint(lo, hi) = lo + floor(u (hi - lo)) for hi > lo, lo otherwise; pixel_num is the sum of the
 * rotated target mask's values (D:74).  Keypoints: (M . kpt - (x_min, y_min)) + (dst_x, dst_y) (D:66, 80-82).  The fused canvas
 * is d_fused_bg or black with the distractors pasted in order, later over earlier (T:105-118).  visible = the target's pixels
 * that no distractor covers (D:96-97).  path: 0 the target over the fused canvas by draw; else 1 the distractors over the
 * target on d_bg when (double)visible / (double)pixel_num >= ratio; else 2 as 0; 3 a target whose rotated mask is empty (the
 * reference raises): the fused canvas, an empty mask.  ratio > 0.  Colours are sampled through inv when a pixel's owner is
 * known; rotated images are not stored.  Writes d_out_img [B,H,W,3], d_out_mask [B,H,W] (0 / 1), d_out_kpt [B,K,2],
 * d_bbox [B,4] int32 (x, y, x + w - 1, y + h - 1 of the mask, D:102-103; the whole canvas for an empty mask), d_path [B] int32,
 * d_place [B,1+N,6] int32 (y_min, x_min, h, w, dst_y, dst_x; (0, 0, -1, -1, 0, 0) for a skipped or empty cut-out) and
 * d_visible [B,2] int64 (visible, pixel_num).  A fill and at most six launches. */
int pvv_tless_compose(const uint8_t *d_bg, const uint8_t *d_fused_bg, const uint8_t *d_img, const uint8_t *d_mask,
                      const double *d_kpt, const uint8_t *d_other_img, const uint8_t *d_other_mask, const int32_t *d_num,
                      const void *d_cuts, const double *d_place_u, const int32_t *d_flags, int B, int H, int W, int N, int K,
                      int ht, int wt, int ho, int wo, int nearest, double ratio, void *d_workspace, size_t workspace_bytes,
                      uint8_t *d_out_img, uint8_t *d_out_mask, double *d_out_kpt, int32_t *d_bbox, int32_t *d_path,
                      int32_t *d_place, long long *d_visible, void *stream);

/* Host-only.  Bytes pvv_tless_augment needs: a record per sample, one binary64 grey partial per (image, 64 x 4 tile of the
 * input) and the grey means; 0 with pvv_last_error set when a size is refused. */
size_t pvv_tless_augment_workspace_bytes(int B, int ih, int iw);

/* V:21-73 (train) and D:115-116 for a batch.  d_img [B,H,W,3], d_mask [B,H,W] uint8, d_kpt [B,K,2] binary64, d_bbox [B,4] int32
 * (x0, y0, x1, y1) on the device; d_factor [B] float32, the drawn scale factor; d_box_ratio [B] binary64; d_colour: B records of
 * PVV_CT_AUGMENT_PARAM_BYTES whose colour fields are read (ignored with train == 0: no colour steps).  scale = float32(max(x1
 * - x0 + 1, y1 - y0 + 1)) * factor in float32; center = ((x0 + x1) / 2, (y0 + y1) / 2); trans = [[a, 0, iw / 2 - a cx], [0, a, ih /
 * 2 - a cy]], a = iw / scale, in binary64 on the device; d_orig [B,ih,iw,3]: the 8-bit bilinear warp inside the rectangle of
 * magnify_box (the box through trans, (p - mean) ratio + mean, rint half to even, clipped to iw - 1 / ih - 1) and zero outside;
 * d_inp [B,3,ih,iw] float32: the colour steps and the normalisation of pvv_ct_augment, the grey mean taken over d_orig;
 * d_out_mask [B,ih,iw]: the nearest warp of d_mask; d_out_kpt = trans . kpt; d_trans [B,2,3], d_center [B,2] binary64;
 * d_scale [B,2] float32; d_box [B,4] int32, the kept rectangle, inclusive.  h_mean, h_std: 3 float32 each on the host.  At most
 * four launches. */
int pvv_tless_augment(const uint8_t *d_img, const uint8_t *d_mask, const double *d_kpt, const int32_t *d_bbox, int B, int H, int W,
                      int K, int ih, int iw, int train, const float *d_factor, const double *d_box_ratio, const void *d_colour,
                      const float *h_mean, const float *h_std, void *d_workspace, size_t workspace_bytes, uint8_t *d_orig,
                      float *d_inp, uint8_t *d_out_mask, double *d_out_kpt, double *d_trans, double *d_center, float *d_scale,
                      int32_t *d_box, void *stream);

/* ------------------------------------------------------------------------
 * Colour renders: shaded colour images, instance labels and depth of a batch of scenes, several objects per image with exact
 * occlusion (ABI v8, additive; the newest section -- it stands in front of the two sections whose place at the end of this file
 * is fixed).  Citations:
 *   R = lib/utils/linemod/opengl_renderer.py:171-179 and lib/datasets/tless/opengl_renderer.py:150-156 (render(mode='rgb'), one
 *       pose at a time through an OpenGL context)
 *   S = lib/utils/linemod/opengl_backend.py:21-67 (the colour shaders), :243-247 (the read-back)
 *   A = linemod_to_coco.py:184 (fused masks under 400 pixels are dropped: d_area decides that without a read-back)
 * Device pointers, caller-owned workspace, the caller's stream last; nothing is read back, nothing synchronises, nothing is
 * allocated and nothing is kept between calls.  No fused multiply-add anywhere, no float atomics: reruns give the same bytes,
 * whatever the batch or the launch shape.  tests/render_twin.py is this contract in numpy.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= M <= 255, B*M <= 65535, sides in [1, 16384], at most 2^24 faces per object.
 *
 * The scene.  One mesh holds O objects: pts [N,3] float32, colors [N,3] uint8, faces [F,3] int32 with indices local to their
 * object, ranges [O,4] int32 on the device = (first vertex, vertex count, first face, face count).  Image b holds the M
 * instances pose[b,m] ([R | t], binary64) of the objects obj[b,m] (NULL: object 0 everywhere).  An instance with obj outside
 * [0, O), with a range row that does not lie inside the mesh or exceeds Nmax / Fmax, or with a non-finite pose entry draws
 * nothing; a face row with an index outside [0, vertex count of its object) is skipped.  All of this is tested on the device.
 *
 * Geometry: eye space, near clip, projection, snapping, coverage and the depth value are those of include/pvnet_vsd.h, word
 * for word: binary64 eye space once per (instance, vertex); 8 sub-pixel bits; 64-bit integer edge functions with the
 * owns-its-line rule; clip pieces with the new vertex computed in the p -> q direction; Z = num/den from the unclipped
 * triangle's plane, kept when den != 0 and near <= Z <= far.  With M = 1 the depth image equals pvs_render_depth_batched's as
 * bit patterns.
 *
 * Ownership: every covered, kept sample of face f of instance m offers the 64-bit key (bits of float32(Z) << 32) | (m << 24) | f
 * and the pixel keeps the unsigned minimum (one integer atomic per sample): the nearest surface wins, equal float32 depths go
 * to the lowest instance, then to the lowest face.
 *
 * Shading, per owned pixel (x, y), binary64, each line rounded once in this order:
 *   v0, v1, v2 = the owner's eye-space vertices in face-row order;  a = v1 - v0;  b = v2 - v0
 *   n = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0);  num = (n0*v00 + n1*v01) + n2*v02
 *   dy = ((y+0.5) - cy)/fy;  dx = (((x+0.5) - cx) - s*dy)/fx;  den = (n0*dx + n1*dy) + n2;  Zd = num/den
 *   P = (dx*Zd, dy*Zd, Zd);  q = P - v0;  nn = (n0*n0 + n1*n1) + n2*n2
 *   w1 = ((q x b) . n)/nn;  w2 = ((a x q) . n)/nn    (cross products in the component order of n, dots as (.0 + .1) + .2)
 *   w0 = (1.0 - w1) - w2
 *   c = (w0*C0 + w1*C1) + w2*C2 per channel, the uint8 vertex colours widened
 *   pp = (P0*P0 + P1*P1) + P2*P2;  diffuse = |num| / sqrt(nn*pp)      (the light at the camera origin; a flat normal that
 *                                                                      always faces the viewer, as dFdx x dFdy does in S)
 *   t = ambient + diffuse;  light = t > 1.0 ? 1.0 : t;  v = light*c
 *   output 0 for v < 0 or NaN, 255 for v > 255, else floor(v + 0.5)   (coverage comes from snapped coordinates: a sample may lie
 *                                                                      up to 1/256 px outside the true triangle and a weight be
 *                                                                      slightly negative; the clamp is the rule)
 *   depth = float32(Zd), equal to the key's high word;  label = m + 1;  face = f
 * A pixel nobody owns: img = bg or bg_color, label 0, depth 0, face -1.
 * Deviations from S, all stated: S interpolates the vertices' unit light vectors and renormalises, here the direction is taken
 * at the sample; parity with OpenGL's fill rule and its float32 shader is unpinned, as for the depth renderer; flat shading and
 * vertex colour only (no textures, no Phong).
 * ---------------------------------------------------------------------- */
#define PVV_RENDER_MAX_M 255
#define PVV_RENDER_MAX_FACES (1 << 24)
#define PVV_RENDER_MAX_SIDE 16384

/* Host-only.  Bytes pvv_render_color needs: 32 bytes per (instance, vertex slot) -- B*M*Nmax slots, Nmax the largest vertex count
 * of an object -- plus the 8-byte key image [B,H,W], each of the two parts rounded up to 256 bytes; 0 with pvv_last_error set
 * when a size is refused. */
size_t pvv_render_workspace_bytes(int B, int M, int Nmax, int H, int W);

/* R:171-179 with S:21-67 for a batch.  d_pts, d_colors, d_faces, d_ranges as above (N vertices, F face rows, O objects; Nmax
 * and Fmax are the largest vertex and face count of an object, computed by the host that built d_ranges); d_pose [B,M,3,4]
 * binary64; d_obj [B,M] int32 or NULL; d_K [9] row-major, shared when K_batched == 0, else [B,9]; d_bg [B,H,W,3] uint8 or NULL
 * for h_bg_color (3 bytes on the host).  d_workspace: pvv_render_workspace_bytes(B, M, Nmax, H, W) bytes, 32-byte aligned.
 * Writes d_img [B,H,W,3] uint8, d_label [B,H,W] uint8, d_depth [B,H,W] float32 (16-byte aligned), d_area [B,M] int32 (the pixels
 * each instance owns) and, unless NULL, d_face [B,H,W] int32 (16-byte aligned).  Two fills and three launches: the vertices, the
 * raster into the key image, the shading pass.  Returns 0, PVV_E_ARG / PVV_E_WORKSPACE with pvv_last_error set (checked before
 * any launch) or a hipError_t. */
int pvv_render_color(const float *d_pts, const uint8_t *d_colors, const int32_t *d_faces, int N, int F, const int32_t *d_ranges,
                     int O, int Nmax, int Fmax, const double *d_pose, const int32_t *d_obj, const double *d_K, int K_batched,
                     const uint8_t *d_bg, const uint8_t *h_bg_color, int B, int M, int H, int W, double near, double far,
                     double ambient, void *d_workspace, size_t workspace_bytes, uint8_t *d_img, uint8_t *d_label, float *d_depth,
                     int32_t *d_area, int32_t *d_face, void *stream);

/* ------------------------------------------------------------------------
 * Detector evaluation: COCO box AP (ABI v8, additive).  Citations:
 *   E = lib/evaluators/tless_test/ct.py:32-79 (Evaluator.evaluate, summarize)
 *   C = lib/evaluators/tless_test/coco_eval.py (computeIoU :164-191, evaluateImg :236-314, accumulate :316-421, Params :499-512)
 *   U = lib/utils/data_utils.py:159-162 (affine_transform)
 * Device pointers, the caller's stream last; nothing is read back, nothing synchronises, nothing is allocated.  Everything is
 * binary64 in the order written, without contraction; integers where the reference counts.  No floating-point atomics: reruns
 * and any split of the same images into calls give the same bytes.  tests/det_eval_twin.py is this contract in numpy.
 *
 * Two-decimal rounding, float('{:.2f}'.format(v)) (E:56, E:61):  p = v*100;  e = fma(v, 100, -p), the exact residual;
 *   n = rint(p);  n + 1 when p - n == 0.5 and e > 0;  n - 1 when p - n == -0.5 and e < 0;  the result is n / 100.0.
 * Box IoU (C:189-190, the rule of maskUtils.iou for xywh boxes):  ga = gw*gh;  da = dw*dh;
 *   w = min(dx+dw, gx+gw) - max(dx, gx), 0 for w <= 0;  h alike;  i = w*h;  u = crowd ? da : (da+ga) - i;  i/u.
 * The order's key, 63 bits: category index << 55 | (2^23 - 1 - n) << 31 | image rank << 7 | rank inside (image, category);
 *   a row that is not evaluated has the key 2^63 - 1.
 * The match word of a detection and an area range: bit t = matched at IoU threshold t, bit 10 + t = ignored there.
 * ---------------------------------------------------------------------- */
#define PVV_DET_T 10               /* IoU thresholds */
#define PVV_DET_R 101              /* recall thresholds */
#define PVV_DET_A 4                /* area ranges */
#define PVV_DET_M 3                /* detection caps */
#define PVV_DET_MAX_K 128          /* detection rows per image */
#define PVV_DET_MAX_D 100          /* detections of one category in one image that are kept (maxDets[-1]) */
#define PVV_DET_MAX_G 64           /* ground truths of one category in one image: a 64-bit mask per lane */
#define PVV_DET_MAX_C 255          /* categories: 8 bits of the key, one value left for the rows left out */
#define PVV_DET_MAX_IMAGES (1 << 24)

/* The IoU rule on its own: d_dt [D,4], d_gt [G,4] xywh binary64, d_iscrowd [G] int32, d_out [D,G].  One launch. */
int pvv_det_box_iou(const double *d_dt, int D, const double *d_gt, const int32_t *d_iscrowd, int G, double *d_out, void *stream);

/* E:35-37, 47, 53-61 for the B*K rows of d_detection [B,K,6] float32 (x0, y0, x1, y1, score, label), one lane per row:
 * the box times down_ratio in float32, both corners through the image's transform in binary64 (x*t00 + y*t01) + t02, xywh, the
 * two-decimal rounding of the four values and the score, area = w*h of the rounded values, the label truncated and mapped
 * through d_label_to_cat [n_labels] to the category index.  d_block [B,8] binary64 = {t00, t01, t02, t10, t11, t12, the image's
 * rank among the ground truth's images in ascending id, 0}: the host computes it, the kernels evaluate no transcendental.
 * Writes d_box [B*K,4], d_score, d_area [B*K] binary64, d_score_int (n) and d_cat [B*K] int32.  *d_err is OR-ed with 1 when a
 * value is not finite, |n| of a score reaches 2^23 or a label lies outside [0, n_labels).  One launch. */
int pvv_det_map(const float *d_detection, const double *d_block, const int32_t *d_label_to_cat, int n_labels, int B, int K,
                float down_ratio, double *d_box, double *d_score, double *d_area, int32_t *d_score_int, int32_t *d_cat,
                int32_t *d_err, void *stream);

/* C:122-159 and C:236-314 for the B images of a call, one workgroup per image, on the outputs of pvv_det_map.  d_num [B] int32
 * or int64 (num_is_i64), or NULL for K: the rows of an image that count; an image with none is left out altogether (E:43-44).
 * Ground truth, sorted by (image rank, category index) and in annotation order inside a cell: d_gt_box [N,4], d_gt_area [N]
 * binary64, d_gt_iscrowd [N] int32, d_gt_off [I*C + 1] int32 (cell = rank*C + category).  At most PVV_DET_MAX_G per cell: the
 * host checks it.  d_iou_thrs [PVV_DET_T], d_area_rng [PVV_DET_A,2] binary64, taken by the host from numpy as C:507-510 does.
 * The image's rows are ordered by (category, n descending, row) inside the workgroup, cut at PVV_DET_MAX_D per category, the
 * IoUs of a category go to LDS and the 40 (area range, threshold) pairs are lanes of one wave running C:274-297 as it stands.
 * Writes, at the ordered position of each row, d_keys [B*K] and d_words [B*K,PVV_DET_A] (all of them), and adds the count of
 * non-ignored ground truths of every evaluated (image, category) to d_npig [C,PVV_DET_A] (integer atomics).  One launch. */
int pvv_det_match(const double *d_box, const double *d_area, const int32_t *d_score_int, const int32_t *d_cat, const void *d_num,
                  int num_is_i64, const double *d_block, int B, int K, const double *d_gt_box, const double *d_gt_area,
                  const int32_t *d_gt_iscrowd, const int32_t *d_gt_off, int I, int C, const double *d_iou_thrs,
                  const double *d_area_rng, long long *d_keys, uint32_t *d_words, int32_t *d_npig, void *stream);

/* Host-only.  Bytes pvv_det_accumulate needs for N rows: 20 bytes per (area range, cap, threshold, row); 0 with pvv_last_error
 * set when N is refused. */
size_t pvv_det_accumulate_workspace_bytes(long long N);

/* C:316-421 on the keys of all calls sorted ascending (d_keys_sorted [N], d_perm [N] int64 = the position of each in d_words'
 * rows): one workgroup per (category, area range, cap), one wave per threshold.  Filter by rank < cap (h_max_dets [PVV_DET_M] on
 * the host), integer prefix counts of true and false positives, rc = tp/npig, pr = tp/((fp+tp) + 2^-52), the backward running
 * maximum as a suffix maximum, searchsorted(rc, recThrs, 'left') as PVV_DET_R binary searches (d_rec_thrs from numpy, C:508); a
 * search that ends past the last row writes 0.  d_precision, d_scores [T,R,C,A,M] and d_recall [T,C,A,M] binary64: the caller
 * fills them with -1, cells with npig == 0 are not written.  The workspace is 8-byte aligned.  One launch. */
int pvv_det_accumulate(const long long *d_keys_sorted, const long long *d_perm, const uint32_t *d_words, long long N,
                       const int32_t *d_npig, int C, const double *d_rec_thrs, const int32_t *h_max_dets, void *d_workspace,
                       size_t workspace_bytes, double *d_precision, double *d_recall, double *d_scores, void *stream);

/* ------------------------------------------------------------------------
 * Detector training: heat-map targets and the detector loss (ABI v8, additive).  Citations:
 *   P = lib/datasets/tless_train/ct.py:46-66 (prepare_detection, called per object at :86-95)
 *   G = lib/utils/data_utils.py:10-65 (gaussian_radius :10-33, gaussian2D :36-47, draw_umich_gaussian :50-65)
 *   K = lib/datasets/collate_batch.py:6-32 (ct_collator)
 *   T = lib/train/trainers/ct.py:14-31 (NetworkWrapper.forward)
 *   L = lib/utils/net_utils.py:9-49 (sigmoid, _neg_loss, FocalLoss), :195-246 (_tranpose_and_gather_feat, IndL1Loss1d)
 * Device pointers, caller-owned workspace (256-byte aligned), the caller's stream last; nothing is read back, nothing
 * synchronises, nothing is allocated and nothing is kept between calls.  No fused multiply-add anywhere;
 * tests/ct_train_twin.py is this contract in numpy.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= B <= 65535, 1 <= N <= PVV_CT_TRAIN_MAX_N, C, H, W >= 1, C*H*W and 2*H*W < 2^31.
 *
 * Targets (P, G, K), binary64, the reference's operations in its order.  boxes [B,N,4] = (x_min, y_min, x_max, y_max) on the
 * output map, PVV_BOX_F32 / PVV_BOX_I32 / PVV_BOX_I64, widened exactly; cls [B,N] and num [B] int32 or int64.  Object n of
 * image b exists when n < num[b] (num is clamped to [0, N]).  For an object:
 *   w = x_max - x_min;  h = y_max - y_min
 *   cx = rint(float32((x_min + x_max) / 2)), cy alike: half to even, as np.round of a float32                        (P:51-52)
 *   R = gaussian_radius((ceil(h), ceil(w))) (G:10-33, min_overlap = 0.7), every step as written there:
 *     s = ceil(h) + ceil(w);  a = ceil(w) * ceil(h)
 *     r1 = (s + sqrt(s*s - 4*((a * (1 - 0.7)) / (1 + 0.7)))) / 2
 *     r2 = (2*s + sqrt((2*s)*(2*s) - 16*(((1 - 0.7) * ceil(w)) * ceil(h)))) / 2
 *     b3 = (-2*0.7) * s;  d3 = b3*b3 - (4*(4*0.7)) * (((0.7 - 1) * ceil(w)) * ceil(h))
 *     r3 = d3 < 0 ? min(r1, r2) : (b3 + sqrt(d3)) / 2;   R = min(r1, r2, r3);   r = max(0, int(R))                    (P:55-56)
 *   sigma = (2r + 1) / 6;  value(dx, dy) = float32(exp(-((dx*dx) / (sigma*sigma) + (dy*dy) / (sigma*sigma)) / 2))     (G:41-45, 52)
 *   for |dx| <= r, |dy| <= r inside the map (G:58-62); the class plane takes the maximum over its objects (G:64), +0 elsewhere.
 *   The centre is exp(-0) = 1 exactly.  The rule of G:46 (values below eps * max become 0) is not applied: it never fires.
 *   wh = (float32(w), float32(h));  ct_ind = cy*W + cx;  ct_cls = cls;  ct_01 = 1                                    (P:59-60, K:18-29)
 * An object is dropped -- it draws nothing and takes no row -- when w <= 0 or h <= 0 (ct.py:91-92 drops the equalities; a
 * negative size makes the reference raise), when a coordinate is not finite or not below 2^24 in magnitude, when cls lies
 * outside [0, C) or (cx, cy) outside the map (the reference's behaviour there is an indexing accident).  The survivors are
 * packed to the front in their order; rows from ct_num[b] on are zeros.  K pads to the batch's largest ct_num; here the
 * width is N (zero-weight rows change neither loss).
 *
 * Loss (T, L).  hm_pred [B,C,H,W] logits, wh_pred [B,2,H,W], ct_hm [B,C,H,W]: float32, each image contiguous, images
 * `*_image_stride` elements apart (channel slices of one network output are read in place).  wh [B,N,2] float32, ct_ind [B,N]
 * int32 or int64, ct_01 [B,N] float32, contiguous.
 * Focal loss (L:9-11, 21-38), per element in binary64 from the float32 logit z and target g:
 *   s = 1 / (1 + exp(-z));   p = min(max(s, lo), hi),  lo = float32(1e-4), hi = float32(1 - 1e-4) = 0.99989998...
 *   g == 1:  pos = log(p) * ((1-p)*(1-p))            g < 1:  neg = (log(1-p) * (p*p)) * (((1-g)*(1-g)) * ((1-g)*(1-g)))
 *   num_pos = the count of g == 1, an integer;  P, Q = the sums of pos, neg
 *   ct_loss = float32(num_pos == 0 ? -Q : -(P + Q) / num_pos)
 * Sums: binary64, in the order of the Training section below over the flattened [C*H*W] image: a lane owns
 * PVV_TRAIN_LANE_PIXELS consecutive elements, a tile is PVV_TRAIN_TILE elements, PVV_TRAIN_IMAGE_SLOTS slots per image,
 * then ascending b.  Reruns give the same bits.
 * Focal gradient, k = num_pos == 0 ? -go_ct : -go_ct / num_pos (go_ct widened):
 *   g == 1:  dp = ((1-p)*(1-p)) / p - (2*(1-p)) * log(p)
 *   g < 1:   dp = ((2*p) * log(1-p) - (p*p) / (1-p)) * (((1-g)*(1-g)) * ((1-g)*(1-g)))
 *   grad = lo <= s <= hi ? float32((k * dp) * ((1-s) * s)) : +0        (the derivative of the sigmoid from the unclamped s)
 * wh loss (L:240-246), per object n and channel c with i = ct_ind[b,n], m = ct_01[b,n], binary64 from the float32 values:
 *   d = wh_pred[b,c,i]*m - wh[b,n,c]*m;  z = |d|;  element = z < 1 ? (0.5*z)*z : z - 0.5
 *   object = element(c = 0) + element(c = 1); image = slot j sums its objects j, j+256, ... ascending, then the slot order
 *   M = the sum of ct_01 in the same order;   wh_loss = float32(S / (M*2 + 1e-4))
 * wh gradient, float32 (what torch's CPU autograd computes): den = float32(M)*2 + 1e-4f;  v = go_wh / den;
 *   d = wh_pred*m - wh*m in float32;  t = (d < -1 ? -v : d > 1 ? v : v*d) * m;  grad[b,c,i] = +0 + the t of the objects with
 *   ct_ind == i in ascending n, +0 everywhere else.  One thread owns an (image, index): no atomics.
 * An index outside [0, H*W) is never used as an address.  At a position with ct_01 != 0 it is counted in out_state, and if
 * the count is not zero wh_loss and every element of the wh gradient are NaN; at a position with ct_01 == 0 it adds nothing.
 * ct_loss and its gradient are not affected.
 *
 * out_state: 32 bytes on the device, 8-byte aligned: int64 num_pos, int64 the count of bad indices, binary64 M, int64 0.
 * ---------------------------------------------------------------------- */
#define PVV_BOX_F32 0
#define PVV_BOX_I32 1
#define PVV_BOX_I64 2
#define PVV_CT_TRAIN_MAX_N 512 /* objects per image: the list of an image is staged in LDS */

/* P:46-66 per object with K:6-32 for a batch: d_ct_hm [B,C,H,W] f32, d_wh [B,N,2] f32, d_ct_cls [B,N] i64, d_ct_ind [B,N] i64,
 * d_ct_01 [B,N] f32, d_ct_num [B] i64, all contiguous and all written completely.  Two launches. */
int pvv_ct_targets(const void *d_boxes, int box_kind, const void *d_cls, int cls_is_i64, const void *d_num, int num_is_i64, int B,
                   int N, int C, int H, int W, float *d_ct_hm, float *d_wh, long long *d_ct_cls, long long *d_ct_ind,
                   float *d_ct_01, long long *d_ct_num, void *stream);

/* Host-only.  Bytes pvv_ct_loss_forward needs: per (image, tile) two binary64 and one int64, per image four binary64 and two
 * int64, each of the four parts rounded up to 256 bytes; 0 with pvv_last_error set when the sizes are refused. */
size_t pvv_ct_loss_workspace_bytes(int B, int C, int H, int W);

/* T:20-26 (L:9-49, L:240-246).  d_out_losses [2] float32 = {ct_loss, wh_loss}; d_out_state as above.  Three launches: the
 * tiles, the images (with the objects), the batch. */
int pvv_ct_loss_forward(const float *d_hm_pred, long long hp_image_stride, const float *d_wh_pred, long long wp_image_stride,
                        const float *d_ct_hm, long long hm_image_stride, const float *d_wh, const void *d_ct_ind, int ind_is_i64,
                        const float *d_ct_01, int B, int N, int C, int H, int W, void *workspace, size_t workspace_bytes,
                        float *d_out_losses, void *d_out_state, void *stream);

/* What autograd derives from T:20-26: d_grad_hm [B,C,H,W] and d_grad_wh [B,2,H,W], contiguous float32, from the inputs of the
 * forward call, its d_out_state and d_grad_losses [2] float32 on the device = {go_ct, go_wh}.  One streaming launch over the
 * heat map; a fill and one launch of a workgroup per image for the wh gradient. */
int pvv_ct_loss_backward(const float *d_hm_pred, long long hp_image_stride, const float *d_wh_pred, long long wp_image_stride,
                         const float *d_ct_hm, long long hm_image_stride, const float *d_wh, const void *d_ct_ind, int ind_is_i64,
                         const float *d_ct_01, int B, int N, int C, int H, int W, const void *d_out_state,
                         const float *d_grad_losses, float *d_grad_hm, float *d_grad_wh, void *stream);

/* ------------------------------------------------------------------------
 * Training: vote targets and the PVNet loss (ABI v8, additive).  Citations:
 *   D = lib/utils/pvnet/pvnet_data_utils.py:30-44 (compute_vertex, called per sample at lib/datasets/<dataset>/pvnet.py:53)
 *   T = lib/train/trainers/pvnet.py:25-34 (NetworkWrapper.forward: the vote loss and the cross entropy)
 *   N = lib/networks/pvnet/resnet18.py:93-94 (seg and vertex are channel slices of one [B, C+2K, H, W] tensor)
 * Device pointers, caller-owned workspace (256-byte aligned), the caller's stream last; nothing is read back, nothing
 * synchronises, nothing is allocated and nothing is kept between calls.
 *   mask        [B,H,W] of PVV_MASK_U8 (uint8, or bool: one byte, 0 or 1), PVV_MASK_I32 or PVV_MASK_I64
 *   kpt_2d      [B,K,2] (x, y), float32 or binary64 (kpt_is_f64); float32 is widened exactly
 *   vertex_pred [B,2K,H,W] and seg_pred [B,C,H,W] float32, each image contiguous, images `*_image_stride` elements apart
 *               (N: channel slices are passed as they lie, without a copy); target likewise, channel 2k = x, 2k+1 = y
 *   Exactly one of kpt_2d and target is given (the other NULL): with kpt_2d the target is recomputed per pixel, the field
 *   never exists.  Both forms are the same kernels.
 * Limits, refused with PVV_E_ARG beyond them: 1 <= B <= 65535, 1 <= K <= PVV_TRAIN_MAX_K, 1 <= C <= PVV_TRAIN_MAX_C,
 * H*W, 2K*H*W and C*H*W < 2^31, B*H*W < 2^53.
 *
 * The arithmetic contract (no fused multiply-add anywhere; tests/train_twin.py is this contract in numpy):
 *
 * Target (D:33-41), binary64, for a pixel (x, y) with mask == 1 and keypoint (kx, ky):
 *   dx = kx - x;  dy = ky - y;  n = sqrt(dx*dx + dy*dy);  if n < 1e-3: n += 1e-3;  target = float32(dx/n), float32(dy/n)
 * every other pixel: +0.
 *
 * Vote loss (T:25-27), per element in float32:  w = float(mask);  d = pred*w - target*w;  z = |d|;
 *   element = z < 1 ? (0.5f*z)*z : z - 0.5f          (torch's smooth_l1_loss, beta = 1; a non-finite pred gives a non-finite
 *   loss as in the reference: no pixel is skipped).
 *
 * Sums: binary64, in one order that no launch parameter changes.
 *   pixel  = its elements (vote) in ascending channel, each widened; its one term (seg)
 *   lane   = PVV_TRAIN_LANE_PIXELS consecutive pixels of the flattened plane, ascending
 *   tile   = PVV_TRAIN_TILE pixels = 256 lanes: slot j += slot j+s for s = 128, 64, ..., 1; pixels past H*W count as +0
 *   image  = slot j (of PVV_TRAIN_IMAGE_SLOTS) = the tiles t = j, j+256, ... ascending, then the same slot order
 *   batch  = ascending b
 * The mask sum M is an integer (the sum of the mask values), converted once: wsum = float32(M).
 *   vote_loss = float32(float32(float32(S) / wsum) / float32(2K));  M = 0 gives 0/0 = NaN as in the reference.
 *
 * Vote gradient, float32, go_vote the upstream gradient:  s = (go_vote / float32(2K)) / wsum;
 *   g = (d < -1 ? -s : d > 1 ? s : s*d) * w
 *
 * Seg loss (T:31-32, CrossEntropyLoss with mean reduction), binary64 from the float32 logits z_c of a pixel:
 *   m = max_c z_c (z > m ? z : m from z_0 on);  e_c = exp(z_c - m);  s = sum_c e_c ascending;
 *   term = (m - z_label) + log(s)                     (both parts >= 0: nothing cancels)
 *   seg_loss = float32(sum / (B*H*W)), the sum in the order above.
 * Seg gradient, N = B*H*W, go_seg widened:
 *   c != label: float32(((go_seg * e_c) / s) / N);   c == label: float32(((-go_seg * r) / s) / N),
 *   r = the sum of e_c over c != label, ascending -- never p - 1.
 *
 * Labels: label = mask value.  A label outside [0, C) is counted in out_state and selects no logit; if the count is not
 * zero both losses and every gradient element are NaN (the reference asserts on the device here): no fault, no
 * synchronisation, no silently wrong value.
 *
 * out_state: two int64 on the device, {M, the count of labels outside [0, C)}; the backward pass reads it.
 * ---------------------------------------------------------------------- */
#define PVV_MASK_U8 0
#define PVV_MASK_I32 1
#define PVV_MASK_I64 2
#define PVV_TRAIN_MAX_K 64
#define PVV_TRAIN_MAX_C 16
#define PVV_TRAIN_LANE_PIXELS 4
#define PVV_TRAIN_TILE 1024
#define PVV_TRAIN_IMAGE_SLOTS 256

/* D:30-44 for a batch: d_out [B,2K,H,W] float32, what batch['vertex'] holds after the loader's transpose(2, 0, 1)
 * (lib/datasets/<dataset>/pvnet.py:53).  One launch. */
int pvv_vertex_target(const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64, int B, int K, int H, int W,
                      float *d_out, void *stream);

/* Host-only.  Bytes pvv_pvnet_loss_forward needs; 0 with pvv_last_error set when the sizes are refused. */
size_t pvv_pvnet_loss_workspace_bytes(int B, int H, int W);

/* T:25-34.  d_out_losses [2] float32 = {vote_loss, seg_loss}; d_out_state as above (8-byte aligned).  Three launches: the
 * tiles, the images, the batch. */
int pvv_pvnet_loss_forward(const float *d_vertex_pred, long long vp_image_stride, const float *d_seg_pred,
                           long long sp_image_stride, const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64,
                           const float *d_target, long long tg_image_stride, int B, int K, int C, int H, int W, void *workspace,
                           size_t workspace_bytes, float *d_out_losses, void *d_out_state, void *stream);

/* What autograd derives from T:25-34, in one launch: d_grad_vertex [B,2K,H,W] and d_grad_seg [B,C,H,W], contiguous float32,
 * from the inputs of the forward call, its d_out_state and d_grad_losses [2] float32 on the device = {go_vote, go_seg}.
 * d and the softmax are recomputed, not saved. */
int pvv_pvnet_loss_backward(const float *d_vertex_pred, long long vp_image_stride, const float *d_seg_pred,
                            long long sp_image_stride, const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64,
                            const float *d_target, long long tg_image_stride, int B, int K, int C, int H, int W,
                            const void *d_out_state, const float *d_grad_losses, float *d_grad_vertex, float *d_grad_seg,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PVNET_VOTE_H_ */
