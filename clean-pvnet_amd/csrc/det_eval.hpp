// det_eval.hpp -- the detector's score on the device: COCO box AP (include/pvnet_vote.h, "Detector evaluation").  Included at the
// end of pvnet_vote.hip: built with -ffp-contract=off, every binary64 operation below rounds once, in the order written, so that
// the numpy twin (tests/det_eval_twin.py) gives the same bits.  The one fused multiply-add is the explicit intrinsic in
// det_round2: it computes the exact residual of a product.
//
// Reference behaviour restated (paths relative to /root/reference):
//   E = lib/evaluators/tless_test/ct.py          C = lib/evaluators/tless_test/coco_eval.py        U = lib/utils/data_utils.py
#pragma once

namespace {

constexpr int kDetT = PVV_DET_T, kDetR = PVV_DET_R, kDetA = PVV_DET_A, kDetM = PVV_DET_M;
constexpr int kDetMaxK = PVV_DET_MAX_K, kDetMaxG = PVV_DET_MAX_G, kDetMaxD = PVV_DET_MAX_D;
constexpr int kDetAccBlock = 64 * kDetT;                 // one wave per IoU threshold
constexpr long long kDetSentinel = 0x7fffffffffffffffll;  // the key of a row that is not evaluated: sorts behind every category

static_assert(kDetA * kDetT <= 64, "the (area range, threshold) pairs are lanes of one wave");
static_assert(kDetMaxK <= kBlock && kDetMaxG <= 64 && kDetMaxD < 128, "one thread per row, a 64-bit mask of ground truths, 7 bits of rank");

// float('{:.2f}'.format(v)) (E:56, E:61): the decimal with two places nearest to the exact binary value, ties to even, read back.
// p + e == v * 100 exactly; n = rint(p) is wrong only when p sits on a half and e decides.  *n_out is the integer n.
__device__ __forceinline__ double det_round2(double v, double *n_out, bool *bad)
{
    const double p = v * 100.0;
    const double e = __builtin_fma(v, 100.0, -p);
    double n = rint(p);
    const double d = p - n;                          // exact, |d| <= 0.5
    if (d == 0.5 && e > 0.0) n = n + 1.0;
    else if (d == -0.5 && e < 0.0) n = n - 1.0;
    if (!(fabs(p) < 4503599627370496.0)) *bad = true;   // not finite, or no room for a half
    *n_out = n;
    return n / 100.0;
}

// C:189-190 for boxes, the rule of maskUtils.iou (bbIou).
__device__ __forceinline__ double det_box_iou(const double *dt, const double *gt, int crowd)
{
    const double ga = gt[2] * gt[3], da = dt[2] * dt[3];
    const double dxe = dt[0] + dt[2], gxe = gt[0] + gt[2];
    const double w = (dxe < gxe ? dxe : gxe) - (dt[0] > gt[0] ? dt[0] : gt[0]);
    if (w <= 0.0) return 0.0;
    const double dye = dt[1] + dt[3], gye = gt[1] + gt[3];
    const double h = (dye < gye ? dye : gye) - (dt[1] > gt[1] ? dt[1] : gt[1]);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : (da + ga) - i;
    return i / u;
}

__global__ __launch_bounds__(kBlock) void k_det_box_iou(const double *__restrict__ dt, int D, const double *__restrict__ gt,
                                                        const int32_t *__restrict__ crowd, int G, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)D * G) return;
    const int d = (int)(i / G), g = (int)(i - (long long)d * G);
    out[i] = det_box_iou(dt + 4 * (size_t)d, gt + 4 * (size_t)g, crowd[g]);
}

// E:35-37, 47, 53-61: one lane per detection row.  block[b] = {t00, t01, t02, t10, t11, t12, image rank, 0}.
__global__ __launch_bounds__(kBlock) void k_det_map(const float *__restrict__ det, const double *__restrict__ block,
                                                    const int32_t *__restrict__ label_to_cat, int n_labels, int rows, int K,
                                                    float down_ratio, double *__restrict__ box, double *__restrict__ score,
                                                    double *__restrict__ area, int32_t *__restrict__ sn, int32_t *__restrict__ cat,
                                                    int32_t *__restrict__ err)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const float *row = det + (size_t)r * 6;
    const double *t = block + (size_t)(r / K) * 8;
    bool bad = false;
    double c[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double x = (double)(row[2 * j] * down_ratio), y = (double)(row[2 * j + 1] * down_ratio);   // E:35, float32
        c[2 * j] = (x * t[0] + y * t[1]) + t[2];                                                           // U:161
        c[2 * j + 1] = (x * t[3] + y * t[4]) + t[5];
    }
    c[2] = c[2] - c[0];                                                                                    // E:54-55
    c[3] = c[3] - c[1];
    double n;
#pragma unroll
    for (int j = 0; j < 4; ++j) box[(size_t)r * 4 + j] = c[j] = det_round2(c[j], &n, &bad);
    score[r] = det_round2((double)row[4], &n, &bad);
    if (!(fabs(n) < 8388608.0)) { bad = true; n = 0.0; }                    // the score integer is 24 bits of the order's key
    sn[r] = (int32_t)n;
    area[r] = c[2] * c[3];                                                  // loadRes: area = w * h
    const float lf = row[5];
    int32_t ci = -1;
    if (lf > -1.f && lf < (float)n_labels) ci = label_to_cat[(int)lf];      // E:37 astype(int) truncates; E:59
    else bad = true;
    cat[r] = ci;
    if (bad) atomicOr(err, 1);
}

// C:122-159, 236-314 for the images of one call: one workgroup per image.
__global__ __launch_bounds__(kBlock) void k_det_match(const double *__restrict__ box, const double *__restrict__ area,
                                                      const int32_t *__restrict__ sn, const int32_t *__restrict__ cat,
                                                      const void *__restrict__ num, int num_is_i64, const double *__restrict__ block,
                                                      int K, const double *__restrict__ gt_box, const double *__restrict__ gt_area,
                                                      const int32_t *__restrict__ gt_crowd, const int32_t *__restrict__ gt_off, int I,
                                                      int C, const double *__restrict__ iou_thrs, const double *__restrict__ area_rng,
                                                      long long *__restrict__ keys, uint32_t *__restrict__ words,
                                                      int32_t *__restrict__ npig)
{
    __shared__ double s_iou[kDetMaxD * kDetMaxG];
    __shared__ unsigned long long s_key[kDetMaxK], s_sorted[kDetMaxK];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long rows = K;
    if (num) rows = num_is_i64 ? ((const long long *)num)[b] : (long long)((const int32_t *)num)[b];
    rows = rows < 0 ? 0 : rows > K ? K : rows;
    const long long rank_ll = (long long)block[(size_t)b * 8 + 6];
    const bool image_ok = rank_ll >= 0 && rank_ll < I;                     // (the host has checked it: never an address otherwise)
    if (rows == 0 || !image_ok) {                                          // E:43-44: the image is not evaluated at all
        if (tid < K) {
            keys[(size_t)b * K + tid] = kDetSentinel;
            for (int a = 0; a < kDetA; ++a) words[((size_t)b * K + tid) * kDetA + a] = 0u;
        }
        return;
    }
    const int rank = (int)rank_ll;
    // the order inside the image: (category, score descending, row ascending), C:174 / C:260 on each category's list
    if (tid < K) {
        const int r = b * K + tid;
        const int ci = tid < rows ? cat[r] : -1;
        const unsigned long long cf = ci >= 0 ? (unsigned long long)ci : 0xffffffull;
        s_key[tid] = (cf << 40) | ((unsigned long long)(8388607 - sn[r]) << 8) | (unsigned long long)tid;
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long mine = s_key[tid];
        int pos = 0;
        for (int j = 0; j < K; ++j) pos += s_key[j] < mine;
        s_sorted[pos] = mine;
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long mine = s_sorted[tid];
        const unsigned long long cf = mine >> 40;
        int first = 0;
        for (int j = 0; j < K; ++j) first += (s_sorted[j] >> 40) < cf;
        const int within = tid - first;
        long long key = kDetSentinel;
        if (cf != 0xffffffull && within < kDetMaxD)                         // C:176-177: the cut at maxDets[-1]
            key = ((long long)cf << 55) | ((long long)((mine >> 8) & 0xffffffull) << 31) | ((long long)rank << 7) | within;
        else
            for (int a = 0; a < kDetA; ++a) words[((size_t)b * K + tid) * kDetA + a] = 0u;
        keys[(size_t)b * K + tid] = key;
    }
    const int lane = tid & 63, wave = tid >> 6;
    int ds = 0;
    for (int c = 0; c < C; ++c) {
        // (uniform: every thread takes the same path through the barriers)
        const int de = __syncthreads_count(tid < K && (s_sorted[tid] >> 40) <= (unsigned long long)c);
        const int g0 = gt_off[(size_t)rank * C + c];
        int G = gt_off[(size_t)rank * C + c + 1] - g0;
        G = G < 0 ? 0 : G > kDetMaxG ? kDetMaxG : G;                        // (the host refuses more than kDetMaxG)
        const int D = de - ds < kDetMaxD ? de - ds : kDetMaxD;
        if (D > 0 || G > 0) {                                               // C:248-249
            for (int i = tid; i < D * G; i += kBlock) {
                const int d = i / G, g = i - d * G;
                const int r = b * K + (int)(s_sorted[ds + d] & 0xff);
                s_iou[i] = det_box_iou(box + (size_t)r * 4, gt_box + (size_t)(g0 + g) * 4, gt_crowd[g0 + g]);
            }
            __syncthreads();
            if (wave == 0) {
                const bool active = lane < kDetA * kDetT;
                const int a = active ? lane / kDetT : 0, t = lane % kDetT;
                const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1], thr = iou_thrs[t];
                const unsigned long long gmask = G == 64 ? ~0ull : (1ull << G) - 1ull;
                unsigned long long ig = 0, crowd = 0, gtm = 0;
                for (int g = 0; g < G; ++g) {                               // C:251-255
                    const double ga = gt_area[g0 + g];
                    const bool cr = gt_crowd[g0 + g] != 0;
                    if (cr) crowd |= 1ull << g;
                    if (cr || ga < lo || ga > hi) ig |= 1ull << g;
                }
                if (active && t == 0) atomicAdd(&npig[c * kDetA + a], __popcll(~ig & gmask));   // C:372-373, an integer
                for (int d = 0; d < D; ++d) {                               // C:274-297
                    const int r = b * K + (int)(s_sorted[ds + d] & 0xff);
                    double iou = thr < 1 - 1e-10 ? thr : 1 - 1e-10;
                    int m = -1;
                    if (active) {
                        // C:258: the ground truths inside the range first, then the ignored ones, each in annotation order
                        for (unsigned long long rest = ~ig & gmask; rest; rest &= rest - 1) {
                            const int g = __builtin_ctzll(rest);
                            if (((gtm >> g) & 1) && !((crowd >> g) & 1)) continue;
                            const double v = s_iou[d * G + g];
                            if (v < iou) continue;
                            iou = v;
                            m = g;
                        }
                        if (m < 0)                                          // C:284-285: a held match stops at the first ignored one
                            for (unsigned long long rest = ig & gmask; rest; rest &= rest - 1) {
                                const int g = __builtin_ctzll(rest);
                                if (((gtm >> g) & 1) && !((crowd >> g) & 1)) continue;
                                const double v = s_iou[d * G + g];
                                if (v < iou) continue;
                                iou = v;
                                m = g;
                            }
                    }
                    const bool matched = m >= 0;
                    bool dig = false;
                    if (matched) { gtm |= 1ull << m; dig = (ig >> m) & 1; }
                    else if (active) { const double da = area[r]; dig = da < lo || da > hi; }   // C:299-300
                    const unsigned long long bm = __ballot(matched), bi = __ballot(dig);
                    if (lane < kDetA) {
                        const uint32_t mb = (uint32_t)(bm >> (lane * kDetT)) & 0x3ffu, ib = (uint32_t)(bi >> (lane * kDetT)) & 0x3ffu;
                        words[((size_t)b * K + ds + d) * kDetA + lane] = mb | (ib << 10);
                    }
                }
            }
            __syncthreads();
        }
        ds = de;
    }
}

__device__ __forceinline__ long long det_lower_bound(const long long *__restrict__ keys, long long n, long long v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// C:354-411: one workgroup per (category, area range, detection cap), one wave per IoU threshold.  ws: per (a, m, t) N slots of
// int32 tp, int32 fp, int32 score integer and binary64 running maximum; a category uses the slots of its own key range.
__global__ __launch_bounds__(kDetAccBlock) void k_det_accumulate(const long long *__restrict__ keys, const long long *__restrict__ perm,
                                                                 const uint32_t *__restrict__ words, long long N,
                                                                 const int32_t *__restrict__ npig_all, int C,
                                                                 const double *__restrict__ rec_thrs, int md0, int md1, int md2,
                                                                 int32_t *__restrict__ ws_tp, int32_t *__restrict__ ws_fp,
                                                                 int32_t *__restrict__ ws_n, double *__restrict__ ws_pm,
                                                                 double *__restrict__ precision, double *__restrict__ recall,
                                                                 double *__restrict__ scores)
{
    const int c = blockIdx.x, a = blockIdx.y, m = blockIdx.z;
    const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
    const int npig = npig_all[c * kDetA + a];
    if (npig == 0) return;                                                   // C:361-362, 374-375: the cells stay -1
    const int max_det = m == 0 ? md0 : m == 1 ? md1 : md2;
    const long long lo = det_lower_bound(keys, N, (long long)c << 55), hi = det_lower_bound(keys, N, (long long)(c + 1) << 55);
    const size_t base = ((size_t)(a * kDetM + m) * kDetT + t) * (size_t)N + (size_t)lo;
    int32_t *tp_arr = ws_tp + base, *fp_arr = ws_fp + base, *n_arr = ws_n + base;
    double *pm_arr = ws_pm + base;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long nd = 0;
    int tp_run = 0, fp_run = 0;
    for (long long i0 = lo; i0 < hi; i0 += 64) {                             // C:363-380: filter, prefix counts
        const long long i = i0 + lane;
        bool valid = false, tpf = false, fpf = false;
        int sn = 0;
        if (i < hi) {
            const long long key = keys[i];
            valid = (int)(key & 127) < max_det;
            if (valid) {
                const uint32_t w = words[(size_t)perm[i] * kDetA + a];
                const bool mt = (w >> t) & 1u, ig = (w >> (kDetT + t)) & 1u;
                tpf = mt && !ig;
                fpf = !mt && !ig;
                sn = 8388607 - (int)((key >> 31) & 0xffffff);
            }
        }
        const unsigned long long bv = __ballot(valid), bt = __ballot(tpf), bf = __ballot(fpf);
        if (valid) {
            const long long pos = nd + __popcll(bv & below);
            tp_arr[pos] = tp_run + __popcll(bt & below) + (tpf ? 1 : 0);
            fp_arr[pos] = fp_run + __popcll(bf & below) + (fpf ? 1 : 0);
            n_arr[pos] = sn;
        }
        nd += __popcll(bv);
        tp_run += __popcll(bt);
        fp_run += __popcll(bf);
    }
    __syncthreads();                                                         // (nd is the same in every wave: the barriers are uniform)
    double carry = -1.0;
    for (long long i0 = nd > 0 ? ((nd - 1) / 64) * 64 : -1; i0 >= 0; i0 -= 64) {   // C:386, 399-401: a suffix maximum
        const long long i = i0 + lane;
        double pr = -1.0;
        if (i < nd) {
            const double tp = (double)tp_arr[i], fp = (double)fp_arr[i];
            pr = tp / ((fp + tp) + 2.220446049250313e-16);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_down(pr, off, 64);
            if (lane + off < 64 && o > pr) pr = o;
        }
        if (carry > pr) pr = carry;
        if (i < nd) pm_arr[i] = pr;
        carry = __shfl(pr, 0, 64);
    }
    __syncthreads();
    const size_t cell = ((size_t)c * kDetA + a) * kDetM + m;
    if (lane == 0) recall[(size_t)t * C * kDetA * kDetM + cell] = nd ? (double)tp_arr[nd - 1] / (double)npig : 0.0;   // C:390-393
    for (int ri = lane; ri < kDetR; ri += 64) {                              // C:403-409
        const double thr = rec_thrs[ri];
        long long l = 0, h = nd;
        while (l < h) {
            const long long mid = l + ((h - l) >> 1);
            if ((double)tp_arr[mid] / (double)npig < thr) l = mid + 1; else h = mid;
        }
        const size_t o = ((size_t)t * kDetR + ri) * C * kDetA * kDetM + cell;
        precision[o] = l < nd ? pm_arr[l] : 0.0;
        scores[o] = l < nd ? (double)n_arr[l] / 100.0 : 0.0;
    }
}

int det_ws_parts(long long N, size_t *ints, size_t *total)
{
    if (N < 0 || N >= (1ll << 31)) return fail(PVV_E_ARG, "det: the detection rows must number less than 2^31");
    const size_t slots = (size_t)kDetA * kDetM * kDetT * (size_t)N;
    *ints = (slots * 4 + 255) / 256 * 256;
    *total = 3 * *ints + slots * 8;
    return PVV_OK;
}

}  // namespace

PVV_EXPORT int pvv_det_box_iou(const double *d_dt, int D, const double *d_gt, const int32_t *d_iscrowd, int G, double *d_out, void *stream)
{
    if (D < 0 || G < 0 || (long long)D * G >= (1ll << 31)) return fail(PVV_E_ARG, "det: D, G >= 0 and D*G < 2^31");
    if (D == 0 || G == 0) return PVV_OK;
    if (!d_dt || !d_gt || !d_iscrowd || !d_out) return fail(PVV_E_ARG, "det: NULL device pointer");
    hipLaunchKernelGGL(k_det_box_iou, dim3((unsigned)(((long long)D * G + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       d_dt, D, d_gt, d_iscrowd, G, d_out);
    return check_launch("k_det_box_iou");
}

PVV_EXPORT int pvv_det_map(const float *d_detection, const double *d_block, const int32_t *d_label_to_cat, int n_labels, int B, int K,
                           float down_ratio, double *d_box, double *d_score, double *d_area, int32_t *d_score_int, int32_t *d_cat,
                           int32_t *d_err, void *stream)
{
    if (B < 1 || B > 65535 || K < 1 || K > PVV_DET_MAX_K) return fail(PVV_E_ARG, "det: 1 <= B <= 65535 and 1 <= K <= PVV_DET_MAX_K");
    if (n_labels < 1 || n_labels > PVV_DET_MAX_C) return fail(PVV_E_ARG, "det: 1 <= categories <= PVV_DET_MAX_C");
    if (!d_detection || !d_block || !d_label_to_cat || !d_box || !d_score || !d_area || !d_score_int || !d_cat || !d_err)
        return fail(PVV_E_ARG, "det: NULL device pointer");
    const int rows = B * K;
    hipLaunchKernelGGL(k_det_map, dim3((rows + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, d_detection, d_block,
                       d_label_to_cat, n_labels, rows, K, down_ratio, d_box, d_score, d_area, d_score_int, d_cat, d_err);
    return check_launch("k_det_map");
}

PVV_EXPORT int pvv_det_match(const double *d_box, const double *d_area, const int32_t *d_score_int, const int32_t *d_cat,
                             const void *d_num, int num_is_i64, const double *d_block, int B, int K, const double *d_gt_box,
                             const double *d_gt_area, const int32_t *d_gt_iscrowd, const int32_t *d_gt_off, int I, int C,
                             const double *d_iou_thrs, const double *d_area_rng, long long *d_keys, uint32_t *d_words,
                             int32_t *d_npig, void *stream)
{
    if (B < 1 || B > 65535 || K < 1 || K > PVV_DET_MAX_K) return fail(PVV_E_ARG, "det: 1 <= B <= 65535 and 1 <= K <= PVV_DET_MAX_K");
    if (C < 1 || C > PVV_DET_MAX_C || I < 1 || I > PVV_DET_MAX_IMAGES) return fail(PVV_E_ARG, "det: categories or images out of range");
    if (!d_box || !d_area || !d_score_int || !d_cat || !d_block || !d_gt_box || !d_gt_area || !d_gt_iscrowd || !d_gt_off ||
        !d_iou_thrs || !d_area_rng || !d_keys || !d_words || !d_npig)
        return fail(PVV_E_ARG, "det: NULL device pointer");
    hipLaunchKernelGGL(k_det_match, dim3(B), dim3(kBlock), 0, (hipStream_t)stream, d_box, d_area, d_score_int, d_cat, d_num, num_is_i64,
                       d_block, K, d_gt_box, d_gt_area, d_gt_iscrowd, d_gt_off, I, C, d_iou_thrs, d_area_rng, d_keys, d_words, d_npig);
    return check_launch("k_det_match");
}

PVV_EXPORT size_t pvv_det_accumulate_workspace_bytes(long long N)
{
    size_t ints, total;
    if (det_ws_parts(N, &ints, &total)) return 0;
    return total;
}

PVV_EXPORT int pvv_det_accumulate(const long long *d_keys_sorted, const long long *d_perm, const uint32_t *d_words, long long N,
                                  const int32_t *d_npig, int C, const double *d_rec_thrs, const int32_t *h_max_dets,
                                  void *d_workspace, size_t workspace_bytes, double *d_precision, double *d_recall, double *d_scores,
                                  void *stream)
{
    size_t ints, total;
    if (int e = det_ws_parts(N, &ints, &total)) return e;
    if (C < 1 || C > PVV_DET_MAX_C) return fail(PVV_E_ARG, "det: 1 <= categories <= PVV_DET_MAX_C");
    if (!h_max_dets || !d_npig || !d_rec_thrs || !d_precision || !d_recall || !d_scores) return fail(PVV_E_ARG, "det: NULL pointer");
    if (N > 0 && (!d_keys_sorted || !d_perm || !d_words || !d_workspace)) return fail(PVV_E_ARG, "det: NULL device pointer");
    if (workspace_bytes < total) return fail(PVV_E_WORKSPACE, "det: workspace too small");
    if (((uintptr_t)d_workspace & 7) != 0) return fail(PVV_E_ARG, "det: the workspace must be 8-byte aligned");
    for (int m = 0; m < kDetM; ++m)
        if (h_max_dets[m] < 1 || h_max_dets[m] > kDetMaxD) return fail(PVV_E_ARG, "det: a detection cap outside [1, PVV_DET_MAX_D]");
    char *ws = (char *)d_workspace;
    hipLaunchKernelGGL(k_det_accumulate, dim3(C, kDetA, kDetM), dim3(kDetAccBlock), 0, (hipStream_t)stream, d_keys_sorted, d_perm,
                       d_words, N, d_npig, C, d_rec_thrs, (int)h_max_dets[0], (int)h_max_dets[1], (int)h_max_dets[2], (int32_t *)ws,
                       (int32_t *)(ws + ints), (int32_t *)(ws + 2 * ints), (double *)(ws + 3 * ints), d_precision, d_recall, d_scores);
    return check_launch("k_det_accumulate");
}
