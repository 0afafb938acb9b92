// crop.hpp -- detector heat maps -> boxes, boxes -> PVNet crops, and crop results -> canvas (include/pvnet_vote.h, "Detector
// decode, crops and the way back").  Part of pvnet_vote.hip: built with -ffp-contract=off, every float and double operation
// below rounds once, in the order written, so that the numpy twin (tests/crop_twin.py) gives the same bits.  sat_rint,
// invert_affine, the two fixed-point warp rules, the crop's map and the rectangle of magnify_box are those of warp.hpp.
//
// Reference behaviour restated (paths relative to /root/reference):
//   D = lib/utils/ct/ct_decode.py        U = lib/utils/data_utils.py       R = lib/networks/ct_pvnet/res.py
//   T = lib/utils/tless/tless_test_utils.py                                E = lib/evaluators/tless_test/pvnet.py
#pragma once

#include "warp.hpp"

namespace {

using ct_key = unsigned long long;

constexpr int kCtTile = 32;                       // a tile is 32 x 32 pixels of one class plane
constexpr int kCtSort = kCtTile * kCtTile;        // keys one block sorts in LDS
constexpr int kCtFan = 32;                        // tile lists one block of the second launch merges
constexpr int kCropMaxSide = 16384;

static_assert(PVV_CT_MAX_K <= kBlock && kCtSort == 4 * kBlock, "the merge keeps kBlock keys and takes 3 * kBlock new ones per round");

// Bitonic sort of s[0, kCtSort) in LDS, descending, by the whole block.  The keys of candidates are unique (the flat index is
// part of them), the key of "no candidate" is 0 and sorts behind all of them.  Starts and ends with a barrier.
__device__ void ct_sort_desc(ct_key *s)
{
    for (int k = 2; k <= kCtSort; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int q = threadIdx.x; q < kCtSort / 2; q += kBlock) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const bool desc = (i & k) == 0;
                const ct_key a = s[i], b = s[l];
                if ((a < b) == desc) { s[i] = b; s[l] = a; }
            }
        }
    __syncthreads();
}

// Launch 1, one block per (image, class, tile): nms (D:6-12) as "not smaller than any of the 8 neighbours inside the image",
// a candidate's key = value bits << 32 | ~flat index (a positive float's bits are monotone, the lower index wins a tie), and the
// tile's K largest keys, sorted, to lists[image][class * tiles + tile][K].
__global__ __launch_bounds__(kBlock) void k_ct_tiles(const float *__restrict__ hm, ct_key *__restrict__ lists, int C, int H, int W,
                                                     int tiles_x, int tiles, int K)
{
    __shared__ float s_v[kCtTile + 2][kCtTile + 3];
    __shared__ ct_key s_key[kCtSort];
    const int tile = blockIdx.x % tiles, c = blockIdx.x / tiles, b = blockIdx.y;
    const int x0 = (tile % tiles_x) * kCtTile, y0 = (tile / tiles_x) * kCtTile;
    const float *plane = hm + ((size_t)b * C + c) * H * W;
    for (int i = threadIdx.x; i < (kCtTile + 2) * (kCtTile + 2); i += kBlock) {
        const int ly = i / (kCtTile + 2), lx = i % (kCtTile + 2), y = y0 + ly - 1, x = x0 + lx - 1;
        s_v[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : -INFINITY;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCtSort; i += kBlock) {
        const int ly = i / kCtTile, lx = i % kCtTile, y = y0 + ly, x = x0 + lx;
        ct_key key = 0;
        if (y < H && x < W) {
            const float v = s_v[ly + 1][lx + 1];
            bool peak = v > 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) peak = peak && v >= s_v[ly + dy][lx + dx];
            if (peak) {
                const uint32_t flat = (uint32_t)(((size_t)c * H + y) * W + x);
                key = ((ct_key)__float_as_uint(v) << 32) | (uint32_t)~flat;
            }
        }
        s_key[i] = key;
    }
    ct_sort_desc(s_key);
    ct_key *out = lists + ((size_t)b * gridDim.x + blockIdx.x) * K;
    for (int i = threadIdx.x; i < K; i += kBlock) out[i] = s_key[i];
}

// Launches 2 and 3, one block per (image, group of `fan` lists): the K largest keys of the group.  The block keeps its best
// kBlock keys sorted in front of the LDS array, takes 3 * kBlock new ones behind them and sorts again.  Launch 2 (out != NULL)
// writes the group's list; launch 3 (one group: everything) writes the rows of D:60-69 with U:373-377 applied.
__global__ __launch_bounds__(kBlock) void k_ct_merge(const ct_key *__restrict__ in, int n_lists, int fan, int K, ct_key *__restrict__ out,
                                                     const float *__restrict__ wh, float *__restrict__ ct, float *__restrict__ det,
                                                     int32_t *__restrict__ count, int H, int W, int clip)
{
    __shared__ ct_key s[kCtSort];
    const int g = blockIdx.x, b = blockIdx.y;
    const int lo = g * fan, hi = min(n_lists, lo + fan);
    const ct_key *src = in + ((size_t)b * n_lists + lo) * K;
    const int n = (hi - lo) * K;
    s[threadIdx.x] = 0;
    for (int base = 0; base < n; base += kCtSort - kBlock) {
        for (int i = threadIdx.x; i < kCtSort - kBlock; i += kBlock) s[kBlock + i] = base + i < n ? src[base + i] : 0;
        ct_sort_desc(s);
    }
    if (out) {
        ct_key *o = out + ((size_t)b * gridDim.x + g) * K;
        for (int i = threadIdx.x; i < K; i += kBlock) o[i] = s[i];
        return;
    }
    const int k = threadIdx.x;
    if (k >= K) return;
    const ct_key key = s[k];
    float row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cx = 0.f, cy = 0.f;
    if (key) {
        const uint32_t flat = ~(uint32_t)key, HW = (uint32_t)H * W;
        const uint32_t cls = flat / HW, rem = flat - cls * HW, y = rem / W, x = rem - y * W;
        const float w = wh[(((size_t)b * 2 + 0) * H + y) * W + x], h = wh[(((size_t)b * 2 + 1) * H + y) * W + x];
        cx = (float)x, cy = (float)y;
        row[0] = cx - w / 2.f, row[1] = cy - h / 2.f, row[2] = cx + w / 2.f, row[3] = cy + h / 2.f;
        row[4] = __uint_as_float((uint32_t)(key >> 32)), row[5] = (float)cls;
        if (clip) {                                                                 // (a NaN stays, as under torch.clamp)
            row[0] = row[0] < 0.f ? 0.f : row[0];
            row[1] = row[1] < 0.f ? 0.f : row[1];
            row[2] = row[2] > (float)(W - 1) ? (float)(W - 1) : row[2];
            row[3] = row[3] > (float)(H - 1) ? (float)(H - 1) : row[3];
        }
        if (k == K - 1 || s[k + 1] == 0) count[b] = k + 1;
    } else if (k == 0) {
        count[b] = 0;
    }
    float *d = det + ((size_t)b * K + k) * 6, *c2 = ct + ((size_t)b * K + k) * 2;
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = row[i];
    c2[0] = cx, c2[1] = cy;
}

int ct_check(int B, int C, int H, int W, int K)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(PVV_E_ARG, "ct: B, C, H, W must be positive");
    if (B > 65535) return fail(PVV_E_ARG, "ct: B > 65535: split the batch");
    if ((long long)C * H * W >= (1ll << 31)) return fail(PVV_E_ARG, "ct: C*H*W must be < 2^31 (the flat index is half of the key)");
    if (K < 1 || K > PVV_CT_MAX_K) return fail(PVV_E_ARG, "ct: K must lie in [1, PVV_CT_MAX_K]");
    if (K > (long long)H * W) return fail(PVV_E_ARG, "ct: K must not exceed H*W");
    const long long tiles = (long long)((W + kCtTile - 1) / kCtTile) * ((H + kCtTile - 1) / kCtTile);
    if (C * tiles > (1ll << 22)) return fail(PVV_E_ARG, "ct: more than 2^22 (class, tile) pairs");
    return PVV_OK;
}

struct CtShape { int tiles_x, tiles, n1, n2; size_t lists2, total; };

CtShape ct_shape(int B, int C, int H, int W, int K)
{
    CtShape s;
    s.tiles_x = (W + kCtTile - 1) / kCtTile;
    s.tiles = s.tiles_x * ((H + kCtTile - 1) / kCtTile);
    s.n1 = C * s.tiles;
    s.n2 = (s.n1 + kCtFan - 1) / kCtFan;
    s.lists2 = (sizeof(ct_key) * (size_t)B * s.n1 * K + 255) & ~(size_t)255;
    s.total = s.lists2 + ((sizeof(ct_key) * (size_t)B * s.n2 * K + 255) & ~(size_t)255);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- the crops
struct CropBox {                  // PVV_CROP_WORKSPACE_PER_BOX bytes: what k_crop_prep hands k_crop_warp
    double inv[6];                // crop pixel -> image pixel
    int32_t rx0, ry0, rx1, ry1;   // the inclusive rectangle that is kept (T:65-69), the whole crop without box_ratio
    int32_t valid, img;
    int32_t pad_[6];
};
static_assert(sizeof(CropBox) == PVV_CROP_WORKSPACE_PER_BOX, "pvnet_vote.h promises this size");

struct CropNorm { float mean[3], std[3]; };

// One thread per box: centre and scale (R:16-17, T:58-59), rounded to float32 as the reference keeps them, the crop's map, its
// inverse, and the rectangle of magnify_box (T:65-67).
__global__ void k_crop_prep(const double *__restrict__ boxes, const int32_t *__restrict__ image_index, int N, int B, int ow, int oh,
                            double scale_ratio, int has_box_ratio, double box_ratio, float *__restrict__ center,
                            float *__restrict__ scale, double *__restrict__ trans, uint8_t *__restrict__ valid, CropBox *__restrict__ prm)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double x0 = boxes[4 * n], y0 = boxes[4 * n + 1], x1 = boxes[4 * n + 2], y1 = boxes[4 * n + 3];
    const double cx = (x0 + x1) / 2., cy = (y0 + y1) / 2., bw = x1 - x0, bh = y1 - y0;
    const double s = (bh > bw ? bh : bw) * scale_ratio;
    const float cxf = (float)cx, cyf = (float)cy, sf = (float)s;
    const int img = image_index[n];
    const bool ok = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(cxf) && isfinite(cyf) && isfinite(sf) &&
                    sf > 0.f && img >= 0 && img < B;
    CropBox p;
    p.valid = ok, p.img = ok ? img : 0;
    for (int i = 0; i < 6; ++i) p.inv[i] = 0., p.pad_[i] = 0;
    double M[6] = {0., 0., 0., 0., 0., 0.};
    int32_t r[4] = {0, 0, ow - 1, oh - 1};
    if (ok) {
        crop_transform((double)cxf, (double)cyf, (double)sf, ow, oh, M);
        invert_affine(M, p.inv);
        if (has_box_ratio) magnify_rect(M, x0, y0, x1, y1, box_ratio, ow, oh, r);
    }
    p.rx0 = r[0], p.ry0 = r[1], p.rx1 = r[2], p.ry1 = r[3];
    center[2 * n] = ok ? cxf : 0.f, center[2 * n + 1] = ok ? cyf : 0.f, scale[n] = ok ? sf : 0.f, valid[n] = ok;
    for (int i = 0; i < 6; ++i) trans[6 * n + i] = M[i];
    prm[n] = p;
}

// One thread per crop pixel, 64 along a row: the 8-bit bilinear warp, the blanking, the normalisation of R:25-27, planar stores.
__global__ __launch_bounds__(kBlock) void k_crop_warp(const uint8_t *__restrict__ img, int H, int W, const CropBox *__restrict__ prm,
                                                      int ow, int oh, CropNorm nm, float *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
    if (x >= ow || y >= oh) return;
    const CropBox *p = prm + n;
    int v[3] = {0, 0, 0};
    if (p->valid && x >= p->rx0 && x <= p->rx1 && y >= p->ry0 && y <= p->ry1)
        sample_linear<3>(img + (size_t)p->img * H * W * 3, H, W, p->inv, x, y, v);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[(((size_t)n * 3 + c) * oh + y) * ow + x] = ((float)v[c] / 255.f - nm.mean[c]) / nm.std[c];
}

// One thread per keypoint: E:229-234 (the inverse map applied in binary64).
template <typename T>
__global__ void k_uncrop_kpt(const T *__restrict__ kpt, const double *__restrict__ trans, int N, int K, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    double I[6];
    invert_affine(trans + 6 * (size_t)(i / K), I);
    const double x = (double)kpt[2 * (size_t)i], y = (double)kpt[2 * (size_t)i + 1];
    out[2 * (size_t)i] = I[0] * x + I[1] * y + I[2];
    out[2 * (size_t)i + 1] = I[3] * x + I[4] * y + I[5];
}

// One thread per 4 canvas pixels of a row: E:243-245, the nearest rule with `trans` as the canvas -> crop map, its row half once.
// `vec` (Wc a multiple of 4) stores the four bytes as one word.
__global__ __launch_bounds__(kBlock) void k_uncrop_mask(const uint8_t *__restrict__ mask, int elem, int h, int w,
                                                        const double *__restrict__ trans, int Hc, int Wc, int vec, uint8_t *__restrict__ out)
{
    const int x4 = (blockIdx.x * kBlock + threadIdx.x) * 4, y = blockIdx.y, n = blockIdx.z;
    if (x4 >= Wc) return;
    const double *T = trans + 6 * (size_t)n;
    long long XR, YR;
    warp_nearest_row(T, y, &XR, &YR);
    const uint8_t *m = mask + (size_t)n * h * w * elem;
    uint8_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = x4 + i;
        long long X, Y;
        warp_nearest_col(T, x, XR, YR, &X, &Y);
        if (x < Wc && X >= 0 && X < w && Y >= 0 && Y < h) r[i] = m[((size_t)Y * w + X) * elem];     // (little endian: the low byte)
    }
    uint8_t *o = out + ((size_t)n * Hc + y) * Wc + x4;
    if (vec) {
        *(uint32_t *)o = (uint32_t)r[0] | (uint32_t)r[1] << 8 | (uint32_t)r[2] << 16 | (uint32_t)r[3] << 24;
    } else {
        for (int i = 0; i < 4 && x4 + i < Wc; ++i) o[i] = r[i];
    }
}

}  // namespace

PVV_EXPORT size_t pvv_ct_workspace_bytes(int B, int C, int H, int W, int K)
{
    if (ct_check(B, C, H, W, K)) return 0;
    return ct_shape(B, C, H, W, K).total;
}

PVV_EXPORT int pvv_ct_decode(const float *d_ct_hm, const float *d_wh, int B, int C, int H, int W, int K, int clip, void *d_workspace,
                             size_t workspace_bytes, float *d_ct, float *d_detection, int32_t *d_count, void *stream)
{
    if (int e = ct_check(B, C, H, W, K)) return e;
    if (!d_ct_hm || !d_wh || !d_workspace || !d_ct || !d_detection || !d_count) return fail(PVV_E_ARG, "ct: NULL device pointer");
    if ((uintptr_t)d_workspace % 256 != 0) return fail(PVV_E_ARG, "workspace must be 256-byte aligned");
    const CtShape s = ct_shape(B, C, H, W, K);
    if (workspace_bytes < s.total) return fail(PVV_E_WORKSPACE, "ct: workspace smaller than pvv_ct_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    ct_key *lists1 = (ct_key *)d_workspace, *lists2 = (ct_key *)((char *)d_workspace + s.lists2);
    hipLaunchKernelGGL(k_ct_tiles, dim3(s.n1, B), dim3(kBlock), 0, st, d_ct_hm, lists1, C, H, W, s.tiles_x, s.tiles, K);
    if (int e = check_launch("k_ct_tiles")) return e;
    hipLaunchKernelGGL(k_ct_merge, dim3(s.n2, B), dim3(kBlock), 0, st, lists1, s.n1, kCtFan, K, lists2, nullptr, nullptr, nullptr, nullptr,
                       H, W, 0);
    if (int e = check_launch("k_ct_merge (groups)")) return e;
    hipLaunchKernelGGL(k_ct_merge, dim3(1, B), dim3(kBlock), 0, st, lists2, s.n2, s.n2, K, nullptr, d_wh, d_ct, d_detection, d_count, H, W,
                       clip ? 1 : 0);
    return check_launch("k_ct_merge (rows)");
}

PVV_EXPORT int pvv_crop_boxes(const uint8_t *d_img, int B, int H, int W, const double *d_boxes, const int32_t *d_image_index, int N,
                              int ow, int oh, double scale_ratio, int has_box_ratio, double box_ratio, const float *h_mean,
                              const float *h_std, void *d_workspace, size_t workspace_bytes, float *d_inp, float *d_center,
                              float *d_scale, double *d_trans, uint8_t *d_valid, void *stream)
{
    if (B <= 0 || H <= 0 || W <= 0 || H > kCropMaxSide * 2 || W > kCropMaxSide * 2) return fail(PVV_E_ARG, "crop: B, H, W must be positive, H and W <= 32768");
    if (N <= 0 || N > 65535) return fail(PVV_E_ARG, "crop: N must lie in [1, 65535]");
    if (ow <= 0 || oh <= 0 || ow > kCropMaxSide || oh > kCropMaxSide) return fail(PVV_E_ARG, "crop: out_size must lie in [1, 16384]");
    if (!d_img || !d_boxes || !d_image_index || !h_mean || !h_std || !d_workspace || !d_inp || !d_center || !d_scale || !d_trans || !d_valid)
        return fail(PVV_E_ARG, "crop: NULL pointer");
    if ((uintptr_t)d_workspace % 8 != 0) return fail(PVV_E_ARG, "crop: workspace must be 8-byte aligned");
    if (workspace_bytes < (size_t)N * PVV_CROP_WORKSPACE_PER_BOX) return fail(PVV_E_WORKSPACE, "crop: workspace smaller than N * PVV_CROP_WORKSPACE_PER_BOX");
    hipStream_t st = (hipStream_t)stream;
    CropNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = h_mean[c], nm.std[c] = h_std[c];
    CropBox *prm = (CropBox *)d_workspace;
    hipLaunchKernelGGL(k_crop_prep, dim3((N + 63) / 64), dim3(64), 0, st, d_boxes, d_image_index, N, B, ow, oh, scale_ratio,
                       has_box_ratio ? 1 : 0, box_ratio, d_center, d_scale, d_trans, d_valid, prm);
    if (int e = check_launch("k_crop_prep")) return e;
    hipLaunchKernelGGL(k_crop_warp, dim3((ow + 63) / 64, (oh + 3) / 4, N), dim3(64, 4), 0, st, d_img, H, W, prm, ow, oh, nm, d_inp);
    return check_launch("k_crop_warp");
}

PVV_EXPORT int pvv_uncrop_keypoints(const void *d_kpt_2d, int kpt_is_f64, const double *d_trans, int N, int K, double *d_out, void *stream)
{
    if (N <= 0 || K <= 0 || (long long)N * K >= (1ll << 30)) return fail(PVV_E_ARG, "uncrop_keypoints: N, K must be positive, N*K < 2^30");
    if (!d_kpt_2d || !d_trans || !d_out) return fail(PVV_E_ARG, "uncrop_keypoints: NULL device pointer");
    const dim3 grid((N * K + kBlock - 1) / kBlock);
    if (kpt_is_f64)
        hipLaunchKernelGGL(k_uncrop_kpt<double>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const double *)d_kpt_2d, d_trans, N, K, d_out);
    else
        hipLaunchKernelGGL(k_uncrop_kpt<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const float *)d_kpt_2d, d_trans, N, K, d_out);
    return check_launch("k_uncrop_kpt");
}

PVV_EXPORT int pvv_uncrop_mask(const void *d_mask, int mask_elem_size, int h, int w, const double *d_trans, int N, int Hc, int Wc,
                               uint8_t *d_out, void *stream)
{
    if (N <= 0 || N > 65535) return fail(PVV_E_ARG, "uncrop_mask: N must lie in [1, 65535]");
    if (h <= 0 || w <= 0 || h > kCropMaxSide || w > kCropMaxSide) return fail(PVV_E_ARG, "uncrop_mask: the crop's sides must lie in [1, 16384]");
    if (Hc <= 0 || Wc <= 0 || Hc > 65535 || Wc > 65535) return fail(PVV_E_ARG, "uncrop_mask: the canvas' sides must lie in [1, 65535]");
    if (mask_elem_size != 1 && mask_elem_size != 8) return fail(PVV_E_ARG, "uncrop_mask: mask_elem_size must be 1 or 8");
    if (!d_mask || !d_trans || !d_out) return fail(PVV_E_ARG, "uncrop_mask: NULL device pointer");
    const int vec = Wc % 4 == 0 && (uintptr_t)d_out % 4 == 0;
    hipLaunchKernelGGL(k_uncrop_mask, dim3((Wc + 4 * kBlock - 1) / (4 * kBlock), Hc, N), dim3(kBlock), 0, (hipStream_t)stream,
                       (const uint8_t *)d_mask, mask_elem_size, h, w, d_trans, Hc, Wc, vec, d_out);
    return check_launch("k_uncrop_mask");
}
