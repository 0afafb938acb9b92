// ct_augment.hpp -- the detector's training batch from cut-outs and a background, and its input preparation (include/pvnet_vote.h,
// "Detector augmentation").  Part of pvnet_vote.hip: built with -ffp-contract=off, every float and double operation below rounds
// once, in the order written, so that the numpy twin (tests/ct_augment_twin.py) gives the same bits.  The two fixed-point warp
// rules, the box accumulator, the placement record and its coverage test are those of warp.hpp, the wave
// reductions and the block tree those of vote_common.hpp, TrainVec4 that of train.hpp.  No random numbers and no
// transcendental function are evaluated here: the host hands over the inverse maps, the rounded alphas and the lighting
// vector.  The grey mean is the only floating-point sum: binary64, per 64 x 4 tile in the block tree, then per image in the
// same tree over slots; every other reduction is over integers.
//
// Reference behaviour restated:
//   U = lib/utils/tless/tless_utils.py (augment :18-63, cut_and_paste :86-97)
//   C = lib/datasets/tless/ct.py:58-70 (Dataset.get_bbox)      C' = lib/datasets/tless_train/ct.py:75-76
//   G = lib/utils/data_utils.py (grayscale :172-173, lighting_ .. contrast_ :176-199, color_aug :202-210)
#pragma once

#include "train.hpp"
#include "warp.hpp"

namespace {

constexpr int kCtaMaxN = PVV_CT_AUGMENT_MAX_N;
constexpr int kCtaMaxSide = 16384;

struct CtaParam {                 // PVV_CT_AUGMENT_PARAM_BYTES per sample, built by the host from the draws
    double inv_in[6], inv_out[6]; // input image -> canvas, output map -> canvas
    double light[3];              // eigvec . (eigval * alpha), added per channel
    float a[3], oma[3];           // alpha and 1 - alpha of the steps in the drawn order
    int32_t order[3], pad_;       // 0 brightness, 1 contrast, 2 saturation
};
static_assert(sizeof(CtaParam) == PVV_CT_AUGMENT_PARAM_BYTES, "pvnet_vote.h promises this size");

struct CtaNorm { float mean[3], std[3]; };

// The block's four waves' maxima of four values; the result is valid in thread 0.
__device__ void cta_block_max4(int *v, int (*sh)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_max(v[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) sh[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) v[k] = max(max(sh[0][k], sh[1][k]), max(sh[2][k], sh[3][k]));
}

// Launch 1 of the composition, one block per (instance, sample): the box of mask != 0 (U:87-90) and the placement (U:93).
// The mask is read four bytes at a time when its planes are 4-byte aligned.
__global__ __launch_bounds__(kBlock) void k_cta_place(const uint8_t *__restrict__ mask, const int32_t *__restrict__ num,
                                                      const double *__restrict__ u, int N, int h, int w, int H, int W, int vec,
                                                      int32_t *__restrict__ place)
{
    __shared__ int s_r[4][4];
    const int n = blockIdx.x, b = blockIdx.y;
    const size_t inst = (size_t)b * N + n;
    Extent e = {{0, 0, 0, 0}};
    if (n < num[b]) {
        const size_t hw = (size_t)h * w;
        const uint8_t *m = mask + inst * hw;
        if (vec) {
            const uint32_t *m4 = reinterpret_cast<const uint32_t *>(m);
            for (size_t i = threadIdx.x; i < hw / 4; i += kBlock) {
                const uint32_t q = m4[i];
                if (q == 0) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((q >> (8 * j)) & 255u) {
                        const size_t p = 4 * i + j;
                        const int y = (int)(p / (size_t)w);
                        e.add((int)(p - (size_t)y * w), y);
                    }
            }
        } else {
            for (size_t p = threadIdx.x; p < hw; p += kBlock)
                if (m[p] != 0) {
                    const int y = (int)(p / (size_t)w);
                    e.add((int)(p - (size_t)y * w), y);
                }
        }
    }
    cta_block_max4(e.v, s_r);
    if (threadIdx.x == 0) place_record(e, H, W, u[2 * inst], u[2 * inst + 1], place + 6 * inst);      // (empty beyond num[b])
}

// Launch 2 of the composition, one lane per canvas pixel, 64 along a row: the last instance whose mask covers the pixel owns
// it (U:94-97 as a gather).  The records are uniform loads.
__global__ __launch_bounds__(kBlock) void k_cta_paste(const uint8_t *__restrict__ bg, const uint8_t *__restrict__ inst_img,
                                                      const uint8_t *__restrict__ inst_mask, const int32_t *__restrict__ num,
                                                      const int32_t *__restrict__ place, int H, int W, int N, int h, int w,
                                                      uint8_t *__restrict__ img, uint8_t *__restrict__ label)
{
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (X >= W || Y >= H) return;
    const int cnt = min(num[b], N);
    int owner = 0;
    size_t src = 0;
    for (int n = cnt - 1; n >= 0; --n) {
        const size_t inst = (size_t)b * N + n;
        if (const uint8_t *m = place_covers(place + 6 * inst, inst_mask + inst * h * w, h, w, X, Y)) {
            owner = n + 1, src = (size_t)(m - inst_mask);
            break;
        }
    }
    const size_t o = ((size_t)b * H + Y) * W + X;
    const uint8_t *s = owner ? inst_img + src * 3 : bg + o * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) img[o * 3 + c] = s[c];
    label[o] = (uint8_t)owner;
}

// G:172-173 on x = (float)u8 / 255.f, channel 0 the blue one
__device__ float cta_grey(const float *x) { return (x[0] * 0.114f + x[1] * 0.587f) + x[2] * 0.299f; }

// Launch 1 of the augmentation, one lane per pixel of the input image, 64 along a row (U:47): the warp, and with GREY the
// tile's binary64 sum of the grey level to part[b][tile].
template <bool GREY>
__global__ __launch_bounds__(kBlock) void k_cta_warp(const uint8_t *__restrict__ img, int H, int W, const CtaParam *__restrict__ prm,
                                                     int ih, int iw, uint8_t *__restrict__ orig, double *__restrict__ part)
{
    __shared__ double s_sum[GREY ? kBlock : 1];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    double g = 0.;
    if (x < iw && y < ih) {
        uint8_t *o = orig + (((size_t)b * ih + y) * iw + x) * 3;
        float f[3];
        sample_linear_to<3>(img + (size_t)b * H * W * 3, H, W, prm[b].inv_in, x, y,
                            [&](int c, int v) { o[c] = (uint8_t)v, f[c] = (float)v / 255.f; });      // (stored as it comes: a register less)
        if constexpr (GREY) g = (double)cta_grey(f);
    }
    if constexpr (GREY) {
        const int tid = threadIdx.y * 64 + threadIdx.x;
        const double sum = block_tree_sum(g, s_sum, tid);
        if (tid == 0) part[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
    }
}

// Launch 2, one block per image: slot j sums the tiles j, j + 256, ... in that order, the slots in the same tree; the mean is
// rounded to float32 once (G:207).
__global__ __launch_bounds__(kBlock) void k_cta_mean(const double *__restrict__ part, int tiles, long long count, float *__restrict__ mean)
{
    __shared__ double s_sum[kBlock];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.;
    for (int i = tid; i < tiles; i += kBlock) s += part[(size_t)b * tiles + i];
    s = block_tree_sum(s, s_sum, tid);
    if (tid == 0) mean[b] = (float)(s / (double)count);
}

// One pixel of launch 3: G:202-210 in the drawn order on x = u8 / 255, then U:56.
__device__ __forceinline__ void cta_colour(const CtaParam *p, float gs_mean, const CtaNorm &nm, const int *v, float *out)
{
    float x[3] = {(float)v[0] / 255.f, (float)v[1] / 255.f, (float)v[2] / 255.f};
    if (p) {
        const float gs = cta_grey(x);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int op = p->order[s];
            const float a = p->a[s];
            const float t = op == 0 ? 0.f : (op == 1 ? gs_mean : gs) * p->oma[s];     // blend_'s image2 *= (1 - alpha)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[c] = x[c] * a;
                if (op != 0) x[c] = x[c] + t;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = (float)((double)x[c] + p->light[c]);     // image += a binary64 vector
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (x[c] - nm.mean[c]) / nm.std[c];
}

// Launch 3, streaming: VEC, a lane owns four pixels of a row (iw % 4 == 0, orig 4-byte and out 16-byte aligned): three 4-byte
// loads, one 16-byte store per plane; otherwise one pixel per lane.  prm is NULL without colour steps.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cta_colour(const uint8_t *__restrict__ orig, int ih, int iw, const CtaParam *__restrict__ prm,
                                                       const float *__restrict__ gs_mean, CtaNorm nm, float *__restrict__ out)
{
    constexpr int P = VEC ? 4 : 1;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * P, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (x0 >= iw || y >= ih) return;
    const CtaParam *p = prm ? prm + b : nullptr;
    const float gm = prm ? gs_mean[b] : 0.f;
    const uint8_t *src = orig + (((size_t)b * ih + y) * iw + x0) * 3;
    uint8_t px[3 * P];
    if constexpr (VEC) {
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t q = s4[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) px[4 * k + j] = (uint8_t)(q >> (8 * j));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = src[k];
    }
    float r[3][P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int v[3] = {px[3 * i], px[3 * i + 1], px[3 * i + 2]};
        float o[3];
        cta_colour(p, gm, nm, v, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c][i] = o[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *dst = out + (((size_t)b * 3 + c) * ih + y) * iw + x0;
        if constexpr (VEC) {
            TrainVec4<float> q;
#pragma unroll
            for (int i = 0; i < 4; ++i) q.v[i] = r[c][i];
            *reinterpret_cast<TrainVec4<float> *>(dst) = q;
        } else {
            dst[0] = r[c][0];
        }
    }
}

// A tap of the label map, tested before its address is formed; 0 outside.
__device__ int cta_label(const uint8_t *__restrict__ lab, int H, int W, long long sx, long long sy)
{
    if (sx < 0 || sx >= W || sy < 0 || sy >= H) return 0;
    return lab[(size_t)sy * W + (size_t)sx];
}

// Launch 4, one lane per pixel of the output map, 64 along a row, all instances at once (C:60-66): the lane's taps, then per
// instance the wave's row into the box st[b][i], zeroed before.  LINEAR: the labels of the taps that carry weight.
template <bool LINEAR>
__global__ __launch_bounds__(kBlock) void k_cta_boxes(const uint8_t *__restrict__ label, int H, int W, const CtaParam *__restrict__ prm,
                                                      int N, int oh, int ow, Extent *__restrict__ st)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    int lab[4] = {0, 0, 0, 0};
    if (x < ow && y < oh) {
        const uint8_t *lb = label + (size_t)b * H * W;
        const double *I = prm[b].inv_out;
        if constexpr (LINEAR) {
            long long sx, sy;
            int a, bb;
            warp_linear_coords(I, x, y, &sx, &sy, &a, &bb);
            lab[0] = cta_label(lb, H, W, sx, sy);                                    // (32 - a) * (32 - bb) > 0 always
            if (a) lab[1] = cta_label(lb, H, W, sx + 1, sy);
            if (bb) lab[2] = cta_label(lb, H, W, sx, sy + 1);
            if (a && bb) lab[3] = cta_label(lb, H, W, sx + 1, sy + 1);
        } else {
            sample_nearest<1>(lb, H, W, I, x, y, lab);
        }
    }
    for (int i = 0; i < N; ++i) {
        const int id = i + 1;
        const bool hit = lab[0] == id || lab[1] == id || lab[2] == id || lab[3] == id;
        if (__ballot(hit) == 0) continue;                                            // the same for the wave's lanes
        st[(size_t)b * N + i].note(hit, x, y);
    }
}

// Launch 5, one lane per instance: cv2.boundingRect as (x, y, x + w, y + h), then C:67-68.
__global__ __launch_bounds__(kBlock) void k_cta_box_finish(const Extent *__restrict__ st, int count, int oh, int ow, int32_t *__restrict__ boxes)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    int32_t *o = boxes + 4 * (size_t)i;
    if (st[i].empty()) {
        o[0] = o[1] = o[2] = o[3] = 0;
        return;
    }
    int box[4];
    st[i].decode(box);
    o[0] = box[0], o[1] = box[1], o[2] = min(box[2] + 1, ow - 1), o[3] = min(box[3] + 1, oh - 1);
}

int cta_check(int B, int H, int W, const char *what)
{
    if (B <= 0 || B > 65535) return fail(PVV_E_ARG, "ct_augment: B must lie in [1, 65535]");
    if (H <= 0 || W <= 0 || H > kCtaMaxSide || W > kCtaMaxSide) return fail(PVV_E_ARG, what);
    return PVV_OK;
}

struct CtaLayout { size_t boxes, part, mean, total; int tx, ty; };

CtaLayout cta_layout(int B, int N, int ih, int iw)
{
    CtaLayout L;
    L.tx = (iw + 63) / 64, L.ty = (ih + 3) / 4;
    L.boxes = 0;
    L.part = align_up(sizeof(Extent) * (size_t)B * N);
    L.mean = L.part + align_up(sizeof(double) * (size_t)B * L.tx * L.ty);
    L.total = L.mean + align_up(sizeof(float) * (size_t)B);
    return L;
}

}  // namespace

PVV_EXPORT int pvv_ct_compose(const uint8_t *d_bg, const uint8_t *d_inst_img, const uint8_t *d_inst_mask, const int32_t *d_num,
                              const double *d_place_u, int B, int H, int W, int N, int h, int w, uint8_t *d_img, uint8_t *d_label,
                              int32_t *d_place, void *stream)
{
    if (int e = cta_check(B, H, W, "ct_compose: the canvas' sides must lie in [1, 16384]")) return e;
    if (int e = cta_check(B, h, w, "ct_compose: the cut-outs' sides must lie in [1, 16384]")) return e;
    if (N < 1 || N > kCtaMaxN) return fail(PVV_E_ARG, "ct_compose: N must lie in [1, 16]");
    if (!d_bg || !d_inst_img || !d_inst_mask || !d_num || !d_place_u || !d_img || !d_label || !d_place)
        return fail(PVV_E_ARG, "ct_compose: NULL device pointer");
    if ((uintptr_t)d_place_u % 8 != 0 || (uintptr_t)d_place % 4 != 0 || (uintptr_t)d_num % 4 != 0)
        return fail(PVV_E_ARG, "ct_compose: place_u must be 8-byte aligned, place and num 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int vec = ((size_t)h * w) % 4 == 0 && (uintptr_t)d_inst_mask % 4 == 0;
    hipLaunchKernelGGL(k_cta_place, dim3(N, B), dim3(kBlock), 0, st, d_inst_mask, d_num, d_place_u, N, h, w, H, W, vec, d_place);
    if (int e = check_launch("k_cta_place")) return e;
    hipLaunchKernelGGL(k_cta_paste, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, st, d_bg, d_inst_img, d_inst_mask, d_num, d_place, H, W,
                       N, h, w, d_img, d_label);
    return check_launch("k_cta_paste");
}

PVV_EXPORT size_t pvv_ct_augment_workspace_bytes(int B, int N, int ih, int iw)
{
    if (cta_check(B, ih, iw, "ct_augment: the input's sides must lie in [1, 16384]")) return 0;
    if (N < 0 || N > kCtaMaxN) {
        fail(PVV_E_ARG, "ct_augment: N must lie in [0, 16]");
        return 0;
    }
    return cta_layout(B, N, ih, iw).total;
}

PVV_EXPORT int pvv_ct_augment(const uint8_t *d_img, const uint8_t *d_label, int B, int H, int W, int N, int ih, int iw, int oh, int ow,
                              int train, int boxes_mode, const void *d_params, const float *h_mean, const float *h_std, void *d_workspace,
                              size_t workspace_bytes, uint8_t *d_orig, float *d_inp, int32_t *d_boxes, void *stream)
{
    if (int e = cta_check(B, H, W, "ct_augment: the image's sides must lie in [1, 16384]")) return e;
    if (int e = cta_check(B, ih, iw, "ct_augment: the input's sides must lie in [1, 16384]")) return e;
    if (!d_label) N = 0;
    if (d_label && (N < 1 || N > kCtaMaxN)) return fail(PVV_E_ARG, "ct_augment: N must lie in [1, 16]");
    if (d_label && (oh < 1 || ow < 1 || oh > ih || ow > iw)) return fail(PVV_E_ARG, "ct_augment: the output map's sides must lie in [1, the input's]");
    if (boxes_mode != PVV_CT_BOXES_LINEAR && boxes_mode != PVV_CT_BOXES_NEAREST) return fail(PVV_E_ARG, "ct_augment: unknown boxes mode");
    if (!d_img || !d_params || !h_mean || !h_std || !d_workspace || !d_orig || !d_inp || (d_label && !d_boxes))
        return fail(PVV_E_ARG, "ct_augment: NULL pointer");
    if ((uintptr_t)d_workspace % 8 != 0 || (uintptr_t)d_params % 8 != 0 || (uintptr_t)d_inp % 4 != 0 || (uintptr_t)d_boxes % 4 != 0)
        return fail(PVV_E_ARG, "ct_augment: workspace and params must be 8-byte aligned, inp and boxes 4-byte aligned");
    const CtaLayout L = cta_layout(B, N, ih, iw);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "ct_augment: workspace smaller than pvv_ct_augment_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    const CtaParam *prm = (const CtaParam *)d_params;
    Extent *box_state = (Extent *)((uint8_t *)d_workspace + L.boxes);
    double *part = (double *)((uint8_t *)d_workspace + L.part);
    float *gs_mean = (float *)((uint8_t *)d_workspace + L.mean);
    const dim3 grid_in(L.tx, L.ty, B), block(64, 4);
    if (train) {
        hipLaunchKernelGGL(k_cta_warp<true>, grid_in, block, 0, st, d_img, H, W, prm, ih, iw, d_orig, part);
        if (int e = check_launch("k_cta_warp")) return e;
        hipLaunchKernelGGL(k_cta_mean, dim3(B), dim3(kBlock), 0, st, part, L.tx * L.ty, (long long)ih * iw, gs_mean);
        if (int e = check_launch("k_cta_mean")) return e;
    } else {
        hipLaunchKernelGGL(k_cta_warp<false>, grid_in, block, 0, st, d_img, H, W, prm, ih, iw, d_orig, part);
        if (int e = check_launch("k_cta_warp")) return e;
    }
    CtaNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = h_mean[c], nm.std[c] = h_std[c];
    const CtaParam *colour = train ? prm : nullptr;
    if (iw % 4 == 0 && (uintptr_t)d_orig % 4 == 0 && (uintptr_t)d_inp % 16 == 0)
        hipLaunchKernelGGL(k_cta_colour<true>, dim3((iw / 4 + 63) / 64, L.ty, B), block, 0, st, d_orig, ih, iw, colour, gs_mean, nm, d_inp);
    else
        hipLaunchKernelGGL(k_cta_colour<false>, grid_in, block, 0, st, d_orig, ih, iw, colour, gs_mean, nm, d_inp);
    if (int e = check_launch("k_cta_colour")) return e;
    if (!d_label) return PVV_OK;
    if (hipMemsetAsync(box_state, 0, sizeof(Extent) * (size_t)B * N, st) != hipSuccess) return fail(PVV_E_ARG, "ct_augment: hipMemsetAsync failed");
    const dim3 grid_out((ow + 63) / 64, (oh + 3) / 4, B);
    if (boxes_mode == PVV_CT_BOXES_LINEAR)
        hipLaunchKernelGGL(k_cta_boxes<true>, grid_out, block, 0, st, d_label, H, W, prm, N, oh, ow, box_state);
    else
        hipLaunchKernelGGL(k_cta_boxes<false>, grid_out, block, 0, st, d_label, H, W, prm, N, oh, ow, box_state);
    if (int e = check_launch("k_cta_boxes")) return e;
    hipLaunchKernelGGL(k_cta_box_finish, dim3((B * N + kBlock - 1) / kBlock), dim3(kBlock), 0, st, box_state, B * N, oh, ow, d_boxes);
    return check_launch("k_cta_box_finish");
}
