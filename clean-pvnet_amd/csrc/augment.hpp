// augment.hpp -- PVNet's training augmentation and loader transforms for a batch (include/pvnet_vote.h, "Training augmentation").
// Part of pvnet_vote.hip: built with -ffp-contract=off, every float and double operation below rounds once, in the order
// written, so that the numpy twin (tests/augment_twin.py) gives the same bits.  sat_rint, invert_affine, the two fixed-point
// warp rules and the box accumulator are those of warp.hpp, the wave reductions those of
// vote_common.hpp.  No random numbers and no transcendental function are evaluated here: the host hands over the drawn values,
// cos and sin included.  Every reduction is over integers.
//
// Reference behaviour restated:
//   P = lib/datasets/linemod/pvnet.py:62-78 (augment)        A = lib/datasets/augmentation.py (rotate_instance :60-69,
//   crop_or_padding_to_fixed_size_instance :126-167, crop_or_padding_to_fixed_size :170-196, crop_resize_instance_v1 :266-295)
//   X = lib/datasets/transforms.py:29-99 (ToTensor, Normalize, ColorJitter, RandomBlur, make_transforms)
#pragma once

#include "warp.hpp"

namespace {

constexpr int kAugMaxSide = 16384;
constexpr int kBlurTile = 16;                     // rows of a blur tile; it is 64 wide
constexpr int kBlurHalo = 4;                      // the 9-tap table reaches 4 pixels

struct AugDraw {                  // PVV_AUGMENT_PARAM_BYTES per sample, built by the host from the draws
    double cs, sn, ratio;         // cos and sin of the drawn degree, the drawn resize ratio
    double u_h, u_w;              // the uniforms that place the window
    int32_t th, tw;               // int(height * ratio), int(width * ratio)
};
static_assert(sizeof(AugDraw) == PVV_AUGMENT_PARAM_BYTES, "pvnet_vote.h promises this size");

struct AugState {                 // per sample, in the workspace; zeroed before the first launch
    unsigned long long n, sx, sy; // the foreground's moments
    Extent box;                   // the rotated mask's box
    double M[6], inv[6];          // image -> rotated image, and its inverse
    int32_t path, th, tw, hbeg, wbeg, pad_h, pad_w, pad_;
};

struct AugJitter {                // PVV_TRANSFORM_PARAM_BYTES per sample, built by the host from the draws
    int32_t k;                    // the blur's size, 0 for none
    int32_t w[9];                 // its taps, centred on w[4], summing to 256
    float f[3];                   // the factors of brightness, contrast, saturation
    int32_t hue;                  // what is added to PIL's 8-bit hue, modulo 256: int(factor * 255) & 255
    int32_t order[4];             // the operations in the drawn order: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none
};
static_assert(sizeof(AugJitter) == PVV_TRANSFORM_PARAM_BYTES, "pvnet_vote.h promises this size");

struct AugNorm { double mean[3], std[3]; };

// cv2.getRotationMatrix2D((cx, cy), degree, 1) around the foreground's centre (A:63-64).
__device__ void aug_matrix(const AugState *s, double a, double b, double *M)
{
    const double cx = (double)s->sx / (double)s->n, cy = (double)s->sy / (double)s->n;
    M[0] = a, M[1] = b, M[2] = (1. - a) * cx - b * cy;
    M[3] = -b, M[4] = a, M[5] = b * cx + (1. - a) * cy;
}

// Launch 1, 8 pixels of the flattened mask per lane: n, sum x, sum y over mask != 0 (A:63).
__global__ __launch_bounds__(kBlock) void k_aug_moments(const uint8_t *__restrict__ mask, int H, int W, AugState *__restrict__ st)
{
    const int b = blockIdx.y;
    const long long HW = (long long)H * W;
    const uint8_t *m = mask + (size_t)b * HW;
    int n = 0, sx = 0, sy = 0;
    for (int j = 0; j < 8; ++j) {
        const long long i = ((long long)blockIdx.x * 8 + j) * kBlock + threadIdx.x;
        if (i < HW && m[i] != 0) {
            const int y = (int)(i / W);
            n += 1, sx += (int)(i - (long long)y * W), sy += y;
        }
    }
    n = wave_sum(n), sx = wave_sum(sx), sy = wave_sum(sy);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&st[b].n, (unsigned long long)n);
        atomicAdd(&st[b].sx, (unsigned long long)sx);
        atomicAdd(&st[b].sy, (unsigned long long)sy);
    }
}

// Launch 2, one lane per pixel of the rotated mask, which is not written: its box (A:130-131).
__global__ __launch_bounds__(kBlock) void k_aug_box(const uint8_t *__restrict__ mask, int H, int W, const AugDraw *__restrict__ dr,
                                                    AugState *__restrict__ st)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    AugState *s = st + b;
    if (s->n == 0) return;
    double M[6], I[6];
    aug_matrix(s, dr[b].cs, dr[b].sn, M);
    invert_affine(M, I);
    int v = 0;
    if (x < W && y < H) sample_nearest<1>(mask + (size_t)b * H * W, H, W, I, x, y, &v);
    s->box.note(v != 0, x, y);
}

// Launch 3, one block per sample: the branch (P:68), the window (A:126-144, 157-158 or A:170-176, 188-189) and the keypoints
// (A:68, 149-150, 162-163, 292-293).
template <typename T>
__global__ __launch_bounds__(64) void k_aug_window(AugState *__restrict__ st, const AugDraw *__restrict__ dr, const T *__restrict__ kpt,
                                                   int K, int H, int W, int oh, int ow, double overlap, double *__restrict__ out_kpt,
                                                   int32_t *__restrict__ path_out, int32_t *__restrict__ window)
{
    const int b = blockIdx.x;
    AugState *s = st + b;
    const AugDraw d = dr[b];
    const int path = s->n == 0 ? 0 : s->box.empty() ? 2 : 1;
    const int th = path == 1 ? d.th : oh, tw = path == 1 ? d.tw : ow;
    const bool hpad = th >= H, wpad = tw >= W;
    int hlo = 0, hhi = H - th, wlo = 0, whi = W - tw;
    double M[6] = {1., 0., 0., 0., 1., 0.}, I[6] = {1., 0., 0., 0., 1., 0.};
    if (path == 1) {
        aug_matrix(s, d.cs, d.sn, M);
        invert_affine(M, I);
        int box[4];
        s->box.decode(box);
        const int wmin = box[0], hmin = box[1], wmax = box[2], hmax = box[3];
        const double vh = (double)hmin + overlap * (double)(hmax - hmin), vw = (double)wmin + overlap * (double)(wmax - wmin);
        const double h_th = (double)(H - th), w_tw = (double)(W - tw), hl = vh - (double)th, wl = vw - (double)tw;
        hhi = (int)(vh < h_th ? vh : h_th), hlo = (int)(hl > 0. ? hl : 0.);
        whi = (int)(vw < w_tw ? vw : w_tw), wlo = (int)(wl > 0. ? wl : 0.);
    }
    const int hbeg = hpad ? 0 : uniform_randint(hlo, hhi, d.u_h), wbeg = wpad ? 0 : uniform_randint(wlo, whi, d.u_w);
    const int pad_h = hpad ? (th - H) / 2 : 0, pad_w = wpad ? (tw - W) / 2 : 0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < 6; ++i) s->M[i] = M[i], s->inv[i] = I[i];
        s->path = path, s->th = th, s->tw = tw, s->hbeg = hbeg, s->wbeg = wbeg, s->pad_h = pad_h, s->pad_w = pad_w;
        path_out[b] = path;
        int32_t *w = window + 6 * (size_t)b;
        w[0] = th, w[1] = tw, w[2] = hbeg, w[3] = wbeg, w[4] = pad_h, w[5] = pad_w;
    }
    for (int k = threadIdx.x; k < K; k += 64) {
        const size_t i = (size_t)b * K + k;
        double x = (double)kpt[2 * i], y = (double)kpt[2 * i + 1];
        if (path == 1) {
            const double xr = (M[0] * x + M[1] * y) + M[2], yr = (M[3] * x + M[4] * y) + M[5];
            x = xr - (double)wbeg, y = yr - (double)hbeg;
            if (hpad || wpad) x = x + (double)pad_w, y = y + (double)pad_h;
            x = x / d.ratio, y = y / d.ratio;
        }
        out_kpt[2 * i] = x, out_kpt[2 * i + 1] = y;
    }
}

// The two taps of the 8-bit bilinear resize along one axis: `src` pixels onto `dst`, destination index d.
__device__ void aug_resize_taps(int d, int src, int dst, int *s0, int *s1, int *w0, int *w1)
{
    const double scale = (double)src / (double)dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    int s = (int)fl;
    f -= fl;
    if (s < 0) s = 0, f = 0.f;
    if (s >= src - 1) s = src - 1, f = 0.f;
    *s0 = s, *s1 = min(s + 1, src - 1);
    *w0 = (int)rintf((1.f - f) * 2048.f), *w1 = (int)rintf(f * 2048.f);
}

// Launch 4, one lane per pixel of the th x tw window, 64 along a row: the rotated image (the 8-bit bilinear warp) inside the
// zero-padded window (A:66, 146-165) to win [B,TH,TW,3] in the workspace; samples on paths 0 and 2 write nothing.  (Recomputing the four rotated pixels
// per resize tap instead, without this image, gives the same bytes and measured 1.5 x slower at 32 x 480 x 640.)
__global__ __launch_bounds__(kBlock) void k_aug_rotate(const uint8_t *__restrict__ img, int H, int W, const AugState *__restrict__ st, int TH,
                                                       int TW, uint8_t *__restrict__ win)
{
    const int wx = blockIdx.x * 64 + threadIdx.x, wy = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    const AugState *s = st + b;
    if (s->path != 1 || wx >= s->tw || wy >= s->th || wx >= TW || wy >= TH) return;
    const long long x = (long long)wx + (s->wbeg - s->pad_w), y = (long long)wy + (s->hbeg - s->pad_h);      // window -> image
    int v[3] = {0, 0, 0};
    if (x >= 0 && x < W && y >= 0 && y < H) sample_linear<3>(img + (size_t)b * H * W * 3, H, W, s->inv, (int)x, (int)y, v);
    uint8_t *o = win + (((size_t)b * TH + wy) * TW + wx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
}

// A tap of the window image, tested before its address is formed.
__device__ void aug_window_pixel(const uint8_t *__restrict__ win, int TH, int TW, int x, int y, int *v)
{
    v[0] = v[1] = v[2] = 0;
    if (x < 0 || x >= TW || y < 0 || y >= TH) return;
    const uint8_t *p = win + ((size_t)y * TW + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = p[c];
}

// Launch 5, one lane per output pixel, 64 along a row.  Path 1: the window scaled to the output (A:289-290), the mask through
// both nearest-neighbour rules at once; paths 0 and 2: the crop or pad of the image as it is (A:170-196).
__global__ __launch_bounds__(kBlock) void k_aug_render(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask, int H, int W,
                                                       const AugState *__restrict__ st, int oh, int ow, const uint8_t *__restrict__ win,
                                                       int TH, int TW, uint8_t *__restrict__ out_img, uint8_t *__restrict__ out_mask)
{
    const int dx = blockIdx.x * 64 + threadIdx.x, dy = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (dx >= ow || dy >= oh) return;
    const AugState *s = st + b;
    const uint8_t *base = img + (size_t)b * H * W * 3, *m = mask + (size_t)b * H * W;
    const int ox = s->wbeg - s->pad_w, oy = s->hbeg - s->pad_h;               // window -> image
    int v[3] = {0, 0, 0}, mv = 0;
    if (s->path == 1) {
        int x0, x1, a0, a1, y0, y1, b0, b1, p[4][3];
        aug_resize_taps(dx, s->tw, ow, &x0, &x1, &a0, &a1);
        aug_resize_taps(dy, s->th, oh, &y0, &y1, &b0, &b1);
        const uint8_t *wb = win + (size_t)b * TH * TW * 3;
        aug_window_pixel(wb, TH, TW, x0, y0, p[0]);
        aug_window_pixel(wb, TH, TW, x1, y0, p[1]);
        aug_window_pixel(wb, TH, TW, x0, y1, p[2]);
        aug_window_pixel(wb, TH, TW, x1, y1, p[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int S0 = p[0][c] * a0 + p[1][c] * a1, S1 = p[2][c] * a0 + p[3][c] * a1;
            v[c] = (b0 * S0 + b1 * S1 + (1 << 21)) >> 22;
        }
        const long long wx = min((long long)floor((double)dx * ((double)s->tw / (double)ow)), (long long)s->tw - 1);
        const long long wy = min((long long)floor((double)dy * ((double)s->th / (double)oh)), (long long)s->th - 1);
        const long long rx = wx + ox, ry = wy + oy;
        if (rx >= 0 && rx < W && ry >= 0 && ry < H) sample_nearest<1>(m, H, W, s->inv, (int)rx, (int)ry, &mv);
    } else {
        const long long x = (long long)dx + ox, y = (long long)dy + oy;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t i = (size_t)y * W + (size_t)x;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = base[i * 3 + c];
            mv = m[i];
        }
    }
    const size_t o = ((size_t)b * oh + dy) * ow + dx;
#pragma unroll
    for (int c = 0; c < 3; ++c) out_img[o * 3 + c] = (uint8_t)v[c];
    out_mask[o] = (uint8_t)mv;
}

// ---------------------------------------------------------------------------------------------------------- the transforms
// cv2.BORDER_REFLECT_101, then clamped: a tile's lanes past the image read a valid pixel that no kept result uses
__device__ int aug_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// One block per 64 x 16 tile: the tile with its halo staged in LDS, rows T = sum w*p, columns (sum w*T + 2^15) >> 16 (X:69-78).
__global__ __launch_bounds__(kBlock) void k_aug_blur(const uint8_t *__restrict__ img, int h, int w, const AugJitter *__restrict__ prm,
                                                     uint8_t *__restrict__ out)
{
    constexpr int R = kBlurHalo, TH = kBlurTile + 2 * R, TW = 64 + 2 * R;
    __shared__ uint8_t s_p[TH][TW][3];
    __shared__ uint16_t s_t[TH][64][3];
    const int b = blockIdx.z, x0 = blockIdx.x * 64, y0 = blockIdx.y * kBlurTile, tid = threadIdx.y * 64 + threadIdx.x;
    const uint8_t *base = img + (size_t)b * h * w * 3;
    int wt[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) wt[j] = prm[b].k ? prm[b].w[j] : (j == R ? 256 : 0);
    for (int i = tid; i < TH * TW; i += kBlock) {
        const int ly = i / TW, lx = i % TW;
        const size_t g = ((size_t)aug_reflect(y0 + ly - R, h) * w + aug_reflect(x0 + lx - R, w)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_p[ly][lx][c] = base[g + c];
    }
    __syncthreads();
    for (int i = tid; i < TH * 64; i += kBlock) {
        const int ly = i / 64, lx = i % 64;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int t = 0;
#pragma unroll
            for (int j = 0; j < 9; ++j) t += wt[j] * s_p[ly][lx + j][c];
            s_t[ly][lx][c] = (uint16_t)t;                                      // at most 255 * 256
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    for (int r = threadIdx.y; r < kBlurTile; r += 4) {
        const int y = y0 + r;
        if (x >= w || y >= h) continue;
        uint8_t *o = out + (((size_t)b * h + y) * w + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int t = 0;
#pragma unroll
            for (int j = 0; j < 9; ++j) t += wt[j] * s_t[r + j][threadIdx.x][c];
            o[c] = (uint8_t)((t + 32768) >> 16);
        }
    }
}

// PIL's ImagingBlend on one band: float32, truncated, clipped where the factor extrapolates.
__device__ int aug_blend(int d, int p, float a)
{
    const float t = (float)d + a * (float)(p - d);
    return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// PIL's convert("L")
__device__ int aug_luma(const int *v) { return (v[0] * 19595 + v[1] * 38470 + v[2] * 7471 + 0x8000) >> 16; }

// torchvision's adjust_hue on one pixel: PIL's convert("HSV"), the 8-bit hue shifted modulo 256, PIL's convert("RGB").  The
// mix of float32 and binary64 is that of PIL's rgb2hsv_row / hsv2rgb; fmod(t, 1) of a positive t is t - floor(t), and every
// value that is rounded to an integer is >= 0, where C's round is floor(. + 0.5).
__device__ void aug_hue(int shift, int *v)
{
    const int r = v[0], g = v[1], b = v[2];
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        const double t = (double)h / 6.0 + 1.0;
        h = (float)(t - floor(t));
        uh = min(max((int)((double)h * 255.0), 0), 255), us = min(max((int)((double)s * 255.0), 0), 255);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        v[0] = v[1] = v[2] = maxc;
        return;
    }
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double vf = (double)(float)maxc;
    const int p = min(max((int)floor(vf * (1.0 - (double)fs) + 0.5), 0), 255);
    const int q = min(max((int)floor(vf * (1.0 - (double)(fs * f)) + 0.5), 0), 255);
    const int u = min(max((int)floor(vf * (1.0 - (double)fs * (1.0 - (double)f)) + 0.5), 0), 255);
    switch (i % 6) {
    case 0: v[0] = maxc, v[1] = u, v[2] = p; break;
    case 1: v[0] = q, v[1] = maxc, v[2] = p; break;
    case 2: v[0] = p, v[1] = maxc, v[2] = u; break;
    case 3: v[0] = p, v[1] = q, v[2] = maxc; break;
    case 4: v[0] = u, v[1] = p, v[2] = maxc; break;
    default: v[0] = maxc, v[1] = p, v[2] = q; break;
    }
}

// ImageEnhance.Brightness / Contrast / Color or the hue shift on one pixel; `grey` is the contrast's mean level.
__device__ void aug_enhance(int op, const AugJitter *j, int grey, int *v)
{
    if (op == 3) {
        aug_hue(j->hue, v);
        return;
    }
    const int d = op == 0 ? 0 : op == 1 ? grey : aug_luma(v);
    const float f = j->f[op];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = aug_blend(d, v[c], f);
}

// One lane per 4 pixels of a column, 64 lanes along a row: the operations in front of the contrast, then the integer sum of
// PIL's L over the image.  An image without a contrast step leaves at once.
__global__ __launch_bounds__(kBlock) void k_aug_luma_sum(const uint8_t *__restrict__ img, int h, int w, const AugJitter *__restrict__ prm,
                                                         unsigned long long *__restrict__ sums)
{
    const int b = blockIdx.z;
    const AugJitter *j = prm + b;                                             // (read in place: uniform loads, no private copy)
    int at = -1;
    for (int i = 3; i >= 0; --i) at = j->order[i] == 1 ? i : at;
    if (at < 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x;
    int sum = 0;
    for (int r = 0; r < 4; ++r) {
        const int y = (blockIdx.y * 4 + threadIdx.y) * 4 + r;
        if (x >= w || y >= h) continue;
        const uint8_t *p = img + (((size_t)b * h + y) * w + x) * 3;
        int v[3] = {p[0], p[1], p[2]};
        for (int i = 0; i < at; ++i)
            if (j->order[i] >= 0) aug_enhance(j->order[i], j, 0, v);
        sum += aug_luma(v);
    }
    sum = wave_sum(sum);
    if (threadIdx.x == 0 && sum) atomicAdd(&sums[b], (unsigned long long)sum);
}

// One lane per pixel, 64 along a row: the jitter in the drawn order (X:50-66), ToTensor and Normalize as numpy computes them
// (X:32, 43-46: float32 / 255, then each in-place step through binary64), planar stores.
__global__ __launch_bounds__(kBlock) void k_aug_finish(const uint8_t *__restrict__ img, int h, int w, const AugJitter *__restrict__ prm,
                                                       const unsigned long long *__restrict__ sums, AugNorm nm, float *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (x >= w || y >= h) return;
    const uint8_t *p = img + (((size_t)b * h + y) * w + x) * 3;
    int v[3] = {p[0], p[1], p[2]};
    if (prm) {
        const AugJitter *j = prm + b;
        const int grey = (int)((double)sums[b] / (double)((long long)h * w) + 0.5);
        for (int i = 0; i < 4; ++i)
            if (j->order[i] >= 0) aug_enhance(j->order[i], j, grey, v);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = (float)v[c] / 255.f;
        t = (float)((double)t - nm.mean[c]);
        t = (float)((double)t / nm.std[c]);
        out[(((size_t)b * 3 + c) * h + y) * w + x] = t;
    }
}

int aug_check(int B, int H, int W)
{
    if (B <= 0 || B > 65535) return fail(PVV_E_ARG, "augment: B must lie in [1, 65535]");
    if (H <= 0 || W <= 0 || H > kAugMaxSide || W > kAugMaxSide) return fail(PVV_E_ARG, "augment: the image's sides must lie in [1, 16384]");
    return PVV_OK;
}

}  // namespace

PVV_EXPORT size_t pvv_augment_workspace_bytes(int B, int max_th, int max_tw)
{
    if (aug_check(B, 1, 1)) return 0;
    if (max_th < 1 || max_tw < 1 || max_th > kAugMaxSide || max_tw > kAugMaxSide) {
        fail(PVV_E_ARG, "augment: max_th and max_tw must lie in [1, 16384]");
        return 0;
    }
    return align_up(sizeof(AugState) * (size_t)B) + align_up((size_t)B * max_th * max_tw * 3);
}

PVV_EXPORT int pvv_pvnet_augment(const uint8_t *d_img, const uint8_t *d_mask, const void *d_kpt_2d, int kpt_is_f64, int B, int H, int W,
                                 int K, int oh, int ow, double overlap_ratio, const void *d_params, int max_th, int max_tw, void *d_workspace,
                                 size_t workspace_bytes, uint8_t *d_out_img, uint8_t *d_out_mask, double *d_out_kpt, int32_t *d_path,
                                 int32_t *d_window, void *stream)
{
    if (int e = aug_check(B, H, W)) return e;
    if (oh < 8 || ow < 8 || oh > kAugMaxSide || ow > kAugMaxSide) return fail(PVV_E_ARG, "augment: out_size sides must lie in [8, 16384]");
    if (K < 0 || K > 65535) return fail(PVV_E_ARG, "augment: K must lie in [0, 65535]");
    if (!(overlap_ratio >= 0. && overlap_ratio <= 1.)) return fail(PVV_E_ARG, "augment: overlap_ratio must lie in [0, 1]");
    if (!d_img || !d_mask || !d_params || !d_workspace || !d_out_img || !d_out_mask || !d_path || !d_window || (K && (!d_kpt_2d || !d_out_kpt)))
        return fail(PVV_E_ARG, "augment: NULL device pointer");
    if ((uintptr_t)d_workspace % 8 != 0 || (uintptr_t)d_params % 8 != 0) return fail(PVV_E_ARG, "augment: workspace and params must be 8-byte aligned");
    if (max_th < 1 || max_tw < 1 || max_th > kAugMaxSide || max_tw > kAugMaxSide) return fail(PVV_E_ARG, "augment: max_th and max_tw must lie in [1, 16384]");
    if (workspace_bytes < pvv_augment_workspace_bytes(B, max_th, max_tw)) return fail(PVV_E_WORKSPACE, "augment: workspace smaller than pvv_augment_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    AugState *state = (AugState *)d_workspace;
    const AugDraw *dr = (const AugDraw *)d_params;
    if (hipMemsetAsync(state, 0, sizeof(AugState) * (size_t)B, st) != hipSuccess) return fail(PVV_E_ARG, "augment: hipMemsetAsync failed");
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(k_aug_moments, dim3((unsigned)((HW + 8 * kBlock - 1) / (8 * kBlock)), B), dim3(kBlock), 0, st, d_mask, H, W, state);
    if (int e = check_launch("k_aug_moments")) return e;
    hipLaunchKernelGGL(k_aug_box, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, st, d_mask, H, W, dr, state);
    if (int e = check_launch("k_aug_box")) return e;
    if (kpt_is_f64)
        hipLaunchKernelGGL(k_aug_window<double>, dim3(B), dim3(64), 0, st, state, dr, (const double *)d_kpt_2d, K, H, W, oh, ow, overlap_ratio,
                           d_out_kpt, d_path, d_window);
    else
        hipLaunchKernelGGL(k_aug_window<float>, dim3(B), dim3(64), 0, st, state, dr, (const float *)d_kpt_2d, K, H, W, oh, ow, overlap_ratio,
                           d_out_kpt, d_path, d_window);
    if (int e = check_launch("k_aug_window")) return e;
    uint8_t *win = (uint8_t *)d_workspace + align_up(sizeof(AugState) * (size_t)B);
    hipLaunchKernelGGL(k_aug_rotate, dim3((max_tw + 63) / 64, (max_th + 3) / 4, B), dim3(64, 4), 0, st, d_img, H, W, state, max_th, max_tw, win);
    if (int e = check_launch("k_aug_rotate")) return e;
    hipLaunchKernelGGL(k_aug_render, dim3((ow + 63) / 64, (oh + 3) / 4, B), dim3(64, 4), 0, st, d_img, d_mask, H, W, state, oh, ow, win, max_th,
                       max_tw, d_out_img, d_out_mask);
    return check_launch("k_aug_render");
}

PVV_EXPORT size_t pvv_transform_workspace_bytes(int B, int h, int w)
{
    if (aug_check(B, h, w)) return 0;
    return align_up(sizeof(unsigned long long) * (size_t)B) + align_up((size_t)B * h * w * 3);
}

PVV_EXPORT int pvv_pvnet_transform(const uint8_t *d_img, int B, int h, int w, const void *d_params, int has_blur, int has_contrast,
                                   const double *h_mean, const double *h_std, void *d_workspace, size_t workspace_bytes, float *d_out,
                                   void *stream)
{
    if (int e = aug_check(B, h, w)) return e;
    if (!d_img || !h_mean || !h_std || !d_out) return fail(PVV_E_ARG, "transform: NULL pointer");
    if (!d_params && (has_blur || has_contrast)) return fail(PVV_E_ARG, "transform: a blur or a contrast step needs params");
    if (d_params && (h < 8 || w < 8)) return fail(PVV_E_ARG, "transform: the image's sides must be at least 8 (the blur reflects 4 pixels)");
    if (d_params && (!d_workspace || (uintptr_t)d_workspace % 8 != 0 || (uintptr_t)d_params % 4 != 0))
        return fail(PVV_E_ARG, "transform: workspace must be 8-byte aligned, params 4-byte aligned");
    if (d_params && workspace_bytes < pvv_transform_workspace_bytes(B, h, w))
        return fail(PVV_E_WORKSPACE, "transform: workspace smaller than pvv_transform_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    const AugJitter *prm = (const AugJitter *)d_params;
    unsigned long long *sums = (unsigned long long *)d_workspace;
    const uint8_t *src = d_img;
    if (prm && has_blur) {
        uint8_t *blurred = (uint8_t *)d_workspace + align_up(sizeof(unsigned long long) * (size_t)B);
        hipLaunchKernelGGL(k_aug_blur, dim3((w + 63) / 64, (h + kBlurTile - 1) / kBlurTile, B), dim3(64, 4), 0, st, d_img, h, w, prm, blurred);
        if (int e = check_launch("k_aug_blur")) return e;
        src = blurred;
    }
    if (prm) {
        if (hipMemsetAsync(sums, 0, sizeof(unsigned long long) * (size_t)B, st) != hipSuccess) return fail(PVV_E_ARG, "transform: hipMemsetAsync failed");
        if (has_contrast) {
            hipLaunchKernelGGL(k_aug_luma_sum, dim3((w + 63) / 64, (h + 15) / 16, B), dim3(64, 4), 0, st, src, h, w, prm, sums);
            if (int e = check_launch("k_aug_luma_sum")) return e;
        }
    }
    AugNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = h_mean[c], nm.std[c] = h_std[c];
    hipLaunchKernelGGL(k_aug_finish, dim3((w + 63) / 64, (h + 3) / 4, B), dim3(64, 4), 0, st, src, h, w, prm, sums, nm, d_out);
    return check_launch("k_aug_finish");
}
