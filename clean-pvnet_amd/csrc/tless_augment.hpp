// tless_augment.hpp -- the T-LESS PVNet loader's training sample from rotated cut-outs and a background, and its crop around the
// target (include/pvnet_vote.h, "T-LESS PVNet augmentation").  Part of pvnet_vote.hip: built with -ffp-contract=off, every float
// and double operation below rounds once, in the order written, so that the numpy twin (tests/tless_augment_twin.py) gives the
// same bits.  The two fixed-point warp rules, the box accumulator, the placement record with its coverage test, the crop's map
// and the rectangle of magnify_box are those of warp.hpp, the wave reductions and the block tree those
// of vote_common.hpp; the colour step is the detector's: CtaParam, the grey level, the mean and the colour kernels are those
// of ct_augment.hpp.  No random numbers and no transcendental function are evaluated here: the host hands over the rotation
// matrices with their inverses and bounds, the drawn factors and the colour records.  Everything is a gather: a pixel has one
// owner, and the only atomics are integer ones on per-sample accumulators.
//
// Reference behaviour restated:
//   T = lib/utils/tless/tless_train_utils.py (cut_and_paste :94-120, get_fused_image :123-136, rotate_image :153-172)
//   U = lib/utils/tless/tless_utils.py:86-97 (cut_and_paste)
//   D = lib/datasets/tless_train/pvnet.py (read_data :60-69, get_training_img :73-105, __getitem__ :113-116)
//   V = lib/utils/tless/tless_pvnet_utils.py (magnify_box :13-18, augment :21-73)
#pragma once

#include "ct_augment.hpp"
#include "warp.hpp"

namespace {

constexpr int kTlaMaxN = PVV_TLESS_MAX_N;
constexpr int kTlaMaxSide = 16384;

struct TlaCut {                   // PVV_TLESS_CUT_BYTES per cut-out, built by the host from the draws
    double M[6], inv[6];          // cut-out -> rotated cut-out (T:157-165), and its inverse
    int32_t bh, bw, pad_[2];      // bound_h, bound_w (T:161-162)
};
static_assert(sizeof(TlaCut) == PVV_TLESS_CUT_BYTES, "pvnet_vote.h promises this size");

struct TlaStat {                  // per cut-out, in the workspace; zeroed before the first launch
    Extent box;                   // the rotated mask's box
    unsigned long long sum;       // the sum of the rotated mask's values (D:74)
};

struct TlaPrep {                  // per sample, in the workspace
    double inv[6];                // input image -> canvas
    int32_t rx0, ry0, rx1, ry1;   // the rectangle magnify_box keeps, inclusive
};

// The rotated mask of G cut-outs per sample, one lane per pixel of the D x D plane, 64 along a row; grid (tiles, G, B).  Plane
// (b, g) reads record cut[b * stride + first + g].  Outside bound_w x bound_h the plane is zero.  With stat: the box of != 0 and
// the sum of the values by wave shuffles, then integer atomics per cut-out.  Cut-outs g >= num[b] are left alone.
__global__ __launch_bounds__(kBlock) void k_tla_rotate_mask(const uint8_t *__restrict__ mask, const TlaCut *__restrict__ cut,
                                                            const int32_t *__restrict__ num, int G, int first, int stride, int h, int w,
                                                            int D, int tiles_x, int nearest, uint8_t *__restrict__ rot,
                                                            TlaStat *__restrict__ stat)
{
    const int x = (blockIdx.x % tiles_x) * 64 + threadIdx.x, y = (blockIdx.x / tiles_x) * 4 + threadIdx.y, g = blockIdx.y, b = blockIdx.z;
    if (num && g >= num[b]) return;
    const size_t r = (size_t)b * stride + first + g, p = (size_t)b * G + g;
    const TlaCut *c = cut + r;
    int v = 0;
    if (x < D && y < D) {
        if (x < c->bw && y < c->bh) {
            if (nearest) sample_nearest<1>(mask + p * h * w, h, w, c->inv, x, y, &v);
            else sample_linear<1>(mask + p * h * w, h, w, c->inv, x, y, &v);
        }
        rot[(p * D + y) * D + x] = (uint8_t)v;
    }
    if (!stat) return;
    const bool hit = v != 0;
    if (__ballot(hit) == 0) return;                                         // the same for the wave's lanes
    stat[r].box.note(hit, x, y);
    const int sum = wave_sum(v);
    if (threadIdx.x == 0) atomicAdd(&stat[r].sum, (unsigned long long)sum);
}

// The rotated image of P cut-outs [P,h,w,3] -> [P,D,D,3], zero outside the bound; grid (tiles, 1, P).
__global__ __launch_bounds__(kBlock) void k_tla_rotate_img(const uint8_t *__restrict__ img, const TlaCut *__restrict__ cut, int h, int w, int D,
                                                           int tiles_x, int nearest, uint8_t *__restrict__ rot)
{
    const int x = (blockIdx.x % tiles_x) * 64 + threadIdx.x, y = (blockIdx.x / tiles_x) * 4 + threadIdx.y;
    const size_t p = blockIdx.z;
    if (x >= D || y >= D) return;
    const TlaCut *c = cut + p;
    int v[3] = {0, 0, 0};
    if (x < c->bw && y < c->bh) {
        if (nearest) sample_nearest<3>(img + p * h * w * 3, h, w, c->inv, x, y, v);
        else sample_linear<3>(img + p * h * w * 3, h, w, c->inv, x, y, v);
    }
    uint8_t *o = rot + ((p * D + y) * D + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (uint8_t)v[k];
}

// One block per sample: the placements of the 1 + N cut-outs (U:87-93), and the keypoints through the target's matrix (D:66) and its
// shift (D:80-82).
__global__ __launch_bounds__(64) void k_tla_place(const TlaStat *__restrict__ stat, const TlaCut *__restrict__ cut, const double *__restrict__ u,
                                                  const double *__restrict__ kpt, int K, int N, int H, int W, int32_t *__restrict__ place,
                                                  double *__restrict__ out_kpt)
{
    const size_t r0 = (size_t)blockIdx.x * (1 + N);
    for (int j = threadIdx.x; j <= N; j += 64) {
        int32_t rec[6];
        place_record(stat[r0 + j].box, H, W, u[2 * (r0 + j)], u[2 * (r0 + j) + 1], rec);
        for (int i = 0; i < 6; ++i) place[6 * (r0 + j) + i] = rec[i];
    }
    int32_t t[6];
    place_record(stat[r0].box, H, W, u[2 * r0], u[2 * r0 + 1], t);
    const double *M = cut[r0].M;
    for (int k = threadIdx.x; k < K; k += 64) {
        const size_t i = (size_t)blockIdx.x * K + k;
        const double x = kpt[2 * i], y = kpt[2 * i + 1];
        const double rx = (M[0] * x + M[1] * y) + M[2], ry = (M[3] * x + M[4] * y) + M[5];
        out_kpt[2 * i] = (rx - (double)t[1]) + (double)t[5];
        out_kpt[2 * i + 1] = (ry - (double)t[0]) + (double)t[4];
    }
}

// One lane per canvas pixel, 64 along a row: the coverage byte (bit 7: the target; the low bits: the last distractor over the
// pixel, plus one) and visible[b], the target's pixels that no distractor covers (D:96-97).
__global__ __launch_bounds__(kBlock) void k_tla_cover(const uint8_t *__restrict__ rot_t, int Dt, const uint8_t *__restrict__ rot_o, int Do,
                                                      const int32_t *__restrict__ place, const int32_t *__restrict__ num, int N, int H, int W,
                                                      uint8_t *__restrict__ cover, unsigned long long *__restrict__ visible)
{
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    bool t = false;
    int owner = 0;
    if (X < W && Y < H) {
        const size_t r0 = (size_t)b * (1 + N);
        t = place_covers(place + 6 * r0, rot_t + (size_t)b * Dt * Dt, Dt, Dt, X, Y) != nullptr;
        const int cnt = num ? min(max(num[b], 0), N) : N;
        for (int n = cnt - 1; n >= 0; --n)
            if (place_covers(place + 6 * (r0 + 1 + n), rot_o + ((size_t)b * N + n) * Do * Do, Do, Do, X, Y)) {
                owner = n + 1;
                break;
            }
        cover[((size_t)b * H + Y) * W + X] = (uint8_t)((t ? 128 : 0) | owner);
    }
    const unsigned long long m = __ballot(t && owner == 0);
    if (threadIdx.x == 0 && m) atomicAdd(&visible[b], (unsigned long long)__popcll(m));
}

// D:93-100: 0 on top by draw, 1 occluded and kept, 2 occluded below the ratio and put on top, 3 no target.
__device__ int tla_path(const TlaStat *target, unsigned long long visible, int top, double ratio)
{
    if (target->box.empty()) return 3;
    if (top) return 0;
    return (double)visible / (double)target->sum < ratio ? 2 : 1;
}

// One lane per canvas pixel: the branch, the owner's colour sampled through its inverse rotation, the mask, the mask's box.
__global__ __launch_bounds__(kBlock) void k_tla_resolve(const uint8_t *__restrict__ bg, const uint8_t *__restrict__ fused_bg,
                                                        const uint8_t *__restrict__ img_t, int ht, int wt, const uint8_t *__restrict__ img_o,
                                                        int ho, int wo, const TlaCut *__restrict__ cut, const int32_t *__restrict__ place,
                                                        const TlaStat *__restrict__ stat, const unsigned long long *__restrict__ visible,
                                                        const int32_t *__restrict__ flags, const uint8_t *__restrict__ cover, int N, int H, int W,
                                                        int nearest, double ratio, uint8_t *__restrict__ out_img, uint8_t *__restrict__ out_mask,
                                                        Extent *__restrict__ box)
{
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    bool m = false;
    if (X < W && Y < H) {
        const size_t r0 = (size_t)b * (1 + N), o = ((size_t)b * H + Y) * W + X;
        const int path = tla_path(stat + r0, visible[b], flags[2 * b], ratio);
        const int cv = cover[o], owner = cv & 127;
        const bool t = (cv & 128) != 0, top = path != 1;
        const int j = top ? (t ? 0 : owner ? owner : -1) : (owner ? owner : t ? 0 : -1);       // the cut-out that owns the pixel
        m = top ? t : (t && !owner);
        int v[3] = {0, 0, 0};
        if (j < 0) {
            const uint8_t *s = top ? (flags[2 * b + 1] ? nullptr : fused_bg) : bg;
            if (s)
                for (int c = 0; c < 3; ++c) v[c] = s[o * 3 + c];
        } else {
            const int32_t *p = place + 6 * (r0 + j);
            const int x = X - p[5] + p[1], y = Y - p[4] + p[0];
            auto sample = [&](const uint8_t *src, int h, int w) {                      // (the sides stay uniform in either branch)
                if (nearest) sample_nearest<3>(src, h, w, cut[r0 + j].inv, x, y, v);
                else sample_linear<3>(src, h, w, cut[r0 + j].inv, x, y, v);
            };
            if (j == 0) sample(img_t + (size_t)b * ht * wt * 3, ht, wt);
            else sample(img_o + ((size_t)b * N + j - 1) * ho * wo * 3, ho, wo);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out_img[o * 3 + c] = (uint8_t)v[c];
        out_mask[o] = m ? 1 : 0;
    }
    if (__ballot(m) == 0) return;
    box[b].note(m, X, Y);
}

// One lane per sample: D:102-103 as (x, y, x + w - 1, y + h - 1), the whole canvas for an empty mask; the branch; (visible, pixel_num).
__global__ __launch_bounds__(kBlock) void k_tla_finish(const Extent *__restrict__ box, const TlaStat *__restrict__ stat,
                                                       const unsigned long long *__restrict__ visible, const int32_t *__restrict__ flags, int B, int N,
                                                       int H, int W, double ratio, int32_t *__restrict__ bbox, int32_t *__restrict__ path,
                                                       long long *__restrict__ vis)
{
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    int32_t *o = bbox + 4 * (size_t)b;
    if (box[b].empty()) o[0] = 0, o[1] = 0, o[2] = W - 1, o[3] = H - 1;
    else box[b].decode(o);
    const TlaStat *t = stat + (size_t)b * (1 + N);
    path[b] = tla_path(t, visible[b], flags[2 * b], ratio);
    vis[2 * b] = (long long)visible[b], vis[2 * b + 1] = (long long)t->sum;
}

// One block per sample: scale (float32), centre (binary64) (V:25-33), the crop's map, its inverse, the rectangle of magnify_box
// (V:13-18, 52-55) and the keypoints (D:115).
__global__ __launch_bounds__(64) void k_tla_prep(const int32_t *__restrict__ bbox, const float *__restrict__ factor,
                                                 const double *__restrict__ box_ratio, const double *__restrict__ kpt, int K, int iw, int ih,
                                                 double *__restrict__ center, float *__restrict__ scale, double *__restrict__ trans,
                                                 int32_t *__restrict__ box, double *__restrict__ out_kpt, TlaPrep *__restrict__ prm)
{
    const int b = blockIdx.x;
    const int x0 = bbox[4 * b], y0 = bbox[4 * b + 1], x1 = bbox[4 * b + 2], y1 = bbox[4 * b + 3];
    const long long bw = (long long)x1 - x0 + 1, bh = (long long)y1 - y0 + 1;
    const float s = (float)(bw > bh ? bw : bh) * factor[b];
    const double cx = (double)((long long)x0 + x1) / 2., cy = (double)((long long)y0 + y1) / 2.;
    double M[6] = {0., 0., 0., 0., 0., 0.}, I[6];
    int32_t r[4] = {0, 0, 0, 0};
    if (s > 0.f && isfinite(s)) {
        crop_transform(cx, cy, (double)s, iw, ih, M);
        magnify_rect(M, (double)x0, (double)y0, (double)x1, (double)y1, box_ratio[b], iw, ih, r);
    }
    invert_affine(M, I);
    if (threadIdx.x == 0) {
        TlaPrep p;
        for (int i = 0; i < 6; ++i) p.inv[i] = I[i], trans[6 * (size_t)b + i] = M[i];
        p.rx0 = r[0], p.ry0 = r[1], p.rx1 = r[2], p.ry1 = r[3];
        prm[b] = p;
        box[4 * b] = p.rx0, box[4 * b + 1] = p.ry0, box[4 * b + 2] = p.rx1, box[4 * b + 3] = p.ry1;
        center[2 * b] = cx, center[2 * b + 1] = cy, scale[2 * b] = s, scale[2 * b + 1] = s;
    }
    for (int k = threadIdx.x; k < K; k += 64) {
        const size_t i = (size_t)b * K + k;
        const double x = kpt[2 * i], y = kpt[2 * i + 1];
        out_kpt[2 * i] = (M[0] * x + M[1] * y) + M[2];
        out_kpt[2 * i + 1] = (M[3] * x + M[4] * y) + M[5];
    }
}

// One lane per pixel of the input image, 64 along a row (V:49-58, D:116): the 8-bit bilinear warp inside the kept rectangle and
// zero outside it, the nearest warp of the mask, and the tile's binary64 sum of the grey level to part[b][tile] as k_cta_warp.
__global__ __launch_bounds__(kBlock) void k_tla_warp(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask, int H, int W,
                                                     const TlaPrep *__restrict__ prm, int ih, int iw, uint8_t *__restrict__ orig,
                                                     uint8_t *__restrict__ out_mask, double *__restrict__ part)
{
    __shared__ double s_sum[kBlock];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    double g = 0.;
    if (x < iw && y < ih) {
        const TlaPrep *p = prm + b;
        int v[3] = {0, 0, 0};
        if (x >= p->rx0 && x <= p->rx1 && y >= p->ry0 && y <= p->ry1)
            sample_linear<3>(img + (size_t)b * H * W * 3, H, W, p->inv, x, y, v);
        int mv;
        sample_nearest<1>(mask + (size_t)b * H * W, H, W, p->inv, x, y, &mv);
        const size_t o = ((size_t)b * ih + y) * iw + x;
        float f[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) orig[o * 3 + c] = (uint8_t)v[c], f[c] = (float)v[c] / 255.f;
        out_mask[o] = (uint8_t)mv;
        g = (double)cta_grey(f);
    }
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const double sum = block_tree_sum(g, s_sum, tid);
    if (tid == 0) part[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

int tla_sides(int B, int H, int W, const char *what)
{
    if (B <= 0 || B > 65535) return fail(PVV_E_ARG, "tless_augment: B must lie in [1, 65535]");
    if (H <= 0 || W <= 0 || H > kTlaMaxSide || W > kTlaMaxSide) return fail(PVV_E_ARG, what);
    return PVV_OK;
}

// floor(sqrt(h^2 + w^2)): no bound_h or bound_w of T:161-162 exceeds it
int tla_diag(int h, int w)
{
    const long long n = (long long)h * h + (long long)w * w;
    long long d = (long long)sqrt((double)n);
    while (d * d > n) --d;
    while ((d + 1) * (d + 1) <= n) ++d;
    return (int)d;
}

struct TlaLayout { size_t stat, visible, box, cover, rot_t, rot_o, total; };

TlaLayout tla_layout(int B, int N, int H, int W, int Dt, int Do)
{
    TlaLayout L;
    L.stat = 0;                                                             // stat, visible and box are zeroed by one fill
    L.visible = L.stat + align_up(sizeof(TlaStat) * (size_t)B * (1 + N));
    L.box = L.visible + align_up(sizeof(unsigned long long) * (size_t)B);
    L.cover = L.box + align_up(sizeof(Extent) * (size_t)B);
    L.rot_t = L.cover + align_up((size_t)B * H * W);
    L.rot_o = L.rot_t + align_up((size_t)B * Dt * Dt);
    L.total = L.rot_o + align_up((size_t)B * N * Do * Do);
    return L;
}

struct TlaAugLayout { size_t prep, part, mean, total; int tx, ty; };

TlaAugLayout tla_aug_layout(int B, int ih, int iw)
{
    TlaAugLayout L;
    L.tx = (iw + 63) / 64, L.ty = (ih + 3) / 4;
    L.prep = 0;
    L.part = align_up(sizeof(TlaPrep) * (size_t)B);
    L.mean = L.part + align_up(sizeof(double) * (size_t)B * L.tx * L.ty);
    L.total = L.mean + align_up(sizeof(float) * (size_t)B);
    return L;
}

}  // namespace

PVV_EXPORT int pvv_tless_rotate_side(int h, int w)
{
    if (h <= 0 || w <= 0 || h > kTlaMaxSide || w > kTlaMaxSide) return 0;
    return tla_diag(h, w);
}

PVV_EXPORT int pvv_tless_rotate(const uint8_t *d_src, const void *d_cuts, int P, int h, int w, int channels, int D, int nearest,
                                uint8_t *d_out, void *stream)
{
    if (int e = tla_sides(P, h, w, "tless_rotate: the cut-outs' sides must lie in [1, 16384]")) return e;
    if (channels != 1 && channels != 3) return fail(PVV_E_ARG, "tless_rotate: channels must be 1 or 3");
    if (D != tla_diag(h, w)) return fail(PVV_E_ARG, "tless_rotate: D must be pvv_tless_rotate_side(h, w)");
    if (!d_src || !d_cuts || !d_out) return fail(PVV_E_ARG, "tless_rotate: NULL device pointer");
    if ((uintptr_t)d_cuts % 8 != 0) return fail(PVV_E_ARG, "tless_rotate: the records must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int tx = (D + 63) / 64, ty = (D + 3) / 4;
    const TlaCut *cut = (const TlaCut *)d_cuts;
    if (channels == 1) {
        hipLaunchKernelGGL(k_tla_rotate_mask, dim3(tx * ty, 1, P), dim3(64, 4), 0, st, d_src, cut, (const int32_t *)nullptr, 1, 0, 1, h, w, D, tx,
                           nearest != 0, d_out, (TlaStat *)nullptr);
        return check_launch("k_tla_rotate_mask");
    }
    hipLaunchKernelGGL(k_tla_rotate_img, dim3(tx * ty, 1, P), dim3(64, 4), 0, st, d_src, cut, h, w, D, tx, nearest != 0, d_out);
    return check_launch("k_tla_rotate_img");
}

PVV_EXPORT size_t pvv_tless_compose_workspace_bytes(int B, int N, int H, int W, int ht, int wt, int ho, int wo)
{
    if (tla_sides(B, H, W, "tless_compose: the canvas' sides must lie in [1, 16384]")) return 0;
    if (tla_sides(B, ht, wt, "tless_compose: the target's sides must lie in [1, 16384]")) return 0;
    if (N < 0 || N > kTlaMaxN) {
        fail(PVV_E_ARG, "tless_compose: N must lie in [0, 16]");
        return 0;
    }
    if (N > 0 && tla_sides(B, ho, wo, "tless_compose: the distractors' sides must lie in [1, 16384]")) return 0;
    return tla_layout(B, N, H, W, tla_diag(ht, wt), N ? tla_diag(ho, wo) : 0).total;
}

PVV_EXPORT int pvv_tless_compose(const uint8_t *d_bg, const uint8_t *d_fused_bg, const uint8_t *d_img, const uint8_t *d_mask,
                                 const double *d_kpt, const uint8_t *d_other_img, const uint8_t *d_other_mask, const int32_t *d_num,
                                 const void *d_cuts, const double *d_place_u, const int32_t *d_flags, int B, int H, int W, int N, int K,
                                 int ht, int wt, int ho, int wo, int nearest, double ratio, void *d_workspace, size_t workspace_bytes,
                                 uint8_t *d_out_img, uint8_t *d_out_mask, double *d_out_kpt, int32_t *d_bbox, int32_t *d_path,
                                 int32_t *d_place, long long *d_visible, void *stream)
{
    if (int e = tla_sides(B, H, W, "tless_compose: the canvas' sides must lie in [1, 16384]")) return e;
    if (int e = tla_sides(B, ht, wt, "tless_compose: the target's sides must lie in [1, 16384]")) return e;
    if (N < 0 || N > kTlaMaxN) return fail(PVV_E_ARG, "tless_compose: N must lie in [0, 16]");
    if (N > 0)
        if (int e = tla_sides(B, ho, wo, "tless_compose: the distractors' sides must lie in [1, 16384]")) return e;
    if (K < 0 || K > 65535) return fail(PVV_E_ARG, "tless_compose: K must lie in [0, 65535]");
    if (!(ratio > 0.)) return fail(PVV_E_ARG, "tless_compose: ratio must be > 0");
    if (!d_bg || !d_img || !d_mask || (K && (!d_kpt || !d_out_kpt)) || (N && (!d_other_img || !d_other_mask)) || !d_cuts || !d_place_u || !d_flags ||
        !d_workspace || !d_out_img || !d_out_mask || !d_bbox || !d_path || !d_place || !d_visible)
        return fail(PVV_E_ARG, "tless_compose: NULL device pointer");
    if ((uintptr_t)d_cuts % 8 != 0 || (uintptr_t)d_place_u % 8 != 0 || (uintptr_t)d_kpt % 8 != 0 || (uintptr_t)d_out_kpt % 8 != 0 ||
        (uintptr_t)d_visible % 8 != 0 || (uintptr_t)d_workspace % 8 != 0 || (uintptr_t)d_flags % 4 != 0 || (uintptr_t)d_num % 4 != 0 ||
        (uintptr_t)d_bbox % 4 != 0 || (uintptr_t)d_path % 4 != 0 || (uintptr_t)d_place % 4 != 0)
        return fail(PVV_E_ARG, "tless_compose: records, uniforms, keypoints, visible and workspace must be 8-byte aligned, the int32 arrays 4-byte aligned");
    const int Dt = tla_diag(ht, wt), Do = N ? tla_diag(ho, wo) : 0;
    const TlaLayout L = tla_layout(B, N, H, W, Dt, Do);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "tless_compose: workspace smaller than pvv_tless_compose_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)d_workspace;
    TlaStat *stat = (TlaStat *)(ws + L.stat);
    unsigned long long *visible = (unsigned long long *)(ws + L.visible);
    Extent *box = (Extent *)(ws + L.box);
    uint8_t *cover = ws + L.cover, *rot_t = ws + L.rot_t, *rot_o = ws + L.rot_o;
    const TlaCut *cut = (const TlaCut *)d_cuts;
    if (hipMemsetAsync(ws, 0, L.cover, st) != hipSuccess) return fail(PVV_E_ARG, "tless_compose: hipMemsetAsync failed");
    const dim3 block(64, 4);
    int tx = (Dt + 63) / 64, ty = (Dt + 3) / 4;
    hipLaunchKernelGGL(k_tla_rotate_mask, dim3(tx * ty, 1, B), block, 0, st, d_mask, cut, (const int32_t *)nullptr, 1, 0, 1 + N, ht, wt, Dt, tx,
                       nearest != 0, rot_t, stat);
    if (int e = check_launch("k_tla_rotate_mask")) return e;
    if (N) {
        tx = (Do + 63) / 64, ty = (Do + 3) / 4;
        hipLaunchKernelGGL(k_tla_rotate_mask, dim3(tx * ty, N, B), block, 0, st, d_other_mask, cut, d_num, N, 1, 1 + N, ho, wo, Do, tx, nearest != 0,
                           rot_o, stat);
        if (int e = check_launch("k_tla_rotate_mask")) return e;
    }
    hipLaunchKernelGGL(k_tla_place, dim3(B), dim3(64), 0, st, stat, cut, d_place_u, d_kpt, K, N, H, W, d_place, d_out_kpt);
    if (int e = check_launch("k_tla_place")) return e;
    const dim3 grid((W + 63) / 64, (H + 3) / 4, B);
    hipLaunchKernelGGL(k_tla_cover, grid, block, 0, st, rot_t, Dt, rot_o, Do, d_place, d_num, N, H, W, cover, visible);
    if (int e = check_launch("k_tla_cover")) return e;
    hipLaunchKernelGGL(k_tla_resolve, grid, block, 0, st, d_bg, d_fused_bg ? d_fused_bg : d_bg, d_img, ht, wt, d_other_img, ho, wo, cut, d_place,
                       stat, visible, d_flags, cover, N, H, W, nearest != 0, ratio, d_out_img, d_out_mask, box);
    if (int e = check_launch("k_tla_resolve")) return e;
    hipLaunchKernelGGL(k_tla_finish, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, st, box, stat, visible, d_flags, B, N, H, W, ratio, d_bbox,
                       d_path, d_visible);
    return check_launch("k_tla_finish");
}

PVV_EXPORT size_t pvv_tless_augment_workspace_bytes(int B, int ih, int iw)
{
    if (tla_sides(B, ih, iw, "tless_augment: the input's sides must lie in [1, 16384]")) return 0;
    return tla_aug_layout(B, ih, iw).total;
}

PVV_EXPORT int pvv_tless_augment(const uint8_t *d_img, const uint8_t *d_mask, const double *d_kpt, const int32_t *d_bbox, int B, int H, int W,
                                 int K, int ih, int iw, int train, const float *d_factor, const double *d_box_ratio, const void *d_colour,
                                 const float *h_mean, const float *h_std, void *d_workspace, size_t workspace_bytes, uint8_t *d_orig,
                                 float *d_inp, uint8_t *d_out_mask, double *d_out_kpt, double *d_trans, double *d_center, float *d_scale,
                                 int32_t *d_box, void *stream)
{
    if (int e = tla_sides(B, H, W, "tless_augment: the image's sides must lie in [1, 16384]")) return e;
    if (int e = tla_sides(B, ih, iw, "tless_augment: the input's sides must lie in [1, 16384]")) return e;
    if (K < 0 || K > 65535) return fail(PVV_E_ARG, "tless_augment: K must lie in [0, 65535]");
    if (!d_img || !d_mask || (K && (!d_kpt || !d_out_kpt)) || !d_bbox || !d_factor || !d_box_ratio || (train && !d_colour) || !h_mean || !h_std ||
        !d_workspace || !d_orig || !d_inp || !d_out_mask || !d_trans || !d_center || !d_scale || !d_box)
        return fail(PVV_E_ARG, "tless_augment: NULL pointer");
    if ((uintptr_t)d_workspace % 8 != 0 || (uintptr_t)d_colour % 8 != 0 || (uintptr_t)d_kpt % 8 != 0 || (uintptr_t)d_out_kpt % 8 != 0 ||
        (uintptr_t)d_box_ratio % 8 != 0 || (uintptr_t)d_trans % 8 != 0 || (uintptr_t)d_center % 8 != 0 || (uintptr_t)d_factor % 4 != 0 ||
        (uintptr_t)d_bbox % 4 != 0 || (uintptr_t)d_inp % 4 != 0 || (uintptr_t)d_scale % 4 != 0 || (uintptr_t)d_box % 4 != 0)
        return fail(PVV_E_ARG, "tless_augment: binary64 arrays, records and workspace must be 8-byte aligned, 32-bit arrays 4-byte aligned");
    const TlaAugLayout L = tla_aug_layout(B, ih, iw);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "tless_augment: workspace smaller than pvv_tless_augment_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)d_workspace;
    TlaPrep *prep = (TlaPrep *)(ws + L.prep);
    double *part = (double *)(ws + L.part);
    float *gs_mean = (float *)(ws + L.mean);
    hipLaunchKernelGGL(k_tla_prep, dim3(B), dim3(64), 0, st, d_bbox, d_factor, d_box_ratio, d_kpt, K, iw, ih, d_center, d_scale, d_trans, d_box,
                       d_out_kpt, prep);
    if (int e = check_launch("k_tla_prep")) return e;
    const dim3 grid(L.tx, L.ty, B), block(64, 4);
    hipLaunchKernelGGL(k_tla_warp, grid, block, 0, st, d_img, d_mask, H, W, prep, ih, iw, d_orig, d_out_mask, part);
    if (int e = check_launch("k_tla_warp")) return e;
    const CtaParam *colour = train ? (const CtaParam *)d_colour : nullptr;
    if (colour) {
        hipLaunchKernelGGL(k_cta_mean, dim3(B), dim3(kBlock), 0, st, part, L.tx * L.ty, (long long)ih * iw, gs_mean);
        if (int e = check_launch("k_cta_mean")) return e;
    }
    CtaNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = h_mean[c], nm.std[c] = h_std[c];
    if (iw % 4 == 0 && (uintptr_t)d_orig % 4 == 0 && (uintptr_t)d_inp % 16 == 0)
        hipLaunchKernelGGL(k_cta_colour<true>, dim3((iw / 4 + 63) / 64, L.ty, B), block, 0, st, d_orig, ih, iw, colour, gs_mean, nm, d_inp);
    else
        hipLaunchKernelGGL(k_cta_colour<false>, grid, block, 0, st, d_orig, ih, iw, colour, gs_mean, nm, d_inp);
    return check_launch("k_cta_colour");
}
