// ct_train.hpp -- the detector's heat-map targets and training loss (include/pvnet_vote.h, "Detector training: heat-map
// targets and the detector loss").  Included at the end of pvnet_vote.hip after train.hpp, whose tile constants, block sum and
// 16-byte accessors it shares, and on the host side its workspace layout (loss_layout), workspace check (train_ws) and out_state
// check (loss_state); CTT_LAUNCH picks a kernel's 16-byte or scalar form.  Built with -ffp-contract=off, so every operation
// below rounds once, in the order written.
// The numpy twin (tests/ct_train_twin.py) follows the same order.
//
// Reference behaviour restated (paths relative to the reference's root):
//   P = lib/datasets/tless_train/ct.py:46-66 (prepare_detection)     G = lib/utils/data_utils.py:10-65 (radius and Gaussian)
//   K = lib/datasets/collate_batch.py:6-32 (ct_collator)             T = lib/train/trainers/ct.py:14-31 (the loss)
//   L = lib/utils/net_utils.py:9-49, 195-246 (sigmoid, _neg_loss, IndL1Loss1d)
//
// Streaming kernels: a lane owns kTrainLanePix consecutive elements of an image's flattened [C*H*W] map, read and written with
// 16-byte accesses when the size and the bases allow it (VEC); the scalar form has the same arithmetic.  Every sum is binary64
// in the order lane, tile, image slots, batch; per-tile partials go to the workspace and two small launches finish them.  No
// float atomics: a maximum needs no order (the heat map is gathered per element from the image's object list in LDS), and the
// wh gradient has one owner per (image, index).
#pragma once

namespace {

constexpr int kCttMaxN = PVV_CT_TRAIN_MAX_N;

struct CttShape {
    int B, N, C, H, W, HW, E, tiles;                  // E = C*H*W elements of an image, tiles of kTrainTile elements
    long long hp_stride, wp_stride, hm_stride;        // elements between two images of hm_pred / wh_pred / ct_hm
};

// Workspace: per (image, tile) {P, Q} binary64 and num_pos int64, then per image {P, Q, S, M} binary64 and {num_pos, bad} int64.
LossLayout ctt_layout(int B, int tiles) { return loss_layout(B, tiles, 2, 1, 4, 2); }

__device__ __forceinline__ double ctt_box_at(const void *__restrict__ boxes, int kind, size_t e)
{
    return kind == PVV_BOX_F32 ? (double)((const float *)boxes)[e]
         : kind == PVV_BOX_I32 ? (double)((const int *)boxes)[e]
                               : (double)((const long long *)boxes)[e];
}

__device__ __forceinline__ long long ctt_int_at(const void *__restrict__ p, int is_i64, size_t e)
{
    return is_i64 ? ((const long long *)p)[e] : (long long)((const int *)p)[e];
}

// G:10-33 with min_overlap = 0.7 for integral height and width, step by step: only + - * / sqrt, so the same bits anywhere.
__device__ __forceinline__ double ctt_gaussian_radius(double height, double width)
{
    const double mo = 0.7;
    const double s = height + width;
    const double c1 = ((width * height) * (1.0 - mo)) / (1.0 + mo);
    const double r1 = (s + sqrt(s * s - 4.0 * c1)) / 2.0;
    const double b2 = 2.0 * s;
    const double c2 = ((1.0 - mo) * width) * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 16.0 * c2)) / 2.0;
    const double a3 = 4.0 * mo;
    const double b3 = (-2.0 * mo) * s;
    const double c3 = ((mo - 1.0) * width) * height;
    const double d3 = b3 * b3 - (4.0 * a3) * c3;
    const double r12 = r2 < r1 ? r2 : r1;
    double r3 = r12;                                  // G:28-29
    if (!(d3 < 0.0)) r3 = (b3 + sqrt(d3)) / 2.0;
    return r3 < r12 ? r3 : r12;
}

// What P:46-66 makes of one object; keep == 0: dropped (it draws nothing and takes no row).
struct CttObject {
    int keep, cx, cy, r, cls;
    float w, h;
};

__device__ __forceinline__ CttObject ctt_object(const void *__restrict__ boxes, int box_kind, const void *__restrict__ cls, int cls_is_i64,
                                              size_t o, int C, int H, int W)
{
    CttObject q = {0, 0, 0, 0, -1, 0.f, 0.f};
    const double x0 = ctt_box_at(boxes, box_kind, 4 * o), y0 = ctt_box_at(boxes, box_kind, 4 * o + 1);
    const double x1 = ctt_box_at(boxes, box_kind, 4 * o + 2), y1 = ctt_box_at(boxes, box_kind, 4 * o + 3);
    const double lim = 16777216.0;
    if (!(fabs(x0) < lim && fabs(y0) < lim && fabs(x1) < lim && fabs(y1) < lim)) return q;   // a NaN fails every comparison
    const double w = x1 - x0, h = y1 - y0;
    if (!(w > 0.0 && h > 0.0)) return q;
    const long long c = ctt_int_at(cls, cls_is_i64, o);
    if (c < 0 || c >= C) return q;
    const int cx = (int)rintf((float)((x0 + x1) / 2.0)), cy = (int)rintf((float)((y0 + y1) / 2.0));   // P:51-52: half to even
    if (cx < 0 || cx >= W || cy < 0 || cy >= H) return q;
    const int r = (int)ctt_gaussian_radius(ceil(h), ceil(w));                                        // P:55-56: >= 0, truncated
    q.keep = 1, q.cx = cx, q.cy = cy, q.r = r < 0 ? 0 : r, q.cls = (int)c;
    q.w = (float)w, q.h = (float)h;
    return q;
}

__device__ __forceinline__ int ctt_image_objects(const void *__restrict__ num, int num_is_i64, int b, int N)
{
    const long long n = ctt_int_at(num, num_is_i64, (size_t)b);
    return n < 0 ? 0 : n > N ? N : (int)n;
}

// One workgroup per image: the rows K:18-29 packs -- the survivors to the front in their order, zeros behind them.
__global__ __launch_bounds__(kBlock) void k_ctt_objects(CttShape s, const void *__restrict__ boxes, int box_kind, const void *__restrict__ cls,
                                                       int cls_is_i64, const void *__restrict__ num, int num_is_i64, float *__restrict__ wh,
                                                       long long *__restrict__ ct_cls, long long *__restrict__ ct_ind,
                                                       float *__restrict__ ct_01, long long *__restrict__ ct_num)
{
    __shared__ int s_keep[kCttMaxN];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int nb = ctt_image_objects(num, num_is_i64, b, s.N);
    for (int n = tid; n < s.N; n += kBlock)
        s_keep[n] = n < nb ? ctt_object(boxes, box_kind, cls, cls_is_i64, (size_t)b * s.N + n, s.C, s.H, s.W).keep : 0;
    __syncthreads();
    int total = 0;
    for (int n = 0; n < s.N; ++n) total += s_keep[n];
    for (int n = tid; n < s.N; n += kBlock) {
        if (s_keep[n]) {
            const CttObject q = ctt_object(boxes, box_kind, cls, cls_is_i64, (size_t)b * s.N + n, s.C, s.H, s.W);
            int at = 0;
            for (int m = 0; m < n; ++m) at += s_keep[m];
            const size_t o = (size_t)b * s.N + at;
            wh[2 * o] = q.w, wh[2 * o + 1] = q.h;
            ct_cls[o] = q.cls, ct_ind[o] = (long long)q.cy * s.W + q.cx, ct_01[o] = 1.f;
        }
        if (n >= total) {
            const size_t o = (size_t)b * s.N + n;
            wh[2 * o] = 0.f, wh[2 * o + 1] = 0.f;
            ct_cls[o] = 0, ct_ind[o] = 0, ct_01[o] = 0.f;
        }
    }
    if (tid == 0) ct_num[b] = total;
}

// One workgroup per (tile, image): every element of the tile looks through the image's objects of its class (G:50-65 as a
// gather).  The rule of G:46 (values below eps * max become 0) is left out, it can never fire: the smallest value of a window is
// its corner, exp(-((r*r + r*r) / (sigma*sigma)) / 2) = exp(-36*r*r / ((2r+1)*(2r+1))) > exp(-9) > 1.2e-4 for every r, and the
// maximum is 1 (checked for r up to 2000).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_ctt_heatmap(CttShape s, const void *__restrict__ boxes, int box_kind, const void *__restrict__ cls,
                                                       int cls_is_i64, const void *__restrict__ num, int num_is_i64, float *__restrict__ hm)
{
    __shared__ int s_cx[kCttMaxN], s_cy[kCttMaxN], s_r[kCttMaxN], s_cls[kCttMaxN];
    __shared__ double s_ss[kCttMaxN];                  // sigma * sigma
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int nb = ctt_image_objects(num, num_is_i64, b, s.N);
    for (int n = tid; n < nb; n += kBlock) {
        const CttObject q = ctt_object(boxes, box_kind, cls, cls_is_i64, (size_t)b * s.N + n, s.C, s.H, s.W);
        const double sigma = (double)(2 * q.r + 1) / 6.0;
        s_cx[n] = q.cx, s_cy[n] = q.cy, s_r[n] = q.r, s_cls[n] = q.keep ? q.cls : -1;
        s_ss[n] = sigma * sigma;
    }
    __syncthreads();
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    int c[4], x[4], y[4];
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = p0 + i < s.E ? p0 + i : 0;
        c[i] = e / s.HW;
        const int rem = e - c[i] * s.HW;
        y[i] = rem / s.W, x[i] = rem - y[i] * s.W;
        v[i] = 0.f;
    }
    for (int n = 0; n < nb; ++n) {
        const int oc = s_cls[n], cx = s_cx[n], cy = s_cy[n], r = s_r[n];
        const double ss = s_ss[n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = x[i] - cx, dy = y[i] - cy;
            if (oc == c[i] && dx >= -r && dx <= r && dy >= -r && dy <= r) {
                const double fx = (double)dx, fy = (double)dy;
                const float g = (float)exp(-((fx * fx) / ss + (fy * fy) / ss) / 2.0);
                v[i] = g > v[i] ? g : v[i];
            }
        }
    }
    train_store4<VEC>(hm + (size_t)b * s.E, p0, s.E, v);
}

// L:9-11: the sigmoid and its clamp, binary64.  lo and hi are the float32 values torch.clamp compares a float32 tensor with.
__device__ __forceinline__ void ctt_sigmoid(float z, double &s, double &p)
{
    const double lo = (double)(float)1e-4, hi = (double)(float)(1.0 - 1e-4);
    s = 1.0 / (1.0 + exp(-(double)z));
    p = s < lo ? lo : s > hi ? hi : s;
}

__device__ __forceinline__ bool ctt_clamp_passes(double s)
{
    const double lo = (double)(float)1e-4, hi = (double)(float)(1.0 - 1e-4);
    return s >= lo && s <= hi;
}

// (1 - g)^4 of L:24 as two squarings.
__device__ __forceinline__ double ctt_neg_weight(float g)
{
    const double w = 1.0 - (double)g, w2 = w * w;
    return w2 * w2;
}

// One workgroup per (tile, image): the tile's sums of L:28-29 and its count of g == 1.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_ctt_focal_tiles(CttShape s, const float *__restrict__ hp, const float *__restrict__ hm,
                                                           double *__restrict__ part, long long *__restrict__ cnt)
{
    __shared__ double sh[kBlock];
    __shared__ long long shi[kBlock];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    float z[4], g[4];
    train_load4<VEC>(hp + (size_t)b * s.hp_stride, p0, s.E, 0.f, z);
    train_load4<VEC>(hm + (size_t)b * s.hm_stride, p0, s.E, 2.f, g);          // past the image: neither positive nor negative
    double pos[4], neg[4];
    long long np = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sg, p;
        ctt_sigmoid(z[i], sg, p);
        pos[i] = neg[i] = 0.0;
        if (g[i] == 1.f) {
            const double q = 1.0 - p;
            pos[i] = log(p) * (q * q);
            np += 1;
        } else if (g[i] < 1.f) {
            neg[i] = (log(1.0 - p) * (p * p)) * ctt_neg_weight(g[i]);
        }
    }
    const double lp = ((pos[0] + pos[1]) + pos[2]) + pos[3], ln = ((neg[0] + neg[1]) + neg[2]) + neg[3];
    const double tp = train_block_sum(lp, sh), tn = train_block_sum(ln, sh);
    const long long tc = train_block_sum(np, shi);
    if (tid == 0) {
        const size_t o = (size_t)b * s.tiles + tile;
        part[2 * o] = tp, part[2 * o + 1] = tn;
        cnt[o] = tc;
    }
}

// One workgroup per image: slot j sums the tiles j, j + 256, ... in ascending order, then the block order; the same for the
// objects of L:240-246 (an object is its two channels, c = 0 first).
__global__ __launch_bounds__(kBlock) void k_ctt_loss_images(CttShape s, const double *__restrict__ part, const long long *__restrict__ cnt,
                                                           const float *__restrict__ wp, const float *__restrict__ wh,
                                                           const void *__restrict__ ind, int ind_is_i64, const float *__restrict__ w01,
                                                           double *__restrict__ img, long long *__restrict__ imgcnt)
{
    __shared__ double sh[kBlock];
    __shared__ long long shi[kBlock];
    const int tid = threadIdx.x, b = blockIdx.x;
    double P = 0.0, Q = 0.0;
    long long np = 0;
    for (int t = tid; t < s.tiles; t += kTrainSlots) {
        const size_t o = (size_t)b * s.tiles + t;
        P += part[2 * o], Q += part[2 * o + 1];
        np += cnt[o];
    }
    const float *wb = wp + (size_t)b * s.wp_stride;
    double S = 0.0, M = 0.0;
    long long bad = 0;
    for (int n = tid; n < s.N; n += kTrainSlots) {
        const size_t o = (size_t)b * s.N + n;
        const long long i = ctt_int_at(ind, ind_is_i64, o);
        const double m = (double)w01[o];
        double obj = 0.0;
        if (i >= 0 && i < s.HW) {
            double el[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double d = (double)wb[(size_t)c * s.HW + (size_t)i] * m - (double)wh[2 * o + c] * m;
                const double z = fabs(d);
                el[c] = z < 1.0 ? (0.5 * z) * z : z - 0.5;
            }
            obj = el[0] + el[1];
        } else if (m != 0.0) {
            bad += 1;
        }
        S += obj, M += m;
    }
    const double iP = train_block_sum(P, sh), iQ = train_block_sum(Q, sh), iS = train_block_sum(S, sh), iM = train_block_sum(M, sh);
    const long long inp = train_block_sum(np, shi), ibad = train_block_sum(bad, shi);
    if (tid == 0) {
        img[4 * b] = iP, img[4 * b + 1] = iQ, img[4 * b + 2] = iS, img[4 * b + 3] = iM;
        imgcnt[2 * b] = inp, imgcnt[2 * b + 1] = ibad;
    }
}

// One thread: the batch in ascending b, then L:35-38 and L:245.
__global__ void k_ctt_loss_final(int B, const double *__restrict__ img, const long long *__restrict__ imgcnt, float *__restrict__ losses,
                                long long *__restrict__ state)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double P = 0.0, Q = 0.0, S = 0.0, M = 0.0;
    long long np = 0, bad = 0;
    for (int b = 0; b < B; ++b) {
        P += img[4 * b], Q += img[4 * b + 1], S += img[4 * b + 2], M += img[4 * b + 3];
        np += imgcnt[2 * b], bad += imgcnt[2 * b + 1];
    }
    losses[0] = np == 0 ? (float)(-Q) : (float)(-(P + Q) / (double)np);
    losses[1] = bad != 0 ? __builtin_nanf("") : (float)(S / (M * 2.0 + 1e-4));
    state[0] = np, state[1] = bad, state[3] = 0;
    reinterpret_cast<double *>(state)[2] = M;
}

// One workgroup per (tile, image): the gradient of the tile's logits, from the recomputed sigmoid.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_ctt_focal_backward(CttShape s, const float *__restrict__ hp, const float *__restrict__ hm,
                                                              const long long *__restrict__ state, const float *__restrict__ go,
                                                              float *__restrict__ gh)
{
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    const long long np = state[0];
    const double k = np == 0 ? -(double)go[0] : -(double)go[0] / (double)np;
    float z[4], g[4], out[4];
    train_load4<VEC>(hp + (size_t)b * s.hp_stride, p0, s.E, 0.f, z);
    train_load4<VEC>(hm + (size_t)b * s.hm_stride, p0, s.E, 2.f, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sg, p;
        ctt_sigmoid(z[i], sg, p);
        const double q = 1.0 - p;
        double dp = 0.0;
        if (g[i] == 1.f) dp = (q * q) / p - (2.0 * q) * log(p);
        else if (g[i] < 1.f) dp = ((2.0 * p) * log(q) - (p * p) / q) * ctt_neg_weight(g[i]);
        out[i] = ctt_clamp_passes(sg) ? (float)((k * dp) * ((1.0 - sg) * sg)) : 0.f;
    }
    train_store4<VEC>(gh + (size_t)b * s.E, p0, s.E, out);
}

// One workgroup per (tile of the [2*H*W] image, image): +0, or NaN after a bad index.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_ctt_wh_fill(int E2, const long long *__restrict__ state, float *__restrict__ gw)
{
    const int p0 = blockIdx.x * kTrainTile + threadIdx.x * kTrainLanePix;
    const float f = state[1] != 0 ? __builtin_nanf("") : 0.f;
    const float v[4] = {f, f, f, f};
    train_store4<VEC>(gw + (size_t)blockIdx.y * E2, p0, E2, v);
}

// One workgroup per image, after the fill: the first object of an index owns it and adds the objects that share it in
// ascending order, float32 (what scatter_add does on one core).
__global__ __launch_bounds__(kBlock) void k_ctt_wh_backward(CttShape s, const float *__restrict__ wp, const float *__restrict__ wh,
                                                           const void *__restrict__ ind, int ind_is_i64, const float *__restrict__ w01,
                                                           const long long *__restrict__ state, const float *__restrict__ go,
                                                           float *__restrict__ gw)
{
    __shared__ int s_ind[kCttMaxN];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int n = tid; n < s.N; n += kBlock) {
        const long long i = ctt_int_at(ind, ind_is_i64, (size_t)b * s.N + n);
        s_ind[n] = (i >= 0 && i < s.HW) ? (int)i : -1;
    }
    __syncthreads();
    if (state[1] != 0) return;                        // the fill wrote NaN; nothing follows the barrier
    const float den = (float)reinterpret_cast<const double *>(state)[2] * 2.f + 1e-4f;
    const float v = go[1] / den;
    const float *wb = wp + (size_t)b * s.wp_stride;
    float *gb = gw + (size_t)b * 2 * s.HW;
    for (int n = tid; n < s.N; n += kBlock) {
        const int i = s_ind[n];
        if (i < 0) continue;
        bool owner = true;
        for (int m = 0; m < n; ++m) owner = owner && s_ind[m] != i;
        if (!owner) continue;
        float acc[2] = {0.f, 0.f};
        for (int m = n; m < s.N; ++m) {
            if (s_ind[m] != i) continue;
            const size_t o = (size_t)b * s.N + m;
            const float w = w01[o];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d = train_d(wb[(size_t)c * s.HW + i], wh[2 * o + c], w);
                acc[c] += (d < -1.f ? -v : d > 1.f ? v : v * d) * w;
            }
        }
        gb[i] = acc[0], gb[(size_t)s.HW + i] = acc[1];
    }
}

// The size checks every entry point shares.  Fills s but for the strides.
int ctt_shape(CttShape &s, int B, int N, int C, int H, int W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(PVV_E_ARG, "ct_train: B, C, H, W must be positive");
    if (B > 65535) return fail(PVV_E_ARG, "ct_train: B > 65535: split the batch");
    if (N < 1 || N > kCttMaxN) return fail(PVV_E_ARG, "ct_train: N must lie in [1, 512]");
    const long long HW = (long long)H * W, lim = 1ll << 31;
    if (2 * HW >= lim || (long long)C * HW >= lim) return fail(PVV_E_ARG, "ct_train: C * H * W and 2 * H * W must be < 2^31 (int32 indexing)");
    s.B = B, s.N = N, s.C = C, s.H = H, s.W = W, s.HW = (int)HW, s.E = (int)(C * HW);
    s.tiles = (int)((C * HW + kTrainTile - 1) / kTrainTile);
    s.hp_stride = s.wp_stride = s.hm_stride = 0;
    return PVV_OK;
}

static_assert(kCttMaxN == 512, "the message of ctt_shape names the limit");

struct CttArgs {
    const float *hp, *wp, *hm, *wh;
    const void *ind;
    const float *w01;
};

// The checks forward and backward share on their inputs; fills the strides of s and whether the 16-byte form applies.
int ctt_inputs(CttShape &s, const CttArgs &a, long long hp_stride, long long wp_stride, long long hm_stride, bool &vec)
{
    if (!a.hp || !a.wp || !a.hm || !a.wh || !a.ind || !a.w01) return fail(PVV_E_ARG, "ct_train: NULL device pointer");
    if (hp_stride < s.E || hm_stride < s.E || wp_stride < 2ll * s.HW) return fail(PVV_E_ARG, "ct_train: an image stride is smaller than its image");
    s.hp_stride = hp_stride, s.wp_stride = wp_stride, s.hm_stride = hm_stride;
    vec = s.E % 4 == 0 && train_aligned(a.hp, hp_stride) && train_aligned(a.hm, hm_stride);
    return PVV_OK;
}

// k<VEC>, the 16-byte or the scalar form of a kernel, on a grid of kBlock-lane workgroups.
#define CTT_LAUNCH(k, vec, grid, st, ...)                                                      \
    do {                                                                                       \
        if (vec) hipLaunchKernelGGL(k<true>, grid, dim3(kBlock), 0, st, __VA_ARGS__);          \
        else hipLaunchKernelGGL(k<false>, grid, dim3(kBlock), 0, st, __VA_ARGS__);             \
    } while (0)

}  // namespace

PVV_EXPORT int pvv_ct_targets(const void *d_boxes, int box_kind, const void *d_cls, int cls_is_i64, const void *d_num, int num_is_i64, int B,
                              int N, int C, int H, int W, float *d_ct_hm, float *d_wh, long long *d_ct_cls, long long *d_ct_ind,
                              float *d_ct_01, long long *d_ct_num, void *stream)
{
    CttShape s;
    if (int e = ctt_shape(s, B, N, C, H, W)) return e;
    if (!d_boxes || !d_cls || !d_num || !d_ct_hm || !d_wh || !d_ct_cls || !d_ct_ind || !d_ct_01 || !d_ct_num)
        return fail(PVV_E_ARG, "ct_train: NULL device pointer");
    if (box_kind != PVV_BOX_F32 && box_kind != PVV_BOX_I32 && box_kind != PVV_BOX_I64)
        return fail(PVV_E_ARG, "ct_train: box_kind must be PVV_BOX_F32, PVV_BOX_I32 or PVV_BOX_I64");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ctt_objects, dim3(B), dim3(kBlock), 0, st, s, d_boxes, box_kind, d_cls, cls_is_i64, d_num, num_is_i64, d_wh, d_ct_cls,
                       d_ct_ind, d_ct_01, d_ct_num);
    if (int e = check_launch("k_ctt_objects")) return e;
    CTT_LAUNCH(k_ctt_heatmap, s.E % 4 == 0 && train_aligned(d_ct_hm, 0), dim3(s.tiles, B), st, s, d_boxes, box_kind, d_cls, cls_is_i64, d_num,
               num_is_i64, d_ct_hm);
    return check_launch("k_ctt_heatmap");
}

PVV_EXPORT size_t pvv_ct_loss_workspace_bytes(int B, int C, int H, int W)
{
    CttShape s;
    if (ctt_shape(s, B, 1, C, H, W)) return 0;
    return ctt_layout(B, s.tiles).total;
}

PVV_EXPORT int pvv_ct_loss_forward(const float *d_hm_pred, long long hp_image_stride, const float *d_wh_pred, long long wp_image_stride,
                                   const float *d_ct_hm, long long hm_image_stride, const float *d_wh, const void *d_ct_ind,
                                   int ind_is_i64, const float *d_ct_01, int B, int N, int C, int H, int W, void *workspace,
                                   size_t workspace_bytes, float *d_out_losses, void *d_out_state, void *stream)
{
    CttShape s;
    if (int e = ctt_shape(s, B, N, C, H, W)) return e;
    const CttArgs a = {d_hm_pred, d_wh_pred, d_ct_hm, d_wh, d_ct_ind, d_ct_01};
    bool vec = false;
    if (int e = ctt_inputs(s, a, hp_image_stride, wp_image_stride, hm_image_stride, vec)) return e;
    if (!d_out_losses) return fail(PVV_E_ARG, "ct_train: NULL device pointer");
    if (int e = loss_state(d_out_state, "ct_train")) return e;
    const LossLayout L = ctt_layout(B, s.tiles);
    if (int e = train_ws(workspace, workspace_bytes, L.total)) return e;
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    double *part = (double *)(ws + L.part), *img = (double *)(ws + L.img);
    long long *cnt = (long long *)(ws + L.cnt), *imgcnt = (long long *)(ws + L.imgcnt);
    CTT_LAUNCH(k_ctt_focal_tiles, vec, dim3(s.tiles, B), st, s, a.hp, a.hm, part, cnt);
    if (int e = check_launch("k_ctt_focal_tiles")) return e;
    hipLaunchKernelGGL(k_ctt_loss_images, dim3(B), dim3(kBlock), 0, st, s, (const double *)part, (const long long *)cnt, a.wp, a.wh, a.ind,
                       ind_is_i64, a.w01, img, imgcnt);
    if (int e = check_launch("k_ctt_loss_images")) return e;
    hipLaunchKernelGGL(k_ctt_loss_final, dim3(1), dim3(64), 0, st, B, (const double *)img, (const long long *)imgcnt, d_out_losses,
                       (long long *)d_out_state);
    return check_launch("k_ctt_loss_final");
}

PVV_EXPORT int pvv_ct_loss_backward(const float *d_hm_pred, long long hp_image_stride, const float *d_wh_pred, long long wp_image_stride,
                                    const float *d_ct_hm, long long hm_image_stride, const float *d_wh, const void *d_ct_ind,
                                    int ind_is_i64, const float *d_ct_01, int B, int N, int C, int H, int W, const void *d_out_state,
                                    const float *d_grad_losses, float *d_grad_hm, float *d_grad_wh, void *stream)
{
    CttShape s;
    if (int e = ctt_shape(s, B, N, C, H, W)) return e;
    const CttArgs a = {d_hm_pred, d_wh_pred, d_ct_hm, d_wh, d_ct_ind, d_ct_01};
    bool vec = false;
    if (int e = ctt_inputs(s, a, hp_image_stride, wp_image_stride, hm_image_stride, vec)) return e;
    if (!d_grad_losses || !d_grad_hm || !d_grad_wh) return fail(PVV_E_ARG, "ct_train: NULL device pointer");
    if (int e = loss_state(d_out_state, "ct_train")) return e;
    hipStream_t st = (hipStream_t)stream;
    const long long *state = (const long long *)d_out_state;
    CTT_LAUNCH(k_ctt_focal_backward, vec && train_aligned(d_grad_hm, 0), dim3(s.tiles, B), st, s, a.hp, a.hm, state, d_grad_losses, d_grad_hm);
    if (int e = check_launch("k_ctt_focal_backward")) return e;
    const int E2 = 2 * s.HW, tiles2 = (int)((2ll * s.HW + kTrainTile - 1) / kTrainTile);
    CTT_LAUNCH(k_ctt_wh_fill, E2 % 4 == 0 && train_aligned(d_grad_wh, 0), dim3(tiles2, B), st, E2, state, d_grad_wh);
    if (int e = check_launch("k_ctt_wh_fill")) return e;
    hipLaunchKernelGGL(k_ctt_wh_backward, dim3(B), dim3(kBlock), 0, st, s, a.wp, a.wh, a.ind, ind_is_i64, a.w01, state, d_grad_losses, d_grad_wh);
    return check_launch("k_ctt_wh_backward");
}
