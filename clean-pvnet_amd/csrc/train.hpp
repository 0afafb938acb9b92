// train.hpp -- PVNet's vote targets and training loss (include/pvnet_vote.h, "Training: vote targets and the PVNet loss").
// Included at the end of pvnet_vote.hip: built with -ffp-contract=off, so every operation below rounds once, in the order
// written.  The numpy twin (tests/train_twin.py) follows the same order.
//
// Reference behaviour restated (paths relative to the reference's root):
//   D = lib/utils/pvnet/pvnet_data_utils.py:30-44 (compute_vertex)      T = lib/train/trainers/pvnet.py:25-34 (the loss)
//
// Streaming kernels: a lane owns kTrainLanePix consecutive pixels of the flattened plane, so every channel plane is read and
// written with 16-byte accesses when the plane size and the bases allow it (VEC); the scalar form has the same arithmetic.
// Every sum is binary64 in one order that the launch does not choose: lane, tile (a workgroup), image, batch.  No float
// atomics: per-tile partials go to the workspace and two small launches sum them.  The target field is recomputed per
// pixel from the mask and the keypoints (KPT) or read (the field form); the backward pass recomputes d and the softmax.
//
// Host side: what this loss and the detector's (ct_train.hpp) have in common is stated here once -- the workspace layout
// (loss_layout, each loss names its four multipliers), the out_state check (loss_state, by message prefix) and the workspace
// check (train_ws).  Every entry point picks its kernel's template form through TRAIN_DISPATCH / TRAIN_DISPATCH_VEC.
#pragma once

namespace {

constexpr int kTrainLanePix = PVV_TRAIN_LANE_PIXELS;
constexpr int kTrainTile = PVV_TRAIN_TILE;            // pixels of a workgroup
constexpr int kTrainSlots = PVV_TRAIN_IMAGE_SLOTS;    // slot j of an image sums its tiles j, j + 256, ...

static_assert(kTrainTile == kBlock * kTrainLanePix && kTrainSlots == kBlock && kTrainLanePix == 4, "one lane, four pixels; one tree for tiles and slots");

struct TrainShape {
    int B, K, C, H, W, HW, tiles;
    long long vp_stride, sp_stride, tg_stride;        // elements between two images of vertex_pred / seg_pred / target
};

// The workspace of a fused loss (this one and ct_train.hpp's): per (image, tile) part_f64 binary64 partials and part_i64 integer
// counts, then per image img_f64 and img_i64 of them; every section starts on a 256-byte boundary.
struct LossLayout { size_t part, cnt, img, imgcnt, total; };

LossLayout loss_layout(int B, int tiles, int part_f64, int part_i64, int img_f64, int img_i64)
{
    LossLayout L;
    const size_t bt = (size_t)B * tiles;
    L.part = 0;
    L.cnt = align_up(L.part + bt * part_f64 * sizeof(double));
    L.img = align_up(L.cnt + bt * part_i64 * sizeof(long long));
    L.imgcnt = align_up(L.img + (size_t)B * img_f64 * sizeof(double));
    L.total = align_up(L.imgcnt + (size_t)B * img_i64 * sizeof(long long));
    return L;
}

// Here: two partials and two counts per (image, tile), the same per image.
LossLayout train_layout(int B, int tiles) { return loss_layout(B, tiles, 2, 2, 2, 2); }

// The order of block_sum (eval_common.hpp): the tree of vote_common.hpp, behind a barrier because sh is used again and again.
template <typename T>
__device__ T train_block_sum(T v, T *sh)
{
    __syncthreads();
    return block_tree_sum(v, sh, (int)threadIdx.x);
}

template <typename T>
struct alignas(sizeof(T) * 4 > 16 ? 16 : sizeof(T) * 4) TrainVec4 { T v[4]; };

// The lane's four values of one plane; pixels >= HW are `fill` and are never read.  VEC: HW % 4 == 0 and the plane is 16-byte
// aligned (4 * sizeof(T) for narrower T), so the four pixels lie inside together or not at all.
template <bool VEC, typename T>
__device__ __forceinline__ void train_load4(const T *__restrict__ plane, int p0, int HW, T fill, T (&out)[4])
{
    if constexpr (VEC) {
        if (p0 < HW) {
            const TrainVec4<T> q = *reinterpret_cast<const TrainVec4<T> *>(plane + p0);
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = q.v[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = fill;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = (p0 + i < HW) ? plane[p0 + i] : fill;
    }
}

template <bool VEC>
__device__ __forceinline__ void train_store4(float *__restrict__ plane, int p0, int HW, const float (&v)[4])
{
    if constexpr (VEC) {
        if (p0 < HW) {
            TrainVec4<float> q;
#pragma unroll
            for (int i = 0; i < 4; ++i) q.v[i] = v[i];
            *reinterpret_cast<TrainVec4<float> *>(plane + p0) = q;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (p0 + i < HW) plane[p0 + i] = v[i];
    }
}

// D:35-38 for one (pixel, keypoint), binary64: the unit vector from the pixel to the keypoint, rounded to float32 once.
__device__ __forceinline__ void train_target(double kx, double ky, int x, int y, float &tx, float &ty)
{
    const double dx = kx - (double)x, dy = ky - (double)y;
    double n = sqrt(dx * dx + dy * dy);
    if (n < 1e-3) n += 1e-3;
    tx = (float)(dx / n), ty = (float)(dy / n);
}

// T:26: d = pred * w - target * w, and the smooth L1 element of it (beta = 1), float32.
__device__ __forceinline__ float train_d(float pred, float tgt, float w) { return pred * w - tgt * w; }

__device__ __forceinline__ float train_elem(float d)
{
    const float z = fabsf(d);
    return z < 1.f ? (0.5f * z) * z : z - 0.5f;
}

// The keypoints of image b in LDS as binary64 (float32 widened exactly): s_kpt[2k] = x, s_kpt[2k + 1] = y.
__device__ __forceinline__ void train_stage_kpt(const void *__restrict__ kpt, int kpt_is_f64, int b, int K, double *s_kpt)
{
    for (int i = threadIdx.x; i < 2 * K; i += kBlock) {
        const size_t e = (size_t)b * 2 * K + i;
        s_kpt[i] = kpt_is_f64 ? ((const double *)kpt)[e] : (double)((const float *)kpt)[e];
    }
    __syncthreads();
}

// What a lane knows of its four pixels before it touches a prediction.
template <typename MaskT>
struct TrainPix {
    float w[4];            // float(mask)
    bool fg[4];            // mask == 1: the pixels that have a target
    bool seg[4];           // inside the plane and the label lies in [0, C)
    int label[4], x[4], y[4];
    long long msum, bad;
};

template <bool VEC, typename MaskT>
__device__ __forceinline__ TrainPix<MaskT> train_pixels(const TrainShape &s, const MaskT *__restrict__ mask, int b, int p0)
{
    TrainPix<MaskT> q;
    MaskT m[4];
    train_load4<VEC>(mask + (size_t)b * s.HW, p0, s.HW, (MaskT)0, m);
    q.msum = 0, q.bad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool inside = p0 + i < s.HW;
        const long long v = (long long)m[i];
        const bool ok = v >= 0 && v < s.C;
        q.w[i] = (float)m[i];
        q.fg[i] = v == 1;
        q.seg[i] = inside && ok;
        q.label[i] = ok ? (int)v : -1;
        q.msum = (long long)((unsigned long long)q.msum + (unsigned long long)v);
        q.bad += (inside && !ok) ? 1 : 0;
        const int p = inside ? p0 + i : 0;
        q.y[i] = p / s.W, q.x[i] = p - q.y[i] * s.W;
    }
    return q;
}

// The lane's targets of keypoint k (channels 2k, 2k + 1).
template <bool KPT, bool VEC, typename MaskT>
__device__ __forceinline__ void train_targets(const TrainShape &s, const TrainPix<MaskT> &q, const double *s_kpt, const float *__restrict__ tb,
                                              int k, int p0, float (&tx)[4], float (&ty)[4])
{
    if constexpr (KPT) {
        const double kx = s_kpt[2 * k], ky = s_kpt[2 * k + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            tx[i] = ty[i] = 0.f;
            if (q.fg[i]) train_target(kx, ky, q.x[i], q.y[i], tx[i], ty[i]);
        }
    } else {
        train_load4<VEC>(tb + (size_t)(2 * k) * s.HW, p0, s.HW, 0.f, tx);
        train_load4<VEC>(tb + (size_t)(2 * k + 1) * s.HW, p0, s.HW, 0.f, ty);
    }
}

// m = max_c z_c for the lane's pixels (z > m ? z : m from z_0 on).
template <bool VEC>
__device__ __forceinline__ void train_seg_max(const TrainShape &s, const float *__restrict__ sb, int p0, float (&mx)[4])
{
    train_load4<VEC>(sb, p0, s.HW, 0.f, mx);
    for (int c = 1; c < s.C; ++c) {
        float z[4];
        train_load4<VEC>(sb + (size_t)c * s.HW, p0, s.HW, 0.f, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) mx[i] = z[i] > mx[i] ? z[i] : mx[i];
    }
}

// One workgroup per (tile, image): the tile's vote sum, seg sum, mask sum and bad-label count.
template <bool KPT, bool VEC, typename MaskT>
__global__ __launch_bounds__(kBlock) void k_train_loss_tiles(TrainShape s, const float *__restrict__ vp, const float *__restrict__ sp,
                                                             const MaskT *__restrict__ mask, const void *__restrict__ kpt, int kpt_is_f64,
                                                             const float *__restrict__ target, double *__restrict__ part,
                                                             long long *__restrict__ cnt)
{
    __shared__ double sh[kBlock];
    __shared__ long long shi[kBlock];
    __shared__ double s_kpt[KPT ? 2 * PVV_TRAIN_MAX_K : 2];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    if constexpr (KPT) train_stage_kpt(kpt, kpt_is_f64, b, s.K, s_kpt);
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    const TrainPix<MaskT> q = train_pixels<VEC>(s, mask, b, p0);

    const float *vb = vp + (size_t)b * s.vp_stride;
    const float *tb = KPT ? nullptr : target + (size_t)b * s.tg_stride;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < s.K; ++k) {
        float px[4], py[4], tx[4], ty[4];
        train_load4<VEC>(vb + (size_t)(2 * k) * s.HW, p0, s.HW, 0.f, px);
        train_load4<VEC>(vb + (size_t)(2 * k + 1) * s.HW, p0, s.HW, 0.f, py);
        train_targets<KPT, VEC>(s, q, s_kpt, tb, k, p0, tx, ty);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[i] += (double)train_elem(train_d(px[i], tx[i], q.w[i]));
            acc[i] += (double)train_elem(train_d(py[i], ty[i], q.w[i]));
        }
    }
    const double vote = ((acc[0] + acc[1]) + acc[2]) + acc[3];

    const float *sb = sp + (size_t)b * s.sp_stride;
    float mx[4];
    train_seg_max<VEC>(s, sb, p0, mx);
    double es[4] = {0.0, 0.0, 0.0, 0.0};
    float zl[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < s.C; ++c) {
        float z[4];
        train_load4<VEC>(sb + (size_t)c * s.HW, p0, s.HW, 0.f, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            es[i] += exp((double)z[i] - (double)mx[i]);
            if (c == q.label[i]) zl[i] = z[i];
        }
    }
    double term[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) term[i] = q.seg[i] ? ((double)mx[i] - (double)zl[i]) + log(es[i]) : 0.0;
    const double seg = ((term[0] + term[1]) + term[2]) + term[3];

    const double tv = train_block_sum(vote, sh), ts = train_block_sum(seg, sh);
    const long long tm = train_block_sum(q.msum, shi), tbad = train_block_sum(q.bad, shi);
    if (tid == 0) {
        const size_t o = ((size_t)b * s.tiles + tile) * 2;
        part[o] = tv, part[o + 1] = ts;
        cnt[o] = tm, cnt[o + 1] = tbad;
    }
}

// One workgroup per image: slot j sums the tiles j, j + 256, ... in ascending order, then the block order.
__global__ __launch_bounds__(kBlock) void k_train_loss_images(int tiles, const double *__restrict__ part, const long long *__restrict__ cnt,
                                                              double *__restrict__ img, long long *__restrict__ imgcnt)
{
    __shared__ double sh[kBlock];
    __shared__ long long shi[kBlock];
    const int tid = threadIdx.x, b = blockIdx.x;
    double v = 0.0, g = 0.0;
    long long m = 0, bad = 0;
    for (int t = tid; t < tiles; t += kTrainSlots) {
        const size_t o = ((size_t)b * tiles + t) * 2;
        v += part[o], g += part[o + 1];
        m += cnt[o], bad += cnt[o + 1];
    }
    const double iv = train_block_sum(v, sh), ig = train_block_sum(g, sh);
    const long long im = train_block_sum(m, shi), ibad = train_block_sum(bad, shi);
    if (tid == 0) {
        img[2 * b] = iv, img[2 * b + 1] = ig;
        imgcnt[2 * b] = im, imgcnt[2 * b + 1] = ibad;
    }
}

// One thread: the batch in ascending b, then T:26-27 and the mean of the cross entropy.
__global__ void k_train_loss_final(int B, int K, double N, const double *__restrict__ img, const long long *__restrict__ imgcnt,
                                   float *__restrict__ losses, long long *__restrict__ state)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double S = 0.0, G = 0.0;
    long long M = 0, bad = 0;
    for (int b = 0; b < B; ++b) {
        S += img[2 * b], G += img[2 * b + 1];
        M += imgcnt[2 * b], bad += imgcnt[2 * b + 1];
    }
    const float wsum = (float)M;
    float vote = ((float)S / wsum) / (float)(2 * K);
    float seg = (float)(G / N);
    if (bad != 0) vote = seg = __builtin_nanf("");
    losses[0] = vote, losses[1] = seg;
    state[0] = M, state[1] = bad;
}

// One workgroup per (tile, image): both gradients of the tile, from the recomputed d and softmax.
template <bool KPT, bool VEC, typename MaskT>
__global__ __launch_bounds__(kBlock) void k_train_loss_backward(TrainShape s, double N, const float *__restrict__ vp, const float *__restrict__ sp,
                                                                const MaskT *__restrict__ mask, const void *__restrict__ kpt, int kpt_is_f64,
                                                                const float *__restrict__ target, const long long *__restrict__ state,
                                                                const float *__restrict__ go, float *__restrict__ gv, float *__restrict__ gs)
{
    __shared__ double s_kpt[KPT ? 2 * PVV_TRAIN_MAX_K : 2];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    if constexpr (KPT) train_stage_kpt(kpt, kpt_is_f64, b, s.K, s_kpt);
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    const TrainPix<MaskT> q = train_pixels<VEC>(s, mask, b, p0);
    const bool bad = state[1] != 0;
    const float nan = __builtin_nanf("");
    const float wsum = (float)state[0];
    const float sv = (go[0] / (float)(2 * s.K)) / wsum;
    const double gseg = (double)go[1];

    const float *vb = vp + (size_t)b * s.vp_stride;
    const float *tb = KPT ? nullptr : target + (size_t)b * s.tg_stride;
    float *gvb = gv + (size_t)b * 2 * s.K * s.HW;
    for (int k = 0; k < s.K; ++k) {
        float px[4], py[4], tx[4], ty[4], gx[4], gy[4];
        train_load4<VEC>(vb + (size_t)(2 * k) * s.HW, p0, s.HW, 0.f, px);
        train_load4<VEC>(vb + (size_t)(2 * k + 1) * s.HW, p0, s.HW, 0.f, py);
        train_targets<KPT, VEC>(s, q, s_kpt, tb, k, p0, tx, ty);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dx = train_d(px[i], tx[i], q.w[i]), dy = train_d(py[i], ty[i], q.w[i]);
            gx[i] = bad ? nan : (dx < -1.f ? -sv : dx > 1.f ? sv : sv * dx) * q.w[i];
            gy[i] = bad ? nan : (dy < -1.f ? -sv : dy > 1.f ? sv : sv * dy) * q.w[i];
        }
        train_store4<VEC>(gvb + (size_t)(2 * k) * s.HW, p0, s.HW, gx);
        train_store4<VEC>(gvb + (size_t)(2 * k + 1) * s.HW, p0, s.HW, gy);
    }

    const float *sb = sp + (size_t)b * s.sp_stride;
    float *gsb = gs + (size_t)b * s.C * s.HW;
    float mx[4];
    train_seg_max<VEC>(s, sb, p0, mx);
    double es[4] = {0.0, 0.0, 0.0, 0.0}, rest[4] = {0.0, 0.0, 0.0, 0.0};   // the sum of all e_c and of those beside the label
    for (int c = 0; c < s.C; ++c) {
        float z[4];
        train_load4<VEC>(sb + (size_t)c * s.HW, p0, s.HW, 0.f, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double e = exp((double)z[i] - (double)mx[i]);
            es[i] += e;
            if (c != q.label[i]) rest[i] += e;
        }
    }
    for (int c = 0; c < s.C; ++c) {
        float z[4], g[4];
        train_load4<VEC>(sb + (size_t)c * s.HW, p0, s.HW, 0.f, z);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double e = exp((double)z[i] - (double)mx[i]);
            const double v = c == q.label[i] ? ((-gseg * rest[i]) / es[i]) / N : ((gseg * e) / es[i]) / N;
            g[i] = bad ? nan : (float)v;
        }
        train_store4<VEC>(gsb + (size_t)c * s.HW, p0, s.HW, g);
    }
}

// One workgroup per (tile, image): the field D writes, channel 2k = x and 2k + 1 = y.
template <bool VEC, typename MaskT>
__global__ __launch_bounds__(kBlock) void k_train_vertex_target(TrainShape s, const MaskT *__restrict__ mask, const void *__restrict__ kpt,
                                                                int kpt_is_f64, float *__restrict__ out)
{
    __shared__ double s_kpt[2 * PVV_TRAIN_MAX_K];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    train_stage_kpt(kpt, kpt_is_f64, b, s.K, s_kpt);
    const int p0 = tile * kTrainTile + tid * kTrainLanePix;
    const TrainPix<MaskT> q = train_pixels<VEC>(s, mask, b, p0);
    float *ob = out + (size_t)b * 2 * s.K * s.HW;
    for (int k = 0; k < s.K; ++k) {
        float tx[4], ty[4];
        train_targets<true, VEC>(s, q, s_kpt, nullptr, k, p0, tx, ty);
        train_store4<VEC>(ob + (size_t)(2 * k) * s.HW, p0, s.HW, tx);
        train_store4<VEC>(ob + (size_t)(2 * k + 1) * s.HW, p0, s.HW, ty);
    }
}

// The size checks every entry point shares; K = 1, C = 1 where they do not matter.  Fills s but for the strides.
int train_shape(TrainShape &s, int B, int K, int C, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return fail(PVV_E_ARG, "train: B, H, W must be positive");
    if (B > 65535) return fail(PVV_E_ARG, "train: B > 65535: split the batch");
    if (K < 1 || K > PVV_TRAIN_MAX_K) return fail(PVV_E_ARG, "train: K must lie in [1, 64]");
    if (C < 1 || C > PVV_TRAIN_MAX_C) return fail(PVV_E_ARG, "train: C must lie in [1, 16]");
    const long long HW = (long long)H * W, lim = 1ll << 31;
    if (HW >= lim || 2ll * K * HW >= lim || (long long)C * HW >= lim)
        return fail(PVV_E_ARG, "train: a per-image tensor has 2^31 elements or more (int32 indexing)");
    if ((long long)B * HW >= (1ll << 53)) return fail(PVV_E_ARG, "train: B * H * W must be < 2^53");
    s.B = B, s.K = K, s.C = C, s.H = H, s.W = W, s.HW = (int)HW, s.tiles = (int)((HW + kTrainTile - 1) / kTrainTile);
    s.vp_stride = s.sp_stride = s.tg_stride = 0;
    return PVV_OK;
}

bool train_aligned(const void *p, long long stride) { return (uintptr_t)p % 16 == 0 && stride % 4 == 0; }

struct TrainArgs {
    const float *vp, *sp;
    const void *mask, *kpt;
    int mask_kind, kpt_is_f64;
    const float *target;
};

int train_mask_kind(int kind)
{
    if (kind != PVV_MASK_U8 && kind != PVV_MASK_I32 && kind != PVV_MASK_I64)
        return fail(PVV_E_ARG, "train: mask_kind must be PVV_MASK_U8, PVV_MASK_I32 or PVV_MASK_I64");
    return PVV_OK;
}

// The checks forward and backward share on their inputs; fills the strides of s and whether the 16-byte form applies.
int train_inputs(TrainShape &s, const TrainArgs &a, long long vp_stride, long long sp_stride, long long tg_stride, bool &vec)
{
    if (!a.vp || !a.sp || !a.mask) return fail(PVV_E_ARG, "train: NULL device pointer");
    if ((a.kpt != nullptr) == (a.target != nullptr)) return fail(PVV_E_ARG, "train: exactly one of kpt_2d and target must be given");
    if (int e = train_mask_kind(a.mask_kind)) return e;
    if (vp_stride < 2ll * s.K * s.HW || sp_stride < (long long)s.C * s.HW || (a.target && tg_stride < 2ll * s.K * s.HW))
        return fail(PVV_E_ARG, "train: an image stride is smaller than its image");
    s.vp_stride = vp_stride, s.sp_stride = sp_stride, s.tg_stride = a.target ? tg_stride : 0;
    vec = s.HW % 4 == 0 && train_aligned(a.vp, vp_stride) && train_aligned(a.sp, sp_stride) && train_aligned(a.mask, 0) &&
          (!a.target || train_aligned(a.target, tg_stride));
    return PVV_OK;
}

int train_ws(const void *ws, size_t ws_bytes, size_t need)
{
    if (!ws) return fail(PVV_E_ARG, "train: NULL workspace");
    if ((uintptr_t)ws % 256 != 0) return fail(PVV_E_ARG, "train: workspace must be 256-byte aligned");
    if (ws_bytes < need) return fail(PVV_E_WORKSPACE, "train: workspace too small");
    return PVV_OK;
}

// The out_state of a fused loss (this one and ct_train.hpp's), which the forward pass writes and the backward pass reads.
int loss_state(const void *state, const char *prefix)
{
    char msg[96];
    if (state && (uintptr_t)state % 8 == 0) return PVV_OK;
    snprintf(msg, sizeof(msg), state ? "%s: out_state must be 8-byte aligned" : "%s: NULL device pointer", prefix);
    return fail(PVV_E_ARG, msg);
}

template <bool KPT, bool VEC, typename MaskT>
void train_launch_tiles(const TrainShape &s, const TrainArgs &a, double *part, long long *cnt, hipStream_t st)
{
    hipLaunchKernelGGL((k_train_loss_tiles<KPT, VEC, MaskT>), dim3(s.tiles, s.B), dim3(kBlock), 0, st, s, a.vp, a.sp, (const MaskT *)a.mask, a.kpt,
                       a.kpt_is_f64, a.target, part, cnt);
}

template <bool KPT, bool VEC, typename MaskT>
void train_launch_backward(const TrainShape &s, const TrainArgs &a, const long long *state, const float *go, float *gv, float *gs,
                           hipStream_t st)
{
    hipLaunchKernelGGL((k_train_loss_backward<KPT, VEC, MaskT>), dim3(s.tiles, s.B), dim3(kBlock), 0, st, s, (double)s.B * (double)s.HW, a.vp, a.sp,
                       (const MaskT *)a.mask, a.kpt, a.kpt_is_f64, a.target, state, go, gv, gs);
}

// f<KPT, VEC, MaskT>(args...), or f<VEC, MaskT>(args...) where there is no target field to choose, for the form the call has:
// one set of kernels, the template parameters from run-time values.  kind has passed train_mask_kind.
#define TRAIN_DISPATCH(f, kpt, vec, kind, ...) TRAIN_BY_MASK(TRAIN_KPT_VEC, kind, f, kpt, vec, __VA_ARGS__)
#define TRAIN_DISPATCH_VEC(f, vec, kind, ...) TRAIN_BY_MASK(TRAIN_VEC, kind, f, vec, __VA_ARGS__)
#define TRAIN_BY_MASK(FORM, kind, ...)                                       \
    do {                                                                     \
        if (kind == PVV_MASK_U8) FORM(unsigned char, __VA_ARGS__);           \
        else if (kind == PVV_MASK_I32) FORM(int, __VA_ARGS__);               \
        else FORM(long long, __VA_ARGS__);                                   \
    } while (0)
#define TRAIN_KPT_VEC(T, f, kpt, vec, ...)                         \
    do {                                                           \
        if (kpt && vec) f<true, true, T>(__VA_ARGS__);             \
        else if (kpt) f<true, false, T>(__VA_ARGS__);              \
        else if (vec) f<false, true, T>(__VA_ARGS__);              \
        else f<false, false, T>(__VA_ARGS__);                      \
    } while (0)
#define TRAIN_VEC(T, f, vec, ...)                                  \
    do {                                                           \
        if (vec) f<true, T>(__VA_ARGS__);                          \
        else f<false, T>(__VA_ARGS__);                             \
    } while (0)

template <bool VEC, typename MaskT>
void train_launch_target(const TrainShape &s, const void *mask, const void *kpt, int kpt_is_f64, float *out, hipStream_t st)
{
    hipLaunchKernelGGL((k_train_vertex_target<VEC, MaskT>), dim3(s.tiles, s.B), dim3(kBlock), 0, st, s, (const MaskT *)mask, kpt, kpt_is_f64, out);
}

}  // namespace

PVV_EXPORT int pvv_vertex_target(const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64, int B, int K, int H, int W,
                                 float *d_out, void *stream)
{
    TrainShape s;
    if (int e = train_shape(s, B, K, 1, H, W)) return e;
    if (!d_mask || !d_kpt_2d || !d_out) return fail(PVV_E_ARG, "train: NULL device pointer");
    if (int e = train_mask_kind(mask_kind)) return e;
    const bool vec = s.HW % 4 == 0 && train_aligned(d_mask, 0) && train_aligned(d_out, 0);
    TRAIN_DISPATCH_VEC(train_launch_target, vec, mask_kind, s, d_mask, d_kpt_2d, kpt_is_f64, d_out, (hipStream_t)stream);
    return check_launch("k_train_vertex_target");
}

PVV_EXPORT size_t pvv_pvnet_loss_workspace_bytes(int B, int H, int W)
{
    TrainShape s;
    if (train_shape(s, B, 1, 1, H, W)) return 0;
    return train_layout(B, s.tiles).total;
}

PVV_EXPORT int pvv_pvnet_loss_forward(const float *d_vertex_pred, long long vp_image_stride, const float *d_seg_pred,
                                      long long sp_image_stride, const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64,
                                      const float *d_target, long long tg_image_stride, int B, int K, int C, int H, int W, void *workspace,
                                      size_t workspace_bytes, float *d_out_losses, void *d_out_state, void *stream)
{
    TrainShape s;
    if (int e = train_shape(s, B, K, C, H, W)) return e;
    const TrainArgs a = {d_vertex_pred, d_seg_pred, d_mask, d_kpt_2d, mask_kind, kpt_is_f64, d_target};
    bool vec = false;
    if (int e = train_inputs(s, a, vp_image_stride, sp_image_stride, tg_image_stride, vec)) return e;
    if (!d_out_losses) return fail(PVV_E_ARG, "train: NULL device pointer");
    if (int e = loss_state(d_out_state, "train")) return e;
    const LossLayout L = train_layout(B, s.tiles);
    if (int e = train_ws(workspace, workspace_bytes, L.total)) return e;
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    double *part = (double *)(ws + L.part), *img = (double *)(ws + L.img);
    long long *cnt = (long long *)(ws + L.cnt), *imgcnt = (long long *)(ws + L.imgcnt);
    const bool kpt = d_kpt_2d != nullptr;
    TRAIN_DISPATCH(train_launch_tiles, kpt, vec, mask_kind, s, a, part, cnt, st);
    if (int e = check_launch("k_train_loss_tiles")) return e;
    hipLaunchKernelGGL(k_train_loss_images, dim3(B), dim3(kBlock), 0, st, s.tiles, (const double *)part, (const long long *)cnt, img, imgcnt);
    if (int e = check_launch("k_train_loss_images")) return e;
    hipLaunchKernelGGL(k_train_loss_final, dim3(1), dim3(64), 0, st, B, K, (double)B * (double)s.HW, (const double *)img,
                       (const long long *)imgcnt, d_out_losses, (long long *)d_out_state);
    return check_launch("k_train_loss_final");
}

PVV_EXPORT int pvv_pvnet_loss_backward(const float *d_vertex_pred, long long vp_image_stride, const float *d_seg_pred,
                                       long long sp_image_stride, const void *d_mask, int mask_kind, const void *d_kpt_2d, int kpt_is_f64,
                                       const float *d_target, long long tg_image_stride, int B, int K, int C, int H, int W,
                                       const void *d_out_state, const float *d_grad_losses, float *d_grad_vertex, float *d_grad_seg,
                                       void *stream)
{
    TrainShape s;
    if (int e = train_shape(s, B, K, C, H, W)) return e;
    const TrainArgs a = {d_vertex_pred, d_seg_pred, d_mask, d_kpt_2d, mask_kind, kpt_is_f64, d_target};
    bool vec = false;
    if (int e = train_inputs(s, a, vp_image_stride, sp_image_stride, tg_image_stride, vec)) return e;
    if (!d_grad_losses || !d_grad_vertex || !d_grad_seg) return fail(PVV_E_ARG, "train: NULL device pointer");
    if (int e = loss_state(d_out_state, "train")) return e;
    vec = vec && train_aligned(d_grad_vertex, 0) && train_aligned(d_grad_seg, 0);
    const bool kpt = d_kpt_2d != nullptr;
    TRAIN_DISPATCH(train_launch_backward, kpt, vec, mask_kind, s, a, (const long long *)d_out_state, d_grad_losses, d_grad_vertex, d_grad_seg,
                   (hipStream_t)stream);
    return check_launch("k_train_loss_backward");
}
