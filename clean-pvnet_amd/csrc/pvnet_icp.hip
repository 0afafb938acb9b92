// pvnet_icp.hip -- one stage of the ICP pose refinement for a whole batch on the device, native HIP for gfx950
// (include/pvnet_icp.h has the arithmetic contract and the reference lines each pass replaces).
//
// Front passes, streaming over the P images (grid (tile chunks, P) unless stated):
//   k_syn_tiles   the synthetic cloud of the render: per tile of 256 pixels the tree-reduced coordinate sums and the count;
//                 the pixels of the mask that equal 1 are counted with an integer atomic.
//   k_syn_scan    one group per pose: the tile counts scanned, the tile sums added in ascending order, the centroid.
//   k_syn_max     the largest squared distance from the centroid: an unsigned atomicMax on the bits of a non-negative double.
//   k_real_tiles  the radius filter of the sensor cloud, per-tile counts.
//   k_plan        one group per pose: the real tile counts scanned, n, the status of a pose that stays unchanged.
//   k_select      grid (samples / 4, 2 clouds, P), a wave per sample: the tile by a binary search over the scanned counts,
//                 the pixel by a ballot rank inside the tile.  No full cloud is ever written.
// The loop is a launch chain: max_iterations times
//   k_search      grid (query tiles, destination slabs, P): a slab of 256 destination points in LDS, one source point per
//                 lane in registers, the partial (d2, index) of every (slab, query);
//   k_fit         one group per pose: partials combined in slab order, the fixed-order sums, the rotation on one lane, the
//                 source updated, the convergence test; on the last round of a pose the final fit and the output.
// A per-pose `done` word makes every later launch of that pose return at once.  No group waits for another.
//
// Index bounds: pixel < H*W and tile < ntiles by the grid tails; pose p < P by the grid; a sample k < n <= n_max; a sample
// index r is checked against [0, count) before it is used, so the binary search ends on a tile < ntiles and the rank is met
// inside it; a neighbour index j < n because every slab holds only j < n; slab s < ceil(n / 256) <= S.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "pvnet_icp.h"

#pragma clang fp contract(off)

namespace {

#include "eval_common.hpp"

constexpr int kTilesPerBlock = 4;    // tiles of 256 pixels a block of a front pass walks
constexpr int kSweeps = 30;

struct State {                       // one per pose, zeroed on the stream at the start of a call
    double centroid[3];
    double prev;                     // the mean distance of the previous round
    unsigned long long maxd2;        // bits of the largest squared distance of the synthetic cloud from its centroid
    int n_syn, n_real, n, mask_px, bad, done, rounds, pad;
};

struct Layout {                      // offsets into the workspace, in bytes; every array is 16-byte aligned
    size_t state, tsum, csyn, creal, a0, src, dst, pd2, pidx, nn, total;
    int ntiles, slabs;
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

Layout make_layout(int P, int H, int W, int n_max)
{
    Layout L;
    L.ntiles = (int)(((size_t)H * W + kBlock - 1) / kBlock);
    L.slabs = ceil_div(n_max, kBlock);
    size_t o = 0;
    L.state = o; o = align16(o + (size_t)P * sizeof(State));
    L.tsum = o;  o = align16(o + (size_t)P * L.ntiles * 3 * sizeof(double));
    L.csyn = o;  o = align16(o + (size_t)P * (L.ntiles + 1) * sizeof(int));
    L.creal = o; o = align16(o + (size_t)P * (L.ntiles + 1) * sizeof(int));
    L.a0 = o;    o = align16(o + (size_t)P * 3 * n_max * sizeof(double));
    L.src = o;   o = align16(o + (size_t)P * 3 * n_max * sizeof(double));
    L.dst = o;   o = align16(o + (size_t)P * 3 * n_max * sizeof(double));
    L.pd2 = o;   o = align16(o + (size_t)P * L.slabs * n_max * sizeof(double));
    L.pidx = o;  o = align16(o + (size_t)P * L.slabs * n_max * sizeof(int));
    L.nn = o;    o = align16(o + (size_t)P * n_max * sizeof(int));
    L.total = o;
    return L;
}

struct Cam {
    double fx, cx, fy, cy;
};

__device__ Cam load_cam(const double *K)
{
    Cam c;
    c.fx = K[0];
    c.cx = K[2];
    c.fy = K[4];
    c.cy = K[5];
    return c;
}

template <int KIND>
__device__ double load_depth(const void *p, size_t i, double scale)
{
    if (KIND == PVI_DEPTH_U16) return (double)((const uint16_t *)p)[i] * scale;
    if (KIND == PVI_DEPTH_F32) return (double)((const float *)p)[i];
    return ((const double *)p)[i];
}

template <int MKIND>
__device__ bool mask_is_one(const void *m, size_t i)
{
    if (MKIND == PVI_MASK_NONE) return true;
    if (MKIND == PVI_MASK_U8) return ((const uint8_t *)m)[i] == 1;
    return ((const long long *)m)[i] == 1;
}

// x = ((u - cx)*z)/fx, y = ((v - cy)*z)/fy
__device__ void back_project(const Cam &c, int pix, int W, double z, double *x, double *y)
{
    const int v = pix / W, u = pix - v * W;
    *x = (((double)u - c.cx) * z) / c.fx;
    *y = (((double)v - c.cy) * z) / c.fy;
}

__device__ double dist2(double x, double y, double z, const double *c)
{
    const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// slot j += slot j + s for s = 128 ... 1, for K rows at once; the sums are in sh[k][0] afterwards
template <int K>
__device__ void tree(double (*sh)[kBlock])
{
    const int tid = threadIdx.x;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][tid] += sh[k][tid + s];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------- the front passes
template <int MKIND>
__global__ __launch_bounds__(kBlock) void k_syn_tiles(const float *__restrict__ render, const void *__restrict__ mask,
                                                      int per_mask, const double *__restrict__ K, int K_batched,
                                                      State *__restrict__ st, double *__restrict__ tsum, int *__restrict__ csyn,
                                                      int W, int HW, int ntiles)
{
    __shared__ double sh[3][kBlock];
    const int p = blockIdx.y, tid = threadIdx.x;
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    const float *img = render + (size_t)p * HW;
    const size_t m0 = (size_t)(p / per_mask) * HW;
    int ones = 0;
    for (int k = 0; k < kTilesPerBlock; ++k) {
        const int tile = blockIdx.x * kTilesPerBlock + k;
        if (tile >= ntiles) break;                          // block-uniform
        const int pix = tile * kBlock + tid;
        double x = 0.0, y = 0.0, z = 0.0;
        bool in = false;
        if (pix < HW) {
            z = (double)img[pix];
            in = z != 0.0;
            if (in) back_project(c, pix, W, z, &x, &y);
            if (MKIND != PVI_MASK_NONE && mask_is_one<MKIND>(mask, m0 + pix)) ++ones;
        }
        __syncthreads();
        sh[0][tid] = x;
        sh[1][tid] = y;
        sh[2][tid] = z;
        tree<3>(sh);
        const int cnt = __syncthreads_count(in ? 1 : 0);
        if (tid < 3) tsum[((size_t)p * ntiles + tile) * 3 + tid] = sh[tid][0];
        if (tid == 0) csyn[(size_t)p * (ntiles + 1) + tile] = cnt;
    }
    if (MKIND != PVI_MASK_NONE) {
        for (int o = 32; o > 0; o >>= 1) ones += __shfl_down(ones, o);
        if ((tid & 63) == 0 && ones) atomicAdd(&st[p].mask_px, ones);
    }
}

// Exclusive scan of cnt[0 .. m) in place, the total in cnt[m]; one block.  Returns the total to every thread.
__device__ int block_scan(int *__restrict__ cnt, int m, int *shi)
{
    const int tid = threadIdx.x;
    const int chunk = (m + kBlock - 1) / kBlock;
    const int lo = min(tid * chunk, m), hi = min(lo + chunk, m);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    __syncthreads();
    shi[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < kBlock; ++i) {
            const int v = shi[i];
            shi[i] = run;
            run += v;
        }
        shi[kBlock] = run;
    }
    __syncthreads();
    int run = shi[tid];
    for (int i = lo; i < hi; ++i) {
        const int v = cnt[i];
        cnt[i] = run;
        run += v;
    }
    const int total = shi[kBlock];
    if (tid == 0) cnt[m] = total;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kBlock) void k_syn_scan(State *__restrict__ st, const double *__restrict__ tsum,
                                                     int *__restrict__ csyn, int ntiles)
{
    __shared__ int shi[kBlock + 1];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n_syn = block_scan(csyn + (size_t)p * (ntiles + 1), ntiles, shi);
    if (tid < 3) {
        const double *t = tsum + (size_t)p * ntiles * 3 + tid;
        double s = 0.0;
        for (int i = 0; i < ntiles; ++i) s = s + t[(size_t)i * 3];
        st[p].centroid[tid] = s / (double)n_syn;
    }
    if (tid == 0) st[p].n_syn = n_syn;
}

__global__ __launch_bounds__(kBlock) void k_syn_max(const float *__restrict__ render, const double *__restrict__ K,
                                                    int K_batched, State *__restrict__ st, int W, int HW, int ntiles)
{
    const int p = blockIdx.y, tid = threadIdx.x;
    if (st[p].n_syn == 0) return;
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    const double cen[3] = {st[p].centroid[0], st[p].centroid[1], st[p].centroid[2]};
    const float *img = render + (size_t)p * HW;
    unsigned long long best = 0;
    for (int k = 0; k < kTilesPerBlock; ++k) {
        const int pix = (blockIdx.x * kTilesPerBlock + k) * kBlock + tid;
        if (pix >= HW) break;
        const double z = (double)img[pix];
        if (z == 0.0) continue;
        double x, y;
        back_project(c, pix, W, z, &x, &y);
        const double d2 = dist2(x, y, z, cen);
        if (d2 >= 0.0) best = max(best, (unsigned long long)__double_as_longlong(d2));    // not for NaN
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_down((long long)best, o));
    if ((tid & 63) == 0 && best) atomicMax(&st[p].maxd2, best);
}

template <int KIND, int MKIND>
__device__ bool real_kept(const void *sensor, size_t s0, const void *mask, size_t m0, int pix, int W, const Cam &c,
                          double depth_scale, const double *cen, double thr, double *x, double *y, double *z)
{
    if (!mask_is_one<MKIND>(mask, m0 + pix)) return false;
    *z = load_depth<KIND>(sensor, s0 + pix, depth_scale);
    if (!(*z != 0.0)) return false;
    back_project(c, pix, W, *z, x, y);
    return sqrt(dist2(*x, *y, *z, cen)) < thr;
}

template <int KIND, int MKIND>
__global__ __launch_bounds__(kBlock) void k_real_tiles(const void *__restrict__ sensor, double depth_scale, int per_image,
                                                       const void *__restrict__ mask, int per_mask,
                                                       const double *__restrict__ K, int K_batched, double factor,
                                                       const State *__restrict__ st, int *__restrict__ creal, int W, int HW,
                                                       int ntiles)
{
    const int p = blockIdx.y, tid = threadIdx.x;
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    const double cen[3] = {st[p].centroid[0], st[p].centroid[1], st[p].centroid[2]};
    const double thr = factor * sqrt(__longlong_as_double((long long)st[p].maxd2));
    const bool any = st[p].n_syn > 0;
    const size_t s0 = (size_t)(p / per_image) * HW, m0 = (size_t)(p / per_mask) * HW;
    for (int k = 0; k < kTilesPerBlock; ++k) {
        const int tile = blockIdx.x * kTilesPerBlock + k;
        if (tile >= ntiles) break;                          // block-uniform
        const int pix = tile * kBlock + tid;
        double x, y, z;
        const bool kept = any && pix < HW && real_kept<KIND, MKIND>(sensor, s0, mask, m0, pix, W, c, depth_scale, cen, thr, &x, &y, &z);
        const int cnt = __syncthreads_count(kept ? 1 : 0);
        if (tid == 0) creal[(size_t)p * (ntiles + 1) + tile] = cnt;
    }
}

__device__ void write_unchanged(const double *__restrict__ pose, double *__restrict__ out, int32_t *__restrict__ info,
                                const State &s, int status, int n)
{
    for (int i = 0; i < 12; ++i) out[i] = pose[i];
    info[PVI_STATUS] = status;
    info[PVI_N_SYN] = s.n_syn;
    info[PVI_N_REAL] = s.n_real;
    info[PVI_N] = n;
    info[PVI_ROUNDS] = s.rounds;
}

__global__ __launch_bounds__(kBlock) void k_plan(State *__restrict__ st, int *__restrict__ creal, const double *__restrict__ pose,
                                                 double *__restrict__ pose_out, int32_t *__restrict__ info, int ntiles, int n_max,
                                                 int has_mask, int min_mask_pixels)
{
    __shared__ int shi[kBlock + 1];
    const int p = blockIdx.x;
    const int n_real = block_scan(creal + (size_t)p * (ntiles + 1), ntiles, shi);
    if (threadIdx.x != 0) return;
    State &s = st[p];
    const double *T = pose + (size_t)p * 12;
    s.n_real = n_real;
    const int n = min(min(n_real, s.n_syn), n_max);
    s.n = n;
    int status = PVI_REFINED;
    if (!pose_finite(T) || !(T[11] > 0.0)) status = PVI_BAD_POSE;
    else if (has_mask && s.mask_px < min_mask_pixels) status = PVI_SMALL_MASK;
    else if (s.n_syn == 0) status = PVI_EMPTY_RENDER;
    else if ((double)n_real < (double)s.n_syn / 20.0) status = PVI_NOT_VISIBLE;
    if (status != PVI_REFINED) {
        write_unchanged(T, pose_out + (size_t)p * 12, info + (size_t)p * PVI_INFO_COLUMNS, s, status, 0);
        s.done = 1;
    }
}

// A wave per sample: the tile that holds rank r by a binary search over the exclusive prefix, the pixel by ballots.
template <int KIND, int MKIND>
__global__ __launch_bounds__(kBlock) void k_select(const float *__restrict__ render, const void *__restrict__ sensor,
                                                   double depth_scale, int per_image, const void *__restrict__ mask, int per_mask,
                                                   const double *__restrict__ K, int K_batched, double factor,
                                                   const int32_t *__restrict__ idx_syn, const int32_t *__restrict__ idx_real,
                                                   const long long *__restrict__ words, State *__restrict__ st,
                                                   const int *__restrict__ csyn, const int *__restrict__ creal,
                                                   double *__restrict__ a0, double *__restrict__ src, double *__restrict__ dst,
                                                   int W, int HW, int ntiles, int n_max)
{
    const int p = blockIdx.z, cloud = blockIdx.y, lane = threadIdx.x & 63;
    const int k = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);                   // wave-uniform
    const State &s = st[p];
    if (s.done || k >= s.n) return;
    const int count = cloud == 0 ? s.n_syn : s.n_real;
    long long r;
    if (idx_syn) r = (cloud == 0 ? idx_syn : idx_real)[(size_t)p * n_max + k];
    else r = (long long)((((unsigned long long)words[((size_t)p * 2 + cloud) * n_max + k] & 0xffffffffull) * (unsigned long long)count) >> 32);
    if (r < 0 || r >= count) {
        if (lane == 0) atomicOr(&st[p].bad, 1);
        return;
    }
    const int *pre = (cloud == 0 ? csyn : creal) + (size_t)p * (ntiles + 1);
    int lo = 0, hi = ntiles - 1;                            // the largest tile with pre[tile] <= r: pre[0] = 0 <= r < pre[ntiles]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= (int)r) lo = mid;
        else hi = mid - 1;
    }
    int rank = (int)r - pre[lo];
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    const double cen[3] = {s.centroid[0], s.centroid[1], s.centroid[2]};
    const double thr = factor * sqrt(__longlong_as_double((long long)s.maxd2));
    const float *img = render + (size_t)p * HW;
    const size_t s0 = (size_t)(p / per_image) * HW, m0 = (size_t)(p / per_mask) * HW;
    for (int q = 0; q < kBlock / 64; ++q) {
        const int pix = lo * kBlock + q * 64 + lane;
        double x = 0.0, y = 0.0, z = 0.0;
        bool in = false;
        if (pix < HW) {
            if (cloud == 0) {
                z = (double)img[pix];
                in = z != 0.0;
                if (in) back_project(c, pix, W, z, &x, &y);
            } else {
                in = real_kept<KIND, MKIND>(sensor, s0, mask, m0, pix, W, c, depth_scale, cen, thr, &x, &y, &z);
            }
        }
        const unsigned long long b = __ballot(in);
        const int cnt = __popcll(b);
        if (rank < cnt) {
            if (in && __popcll(b & ((1ull << lane) - 1ull)) == rank) {
                const size_t o = (size_t)p * 3 * n_max + k;
                if (cloud == 0) {
                    a0[o] = x; a0[o + n_max] = y; a0[o + 2 * (size_t)n_max] = z;
                    src[o] = x; src[o + n_max] = y; src[o + 2 * (size_t)n_max] = z;
                } else {
                    dst[o] = x; dst[o + n_max] = y; dst[o + 2 * (size_t)n_max] = z;
                }
            }
            return;
        }
        rank -= cnt;
    }
}

// -------------------------------------------------------------------------------------------------------------- the loop
__global__ __launch_bounds__(kBlock) void k_search(const State *__restrict__ st, const double *__restrict__ src,
                                                   const double *__restrict__ dst, double *__restrict__ pd2,
                                                   int *__restrict__ pidx, int n_max, int slabs)
{
    __shared__ double sx[kBlock], sy[kBlock], sz[kBlock];
    const int p = blockIdx.z, tid = threadIdx.x;
    const State &s = st[p];
    if (s.done || s.bad) return;
    const int n = s.n, q0 = blockIdx.x * kBlock, j0 = blockIdx.y * kBlock;
    if (q0 >= n || j0 >= n) return;
    const int cnt = min(kBlock, n - j0);
    const double *d = dst + (size_t)p * 3 * n_max;
    if (tid < cnt) {
        sx[tid] = d[j0 + tid];
        sy[tid] = d[(size_t)n_max + j0 + tid];
        sz[tid] = d[2 * (size_t)n_max + j0 + tid];
    }
    __syncthreads();
    const int i = q0 + tid;
    if (i >= n) return;
    const double *a = src + (size_t)p * 3 * n_max;
    const double x = a[i], y = a[(size_t)n_max + i], z = a[2 * (size_t)n_max + i];
    double best = HUGE_VAL;
    int bj = 0;
    for (int j = 0; j < cnt; ++j) {
        const double ex = x - sx[j], ey = y - sy[j], ez = z - sz[j];
        const double d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 < best) {
            best = d2;
            bj = j;
        }
    }
    const size_t o = ((size_t)p * slabs + blockIdx.y) * n_max + i;
    pd2[o] = best;
    pidx[o] = j0 + bj;
}

// The rotation of the header from S (row-major 3x3): Horn's N, cyclic Jacobi, the quaternion's matrix.  One lane.
#define PVI_ROTATE(P_, Q_)                                                                                     \
    {                                                                                                          \
        const double g = fabs(N[P_][Q_]);                                                                      \
        if (g == 0.0 || (fabs(N[P_][P_]) + g == fabs(N[P_][P_]) && fabs(N[Q_][Q_]) + g == fabs(N[Q_][Q_]))) {  \
            N[P_][Q_] = 0.0;                                                                                   \
            N[Q_][P_] = 0.0;                                                                                   \
        } else {                                                                                               \
            rotated = true;                                                                                    \
            const double apq = N[P_][Q_];                                                                      \
            const double theta = (N[Q_][Q_] - N[P_][P_]) / (2.0 * apq);                                        \
            const double r = sqrt(theta * theta + 1.0);                                                        \
            double tt = 1.0 / (fabs(theta) + r);                                                               \
            if (theta < 0.0) tt = -tt;                                                                         \
            const double c = 1.0 / sqrt(tt * tt + 1.0);                                                        \
            const double s = tt * c;                                                                           \
            N[P_][P_] = N[P_][P_] - tt * apq;                                                                  \
            N[Q_][Q_] = N[Q_][Q_] + tt * apq;                                                                  \
            N[P_][Q_] = 0.0;                                                                                   \
            N[Q_][P_] = 0.0;                                                                                   \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                    \
                if (k != P_ && k != Q_) {                                                                      \
                    const double akp = N[k][P_], akq = N[k][Q_];                                               \
                    N[k][P_] = c * akp - s * akq;                                                              \
                    N[k][Q_] = s * akp + c * akq;                                                              \
                    N[P_][k] = N[k][P_];                                                                       \
                    N[Q_][k] = N[k][Q_];                                                                       \
                }                                                                                              \
            }                                                                                                  \
            _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                    \
                const double vkp = V[k][P_], vkq = V[k][Q_];                                                   \
                V[k][P_] = c * vkp - s * vkq;                                                                  \
                V[k][Q_] = s * vkp + c * vkq;                                                                  \
            }                                                                                                  \
        }                                                                                                      \
    }

__device__ void rotation_of(const double *S, double *R)
{
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[4][4], V[4][4];
    N[0][0] = (Sxx + Syy) + Szz;
    N[1][1] = (Sxx - Syy) - Szz;
    N[2][2] = (Syy - Sxx) - Szz;
    N[3][3] = (Szz - Sxx) - Syy;
    N[0][1] = N[1][0] = Syz - Szy;
    N[0][2] = N[2][0] = Szx - Sxz;
    N[0][3] = N[3][0] = Sxy - Syx;
    N[1][2] = N[2][1] = Sxy + Syx;
    N[1][3] = N[3][1] = Szx + Sxz;
    N[2][3] = N[3][2] = Syz + Szy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        bool rotated = false;
        PVI_ROTATE(0, 1)
        PVI_ROTATE(0, 2)
        PVI_ROTATE(0, 3)
        PVI_ROTATE(1, 2)
        PVI_ROTATE(1, 3)
        PVI_ROTATE(2, 3)
        if (!rotated) break;
    }
    double lam = N[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (N[j][j] > lam) {
            lam = N[j][j];
            w = V[0][j]; x = V[1][j]; y = V[2][j]; z = V[3][j];
        }
    }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// fit(a_i -> b_nn(i)) of the header (nn == nullptr: b_i).  a, b: SoA with stride n_max.  The twelve values [R | t] land in
// T (shared memory, R row-major then t); every thread may read them after the call.  sh[6][.] on entry holds an extra addend
// row for the first tree (the distances of a round), whose sum is returned.
__device__ double fit(const double *__restrict__ a, const double *__restrict__ b, const int *__restrict__ nn, int n, int n_max,
                      int flags, double (*sh)[kBlock], double *T)
{
    const int tid = threadIdx.x;
    const size_t m = (size_t)n_max;
    double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kBlock) {
        const int j = nn ? nn[i] : i;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ca[k] += a[k * m + i];
            cb[k] += b[k * m + j];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sh[k][tid] = ca[k];
        sh[3 + k][tid] = cb[k];
    }
    tree<7>(sh);
    const double dn = (double)n, extra = sh[6][0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ca[k] = sh[k][0] / dn;
        cb[k] = sh[3 + k][0] / dn;
    }
    __syncthreads();
    const bool identity = (flags & PVI_DEPTH_ONLY) && !(flags & PVI_NO_DEPTH);
    if (identity) {
        if (tid == 0) {
            for (int k = 0; k < 9; ++k) T[k] = (k % 4 == 0) ? 1.0 : 0.0;
            for (int k = 0; k < 3; ++k) T[9 + k] = cb[k] - ca[k];
        }
    } else {
        double h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = 0.0;
        for (int i = tid; i < n; i += kBlock) {
            const int j = nn ? nn[i] : i;
            double aa[3], bb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                aa[k] = a[k * m + i] - ca[k];
                bb[k] = b[k * m + j] - cb[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l) h[k * 3 + l] += aa[k] * bb[l];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) sh[k][tid] = h[k];
        tree<9>(sh);
        if (tid == 0) {
            double S[9], R[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) S[k] = sh[k][0];
            rotation_of(S, R);
#pragma unroll
            for (int k = 0; k < 9; ++k) T[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) T[9 + k] = cb[k] - ((R[k * 3] * ca[0] + R[k * 3 + 1] * ca[1]) + R[k * 3 + 2] * ca[2]);
            if ((flags & PVI_NO_DEPTH) && !(flags & PVI_DEPTH_ONLY)) T[11] = 0.0;
        }
    }
    __syncthreads();
    return extra;
}

__global__ __launch_bounds__(kBlock) void k_fit(State *__restrict__ st, const double *__restrict__ a0, double *__restrict__ src,
                                                const double *__restrict__ dst, const double *__restrict__ pd2,
                                                const int *__restrict__ pidx, int *__restrict__ nn, const double *__restrict__ pose,
                                                double *__restrict__ pose_out, int32_t *__restrict__ info, int n_max, int slabs,
                                                int flags, double tolerance, double cos_limit, int last)
{
    __shared__ double sh[9][kBlock];
    __shared__ double T[12];
    __shared__ int stop;
    const int p = blockIdx.x, tid = threadIdx.x;
    State &s = st[p];
    if (s.done) return;                                     // block-uniform: written only by thread 0 of this pose's group
    const double *Tin = pose + (size_t)p * 12;
    double *Tout = pose_out + (size_t)p * 12;
    int32_t *inf = info + (size_t)p * PVI_INFO_COLUMNS;
    if (s.bad) {
        if (tid == 0) {
            write_unchanged(Tin, Tout, inf, s, PVI_BAD_INDEX, s.n);
            s.done = 1;
        }
        return;
    }
    const int n = s.n;
    const size_t m = (size_t)n_max;
    const double *A0 = a0 + (size_t)p * 3 * m, *D = dst + (size_t)p * 3 * m;
    double *A = src + (size_t)p * 3 * m;
    int *NN = nn + (size_t)p * m;
    const int used = (n + kBlock - 1) / kBlock;             // slabs that hold a destination point: used <= slabs
    double dsum = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        double best = pd2[((size_t)p * slabs) * m + i];
        int bj = pidx[((size_t)p * slabs) * m + i];
        for (int q = 1; q < used; ++q) {
            const double d2 = pd2[((size_t)p * slabs + q) * m + i];
            if (d2 < best) {                                // slabs ascend: the lowest index keeps a tie
                best = d2;
                bj = pidx[((size_t)p * slabs + q) * m + i];
            }
        }
        NN[i] = bj;
        dsum += sqrt(best);
    }
    sh[6][tid] = dsum;
    const double total = fit(A, D, NN, n, n_max, flags, sh, T);
    for (int i = tid; i < n; i += kBlock) {
        const double x = A[i], y = A[m + i], z = A[2 * m + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) A[k * m + i] = ((T[k * 3] * x + T[k * 3 + 1] * y) + T[k * 3 + 2] * z) + T[9 + k];
    }
    if (tid == 0) {
        const double mean = total / (double)n;
        s.rounds += 1;
        stop = (fabs(s.prev - mean) < tolerance || last) ? 1 : 0;
        s.prev = mean;
    }
    __syncthreads();                                        // also orders the source update before the final fit reads it
    if (!stop) return;
    sh[6][tid] = 0.0;
    fit(A0, A, nullptr, n, n_max, flags, sh, T);
    if (tid != 0) return;
    s.done = 1;
    if ((flags & PVI_NO_DEPTH) && (((T[0] + T[4]) + T[8]) - 1.0) / 2.0 < cos_limit) {
        write_unchanged(Tin, Tout, inf, s, PVI_ROTATION_LIMIT, n);
        return;
    }
    const bool identity = (flags & PVI_DEPTH_ONLY) && !(flags & PVI_NO_DEPTH);
    for (int k = 0; k < 3; ++k) {
        for (int l = 0; l < 3; ++l)
            Tout[k * 4 + l] = identity ? Tin[k * 4 + l]
                                       : (T[k * 3] * Tin[l] + T[k * 3 + 1] * Tin[4 + l]) + T[k * 3 + 2] * Tin[8 + l];
        Tout[k * 4 + 3] = ((T[k * 3] * Tin[3] + T[k * 3 + 1] * Tin[7]) + T[k * 3 + 2] * Tin[11]) + T[9 + k];
    }
    inf[PVI_STATUS] = PVI_REFINED;
    inf[PVI_N_SYN] = s.n_syn;
    inf[PVI_N_REAL] = s.n_real;
    inf[PVI_N] = n;
    inf[PVI_ROUNDS] = s.rounds;
}

struct Args {
    const float *render;
    const void *sensor, *mask;
    double depth_scale, factor;
    int per_image, per_mask, K_batched, W, HW, ntiles, n_max, P;
    const double *K;
    const int32_t *idx_syn, *idx_real;
    const long long *words;
    State *st;
    double *tsum, *a0, *src, *dst;
    int *csyn, *creal;
    hipStream_t stream;
};

template <int MKIND>
void launch_syn_tiles(const Args &a)
{
    hipLaunchKernelGGL((k_syn_tiles<MKIND>), dim3(ceil_div(a.ntiles, kTilesPerBlock), a.P), dim3(kBlock), 0, a.stream, a.render,
                       a.mask, a.per_mask, a.K, a.K_batched, a.st, a.tsum, a.csyn, a.W, a.HW, a.ntiles);
}

template <int KIND, int MKIND>
void launch_real(const Args &a, bool select)
{
    if (!select)
        hipLaunchKernelGGL((k_real_tiles<KIND, MKIND>), dim3(ceil_div(a.ntiles, kTilesPerBlock), a.P), dim3(kBlock), 0, a.stream,
                           a.sensor, a.depth_scale, a.per_image, a.mask, a.per_mask, a.K, a.K_batched, a.factor, a.st, a.creal,
                           a.W, a.HW, a.ntiles);
    else
        hipLaunchKernelGGL((k_select<KIND, MKIND>), dim3(ceil_div(a.n_max, kBlock / 64), 2, a.P), dim3(kBlock), 0, a.stream,
                           a.render, a.sensor, a.depth_scale, a.per_image, a.mask, a.per_mask, a.K, a.K_batched, a.factor,
                           a.idx_syn, a.idx_real, a.words, a.st, a.csyn, a.creal, a.a0, a.src, a.dst, a.W, a.HW, a.ntiles,
                           a.n_max);
}

template <int KIND>
void launch_real_m(const Args &a, int mask_kind, bool select)
{
    if (mask_kind == PVI_MASK_NONE) launch_real<KIND, PVI_MASK_NONE>(a, select);
    else if (mask_kind == PVI_MASK_U8) launch_real<KIND, PVI_MASK_U8>(a, select);
    else launch_real<KIND, PVI_MASK_I64>(a, select);
}

void launch_real_km(const Args &a, int sensor_kind, int mask_kind, bool select)
{
    if (sensor_kind == PVI_DEPTH_U16) launch_real_m<PVI_DEPTH_U16>(a, mask_kind, select);
    else if (sensor_kind == PVI_DEPTH_F32) launch_real_m<PVI_DEPTH_F32>(a, mask_kind, select);
    else launch_real_m<PVI_DEPTH_F64>(a, mask_kind, select);
}

bool sizes_ok(int P, int H, int W, int n_max)
{
    return P >= 0 && P <= 65535 && H > 0 && H <= PVI_MAX_SIDE && W > 0 && W <= PVI_MAX_SIDE && n_max > 0 &&
           n_max <= PVI_MAX_SAMPLES && (long long)H * W <= INT_MAX - 4 * kBlock;
}

}  // namespace

PVE_EXPORT size_t pvi_workspace_bytes(int P, int H, int W, int n_max)
{
    if (P <= 0 || !sizes_ok(P, H, W, n_max)) return 0;
    return make_layout(P, H, W, n_max).total;
}

PVE_EXPORT int pvi_refine_batched(const float *d_render, const void *d_sensor, int sensor_kind, double depth_scale, int per_image,
                                  const void *d_mask, int mask_kind, int per_mask, int min_mask_pixels, const double *d_pose,
                                  const double *d_K, int K_batched, const int32_t *d_idx_syn, const int32_t *d_idx_real,
                                  const long long *d_words, int flags, double max_mean_dist_factor, int n_max, int max_iterations,
                                  double tolerance, double cos_limit, double *d_pose_out, int32_t *d_info, void *d_workspace,
                                  int P, int H, int W, void *stream)
{
    if (!sizes_ok(P, H, W, n_max)) return -1;
    if (sensor_kind < PVI_DEPTH_U16 || sensor_kind > PVI_DEPTH_F64 || mask_kind < PVI_MASK_NONE || mask_kind > PVI_MASK_I64) return -1;
    if (max_iterations < 1 || max_iterations > 100000 || per_image < 1 || per_mask < 1) return -1;
    if ((flags & ~(PVI_DEPTH_ONLY | PVI_NO_DEPTH)) != 0) return -1;
    if (!(tolerance >= 0.0) || !(max_mean_dist_factor >= 0.0) || cos_limit != cos_limit) return -1;     // also refuses NaN
    if (P == 0) return 0;
    if (P % per_image != 0 || P % per_mask != 0) return -1;
    if (!d_render || !d_sensor || !d_pose || !d_K || !d_pose_out || !d_info || !d_workspace) return -1;
    if ((mask_kind != PVI_MASK_NONE) != (d_mask != nullptr)) return -1;
    if ((d_idx_syn != nullptr) != (d_idx_real != nullptr)) return -1;
    if (!d_idx_syn && !d_words) return -1;
    if (((uintptr_t)d_workspace & 15) != 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = make_layout(P, H, W, n_max);
    char *ws = (char *)d_workspace;
    Args a;
    a.render = d_render; a.sensor = d_sensor; a.mask = d_mask;
    a.depth_scale = depth_scale; a.factor = max_mean_dist_factor;
    a.per_image = per_image; a.per_mask = per_mask; a.K_batched = K_batched; a.W = W; a.HW = H * W; a.ntiles = L.ntiles;
    a.n_max = n_max; a.P = P; a.K = d_K; a.idx_syn = d_idx_syn; a.idx_real = d_idx_real; a.words = d_words;
    a.st = (State *)(ws + L.state); a.tsum = (double *)(ws + L.tsum); a.a0 = (double *)(ws + L.a0);
    a.src = (double *)(ws + L.src); a.dst = (double *)(ws + L.dst); a.csyn = (int *)(ws + L.csyn);
    a.creal = (int *)(ws + L.creal); a.stream = st;
    double *pd2 = (double *)(ws + L.pd2);
    int *pidx = (int *)(ws + L.pidx), *nn = (int *)(ws + L.nn);
    hipError_t e = hipMemsetAsync(a.st, 0, (size_t)P * sizeof(State), st);
    if (e != hipSuccess) return (int)e;
    if (mask_kind == PVI_MASK_NONE) launch_syn_tiles<PVI_MASK_NONE>(a);
    else if (mask_kind == PVI_MASK_U8) launch_syn_tiles<PVI_MASK_U8>(a);
    else launch_syn_tiles<PVI_MASK_I64>(a);
    hipLaunchKernelGGL(k_syn_scan, dim3(P), dim3(kBlock), 0, st, a.st, a.tsum, a.csyn, L.ntiles);
    hipLaunchKernelGGL(k_syn_max, dim3(ceil_div(L.ntiles, kTilesPerBlock), P), dim3(kBlock), 0, st, d_render, d_K, K_batched, a.st,
                       W, a.HW, L.ntiles);
    launch_real_km(a, sensor_kind, mask_kind, false);
    hipLaunchKernelGGL(k_plan, dim3(P), dim3(kBlock), 0, st, a.st, a.creal, d_pose, d_pose_out, d_info, L.ntiles, n_max,
                       mask_kind != PVI_MASK_NONE ? 1 : 0, min_mask_pixels);
    launch_real_km(a, sensor_kind, mask_kind, true);
    const dim3 sgrid(L.slabs, L.slabs, P);
    for (int it = 0; it < max_iterations; ++it) {
        hipLaunchKernelGGL(k_search, sgrid, dim3(kBlock), 0, st, a.st, a.src, a.dst, pd2, pidx, n_max, L.slabs);
        hipLaunchKernelGGL(k_fit, dim3(P), dim3(kBlock), 0, st, a.st, a.a0, a.src, a.dst, pd2, pidx, nn, d_pose, d_pose_out, d_info,
                           n_max, L.slabs, flags, tolerance, cos_limit, it == max_iterations - 1 ? 1 : 0);
    }
    return (int)hipGetLastError();
}
