// pvnet_metrics.hip -- clean-pvnet's pose scores for a whole batch on the device, native HIP for gfx950
// (include/pvnet_metrics.h has the arithmetic contract and the reference lines each pass replaces).
//
//   k_transform     grid (point tiles, B): both clouds in binary64, the per-point ADD and projection distances reduced to one
//                   partial sum per tile, the float32 clouds (padded to 16 bytes a point) for the symmetric images.
//   k_adds_search   grid (query tiles, slabs, B): the nearest predicted point of every ground-truth point inside one slab of
//                   the predicted cloud; 4 queries per lane in registers, the slab staged through LDS and read as a broadcast
//                   ds_read_b128.  One 64-bit key (float bits of the distance << 32 | index) per (slab, query).
//   k_adds_merge    grid (point tiles, B): the minimum key over the slabs (unsigned order = distance, then index = "first
//                   minimum wins"), the index, the binary64 ADD-S distance, one partial sum per tile.
//   k_finish        one thread per image: the tile sums in ascending order, the means, translation and angle.
//   k_mask_iou      grid (chunks, B): integer sums of mask_pred & mask_gt and mask_pred | mask_gt.
//
// Every index is bounded by p < N (points), b < B (grid) and s < S (grid); the workspace offsets are those of `layout`.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "pvnet_metrics.h"

#pragma clang fp contract(off)

namespace {

#include "eval_common.hpp"

constexpr int kQ = 4;              // queries per lane in the search
constexpr int kQTile = kBlock * kQ;
constexpr int kRefTile = 1024;     // predicted points staged in LDS per step (16 KB)
constexpr int kMinSlab = 64;       // the automatic slab count leaves at least this many points in a slab
constexpr int kTargetBlocks = 3072;   // 12 blocks on each of the 256 compute units (measured: DESIGN.md section 9)
constexpr int kMaskPerThread = 8;

struct Layout {
    size_t part, pred4, targ4, keys, total;
};

int auto_slabs(int B, int N)
{
    if (B <= 0 || N <= 0) return 1;
    const long long blocks = (long long)ceil_div(N, kQTile) * B;
    long long S = (kTargetBlocks + blocks - 1) / blocks;
    const long long most = N / kMinSlab > 1 ? N / kMinSlab : 1;
    if (S > most) S = most;
    return S < 1 ? 1 : (int)S;
}

int pick_slabs(int B, int N, int slabs)
{
    if (slabs <= 0) return auto_slabs(B, N);
    return slabs > N ? N : slabs;
}

Layout layout(int B, int N, int S)
{
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t nt = (size_t)ceil_div(N, kBlock);
    Layout l;
    l.part = 0;
    l.pred4 = up((size_t)B * nt * 3 * sizeof(double));
    l.targ4 = l.pred4 + (size_t)B * N * sizeof(float4);
    l.keys = l.targ4 + (size_t)B * N * sizeof(float4);
    l.total = l.keys + (size_t)B * S * N * sizeof(unsigned long long);
    return l;
}

// x[i] = ((m0*R[i,0] + m1*R[i,1]) + m2*R[i,2]) + t[i]
__device__ void transform(const double *P, const float *m, double *x)
{
    const double m0 = (double)m[0], m1 = (double)m[1], m2 = (double)m[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = ((m0 * P[i * 4] + m1 * P[i * 4 + 1]) + m2 * P[i * 4 + 2]) + P[i * 4 + 3];
}

__device__ double dist3(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ void project(const double *Kc, const double *x, double *uv)
{
    double u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = (x[0] * Kc[i * 3] + x[1] * Kc[i * 3 + 1]) + x[2] * Kc[i * 3 + 2];
    uv[0] = u[0] / u[2];
    uv[1] = u[1] / u[2];
}

__global__ __launch_bounds__(kBlock) void k_transform(const double *__restrict__ pose_pred, const double *__restrict__ pose_gt,
                                                      const float *__restrict__ model, const double *__restrict__ K,
                                                      const uint8_t *__restrict__ sym, double *__restrict__ part,
                                                      float4 *__restrict__ pred4, float4 *__restrict__ targ4, int N, int nt,
                                                      int K_batched)
{
    __shared__ double sh[kBlock];
    const int b = blockIdx.y, t = blockIdx.x;
    const int p = t * kBlock + threadIdx.x;
    const double *P = pose_pred + (size_t)b * 12, *G = pose_gt + (size_t)b * 12;
    const double *Kc = K + (K_batched ? (size_t)b * 9 : 0);
    double d_add = 0.0, d_proj = 0.0;
    if (p < N) {
        double xp[3], xg[3], up[2], ug[2];
        transform(P, model + (size_t)p * 3, xp);
        transform(G, model + (size_t)p * 3, xg);
        d_add = dist3(xp, xg);
        project(Kc, xp, up);
        project(Kc, xg, ug);
        const double du = up[0] - ug[0], dv = up[1] - ug[1];
        d_proj = sqrt(du * du + dv * dv);
        if (sym && sym[b]) {
            pred4[(size_t)b * N + p] = make_float4((float)xp[0], (float)xp[1], (float)xp[2], 0.f);
            targ4[(size_t)b * N + p] = make_float4((float)xg[0], (float)xg[1], (float)xg[2], 0.f);
        }
    }
    const double s_add = block_sum(d_add, sh);
    const double s_proj = block_sum(d_proj, sh);
    if (threadIdx.x == 0) {
        part[((size_t)b * nt + t) * 3 + 0] = s_add;
        part[((size_t)b * nt + t) * 3 + 1] = s_proj;
    }
}

// One slab [s*L, min(N, (s+1)*L)) of the predicted cloud against kQTile ground-truth points.  The evaluation is the one of
// k_find_nearest (pvnet_nn.hip): (dx*dx + dy*dy) + dz*dz in binary32, uncontracted, strict `<` in ascending index order.
__global__ __launch_bounds__(kBlock) void k_adds_search(const float4 *__restrict__ pred4, const float4 *__restrict__ targ4,
                                                        const uint8_t *__restrict__ sym, unsigned long long *__restrict__ keys,
                                                        int N, int S, int L)
{
    __shared__ float4 tile[kRefTile];
    const int b = blockIdx.z, s = blockIdx.y;
    if (!sym[b]) return;                                         // the same for the whole block
    const float4 *ref = pred4 + (size_t)b * N;
    const float4 *que = targ4 + (size_t)b * N;
    const int q0 = blockIdx.x * kQTile + threadIdx.x;
    float qx[kQ], qy[kQ], qz[kQ], mind[kQ];
    int mini[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int qi = q0 + k * kBlock;
        const float4 q = qi < N ? que[qi] : make_float4(0.f, 0.f, 0.f, 0.f);
        qx[k] = q.x; qy[k] = q.y; qz[k] = q.z;
        mind[k] = FLT_MAX;
        mini[k] = 0;
    }
    const int r0 = min(N, s * L), r1 = min(N, r0 + L);
    for (int t0 = r0; t0 < r1; t0 += kRefTile) {
        const int n = min(kRefTile, r1 - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kBlock) tile[i] = ref[t0 + i];
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const float4 r = tile[j];                            // every lane reads the same address: broadcast
            const int p1i = t0 + j;
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                const float dx = r.x - qx[k], dy = r.y - qy[k], dz = r.z - qz[k];
                const float dist = (dx * dx + dy * dy) + dz * dz;
                if (dist < mind[k]) { mind[k] = dist; mini[k] = p1i; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int qi = q0 + k * kBlock;
        if (qi < N)
            keys[((size_t)b * S + s) * N + qi] = ((unsigned long long)__float_as_uint(mind[k]) << 32) | (unsigned)mini[k];
    }
}

__global__ __launch_bounds__(kBlock) void k_adds_merge(const double *__restrict__ pose_pred, const double *__restrict__ pose_gt,
                                                       const float *__restrict__ model, const uint8_t *__restrict__ sym,
                                                       const unsigned long long *__restrict__ keys, double *__restrict__ part,
                                                       int32_t *__restrict__ adds_idx, int N, int nt, int S)
{
    __shared__ double sh[kBlock];
    const int b = blockIdx.y, t = blockIdx.x;
    const int p = t * kBlock + threadIdx.x;
    const double *P = pose_pred + (size_t)b * 12, *G = pose_gt + (size_t)b * 12;
    if (!(sym && sym[b]) || !pose_finite(P) || !pose_finite(G)) {   // the same for the whole block
        if (adds_idx && p < N) adds_idx[(size_t)b * N + p] = 0;
        return;
    }
    double d = 0.0;
    if (p < N) {
        const unsigned long long *kp = keys + ((size_t)b * S) * N + p;
        unsigned long long key = kp[0];
        int s = 1;
        for (; s + 8 <= S; s += 8) {                              // eight independent loads in flight, then their minimum
            unsigned long long k8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) k8[j] = kp[(size_t)(s + j) * N];
#pragma unroll
            for (int j = 0; j < 8; ++j) key = k8[j] < key ? k8[j] : key;
        }
        for (; s < S; ++s) {
            const unsigned long long k2 = kp[(size_t)s * N];
            key = k2 < key ? k2 : key;
        }
        int idx = (int)(unsigned)(key & 0xffffffffull);
        idx = idx < N ? idx : 0;                                 // a key is always a valid index; this keeps the gather in bounds
        if (adds_idx) adds_idx[(size_t)b * N + p] = idx;
        double xp[3], xg[3];
        transform(P, model + (size_t)idx * 3, xp);
        transform(G, model + (size_t)p * 3, xg);
        d = dist3(xp, xg);
    }
    const double s_adds = block_sum(d, sh);
    if (threadIdx.x == 0) part[((size_t)b * nt + t) * 3 + 2] = s_adds;
}

__global__ __launch_bounds__(64) void k_finish(const double *__restrict__ pose_pred, const double *__restrict__ pose_gt,
                                               const uint8_t *__restrict__ sym, const double *__restrict__ part,
                                               double *__restrict__ metrics, int B, int N, int nt)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *P = pose_pred + (size_t)b * 12, *G = pose_gt + (size_t)b * 12;
    double *out = metrics + (size_t)b * 5;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!pose_finite(P) || !pose_finite(G)) {
        for (int i = 0; i < 5; ++i) out[i] = nan;
        return;
    }
    const bool symb = sym && sym[b];
    double s_add = 0.0, s_proj = 0.0, s_adds = 0.0;
    const double *q = part + (size_t)b * nt * 3;
    int t = 0;
    for (; t + 8 <= nt; t += 8) {                                // ascending tile order; the loads of eight tiles in flight
        double v[24];
#pragma unroll
        for (int j = 0; j < 24; ++j) v[j] = (j % 3 == 2 && !symb) ? 0.0 : q[t * 3 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s_add += v[j * 3]; s_proj += v[j * 3 + 1]; s_adds += v[j * 3 + 2]; }
    }
    for (; t < nt; ++t) {
        s_add += q[t * 3];
        s_proj += q[t * 3 + 1];
        if (symb) s_adds += q[t * 3 + 2];
    }
    out[PVM_ADD] = s_add / (double)N;
    out[PVM_ADDS] = symb ? s_adds / (double)N : nan;
    out[PVM_PROJ2D] = s_proj / (double)N;
    const double dx = P[3] - G[3], dy = P[7] - G[7], dz = P[11] - G[11];
    out[PVM_TRANS_CM] = sqrt((dx * dx + dy * dy) + dz * dz) * 100.0;
    double trace = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double di = (P[i * 4] * G[i * 4] + P[i * 4 + 1] * G[i * 4 + 1]) + P[i * 4 + 2] * G[i * 4 + 2];
        trace = i ? trace + di : di;
    }
    trace = trace <= 3.0 ? trace : 3.0;
    trace = trace >= -1.0 ? trace : -1.0;
    out[PVM_ANG_DEG] = acos((trace - 1.0) / 2.0) * 57.29577951308232;   // np.rad2deg: x * (180 / pi)
}

__device__ long long mask_value(const void *base, size_t i, int elem)
{
    if (elem == 8) return ((const long long *)base)[i];
    if (elem == 4) return (long long)((const int *)base)[i];
    return (long long)((const uint8_t *)base)[i];
}

__global__ __launch_bounds__(kBlock) void k_mask_iou(const void *__restrict__ mp, const void *__restrict__ mg, long long sp,
                                                     long long sg, int ep, int eg, unsigned long long *__restrict__ inter,
                                                     unsigned long long *__restrict__ uni, int HW)
{
    __shared__ long long sh[2][kBlock / 64];
    const int b = blockIdx.y;
    const size_t op = (size_t)b * (size_t)sp, og = (size_t)b * (size_t)sg;
    long long si = 0, su = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < HW; i += gridDim.x * kBlock) {
        const long long a = mask_value(mp, op + i, ep), c = mask_value(mg, og + i, eg);
        si += a & c;
        su += a | c;
    }
    for (int off = 32; off > 0; off >>= 1) {                     // integer sums: any order is exact
        si += __shfl_down(si, off, 64);
        su += __shfl_down(su, off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[0][w] = si; sh[1][w] = su; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) { si += sh[0][k]; su += sh[1][k]; }
        atomicAdd(inter + b, (unsigned long long)si);
        atomicAdd(uni + b, (unsigned long long)su);
    }
}

}  // namespace

PVE_EXPORT int pvm_adds_slabs(int B, int N) { return auto_slabs(B, N); }

PVE_EXPORT size_t pvm_workspace_bytes(int B, int N, int slabs)
{
    if (B <= 0 || N <= 0) return 0;
    return layout(B, N, pick_slabs(B, N, slabs)).total;
}

PVE_EXPORT int pvm_pose_metrics_batched(const double *d_pose_pred, const double *d_pose_gt, const float *d_model,
                                        const double *d_K, const uint8_t *d_symmetric, double *d_metrics, int32_t *d_adds_idx,
                                        void *d_workspace, int B, int N, int K_batched, int slabs, void *stream)
{
    if (B < 0 || N <= 0 || B > 65535) return -1;
    if (B == 0) return 0;
    if (!d_pose_pred || !d_pose_gt || !d_model || !d_K || !d_metrics || !d_workspace) return -1;
    if (((uintptr_t)d_workspace & 15) != 0) return -1;
    const int S = pick_slabs(B, N, slabs);
    if (S > 65535) return -1;
    const Layout l = layout(B, N, S);
    char *ws = (char *)d_workspace;
    double *part = (double *)(ws + l.part);
    float4 *pred4 = (float4 *)(ws + l.pred4), *targ4 = (float4 *)(ws + l.targ4);
    unsigned long long *keys = (unsigned long long *)(ws + l.keys);
    hipStream_t st = (hipStream_t)stream;
    const int nt = ceil_div(N, kBlock);
    hipLaunchKernelGGL(k_transform, dim3(nt, B), dim3(kBlock), 0, st, d_pose_pred, d_pose_gt, d_model, d_K, d_symmetric, part,
                       pred4, targ4, N, nt, K_batched);
    if (d_symmetric) {
        const int L = ceil_div(N, S);
        hipLaunchKernelGGL(k_adds_search, dim3(ceil_div(N, kQTile), S, B), dim3(kBlock), 0, st, pred4, targ4, d_symmetric, keys,
                           N, S, L);
    }
    if (d_symmetric || d_adds_idx)
        hipLaunchKernelGGL(k_adds_merge, dim3(nt, B), dim3(kBlock), 0, st, d_pose_pred, d_pose_gt, d_model, d_symmetric, keys,
                           part, d_adds_idx, N, nt, S);
    hipLaunchKernelGGL(k_finish, dim3(ceil_div(B, 64)), dim3(64), 0, st, d_pose_pred, d_pose_gt, d_symmetric, part, d_metrics,
                       B, N, nt);
    return (int)hipGetLastError();
}

PVE_EXPORT int pvm_mask_iou_batched(const void *d_mask_pred, const void *d_mask_gt, long long pred_stride_b,
                                    long long gt_stride_b, int pred_elem_size, int gt_elem_size, long long *d_inter,
                                    long long *d_union, int B, int H, int W, void *stream)
{
    auto size_ok = [](int e) { return e == 1 || e == 4 || e == 8; };
    if (B < 0 || H <= 0 || W <= 0 || B > 65535 || (long long)H * W > 0x7fffffffll) return -1;
    if (B == 0) return 0;
    if (!d_mask_pred || !d_mask_gt || !d_inter || !d_union || !size_ok(pred_elem_size) || !size_ok(gt_elem_size)) return -1;
    if (pred_stride_b < 0 || gt_stride_b < 0) return -1;
    if (((uintptr_t)d_mask_pred % pred_elem_size) != 0 || ((uintptr_t)d_mask_gt % gt_elem_size) != 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(d_inter, 0, (size_t)B * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(d_union, 0, (size_t)B * sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    const int HW = H * W;
    int chunks = ceil_div(HW, kBlock * kMaskPerThread);
    chunks = chunks > 256 ? 256 : chunks;
    hipLaunchKernelGGL(k_mask_iou, dim3(chunks, B), dim3(kBlock), 0, st, d_mask_pred, d_mask_gt, pred_stride_b, gt_stride_b,
                       pred_elem_size, gt_elem_size, (unsigned long long *)d_inter, (unsigned long long *)d_union, HW);
    return (int)hipGetLastError();
}
