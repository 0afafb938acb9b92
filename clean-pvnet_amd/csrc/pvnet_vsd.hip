// pvnet_vsd.hip -- a batched depth rasteriser and the Visible Surface Discrepancy of a whole batch on the device, native HIP
// for gfx950 (include/pvnet_vsd.h has both arithmetic contracts and the reference lines each pass replaces).  The coverage rules
// of the rasteriser -- snapping, near clip, edge functions, the sweep -- are raster.hpp's, shared with the colour renderer.
//
//   k_vertices    grid (vertex tiles, P): eye-space coordinates in binary64 and the snapped image coordinates of every
//                 (pose, vertex), once -- not once per triangle corner.
//   k_raster      grid (tiles of 256 triangles, P).  A lane sets up one triangle (near clip, orientation, bounding box);
//                 then the work is shared by its size: a piece whose bounding box holds at most kSmall samples is swept by
//                 its own lane, every other piece by the whole wave -- 64 blocks of 8x8 samples are tested against the
//                 three edges at a time (one block per lane), the blocks that survive are sampled one sample per lane.
//                 A large flat triangle therefore keeps 64 lanes busy instead of leaving 63 waiting.  Depth: an unsigned
//                 atomicMin on the float bits.
//   k_resolve     the untouched samples (0xffffffff from the memset on the stream) become 0, the background.
//   k_vsd         grid (pixel chunks, pairs): distance images, visibility masks and costs of one (prediction, ground truth)
//                 pair, integer counts reduced per block and added with integer atomics; the 'tlinear' costs as one
//                 tree-reduced sum per tile of 256 pixels.
//   k_vsd_finish  a thread per pair: the tile sums in ascending order and the error.
//
// Index bounds: vertex i < N (grid tail and the face check 0 <= index < N before any vertex is read), triangle f < F, pose
// p < P by the grid; every sample a kernel touches satisfies 0 <= x < W and 0 <= y < H because a piece's bounding box is
// clamped to the image rectangle before it is swept (raster.hpp, make_piece); pixel index < H*W and tile < ntiles in k_vsd.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "pvnet_vsd.h"

#pragma clang fp contract(off)

namespace {

#include "eval_common.hpp"
#include "raster.hpp"

using namespace raster;

constexpr int kTilesPerBlock = 4;    // k_vsd: tiles of 256 pixels a block walks
constexpr unsigned kEmpty = 0xffffffffu;

__global__ __launch_bounds__(kBlock) void k_vertices(const float *__restrict__ pts, const double *__restrict__ pose,
                                                     const double *__restrict__ K, Vtx *__restrict__ vtx, int N, int K_batched,
                                                     double near)
{
    const int p = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    vtx[(size_t)p * N + i] = vertex(pose + (size_t)p * 12, c, (double)pts[i * 3], (double)pts[i * 3 + 1], (double)pts[i * 3 + 2], near);
}

// The depth sink: an unsigned atomicMin on the float bits of a sample's depth, the same image whichever lane owns the piece.
struct DepthSink {
    unsigned *img;
    int W;
    double near, far;

    __device__ void operator()(int x, int y, const Plane &pl, const Cam &c) const
    {
        double dx, dy, Z;
        if (!plane_depth(pl, c, x, y, &dx, &dy, &Z)) return;
        if (Z >= near && Z <= far) atomicMin(img + (size_t)y * W + x, __float_as_uint((float)Z));
    }

    __device__ const DepthSink &of(int) const { return *this; }
};

__global__ __launch_bounds__(kBlock) void k_raster(const int32_t *__restrict__ faces, const Vtx *__restrict__ vtx,
                                                   const double *__restrict__ pose, const double *__restrict__ K,
                                                   unsigned *__restrict__ depth, int N, int F, int K_batched, int W, int H,
                                                   double near, double far)
{
    const int p = blockIdx.y;
    if (!pose_finite(pose + (size_t)p * 12)) return;       // block-uniform: an all-zero image
    const Cam c = load_cam(K + (K_batched ? (size_t)p * 9 : 0));
    const int f = blockIdx.x * kBlock + threadIdx.x;
    Face fc = {};                                           // no piece
    if (f < F) {
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        if (i0 >= 0 && i0 < N && i1 >= 0 && i1 < N && i2 >= 0 && i2 < N) {
            const Vtx *vp = vtx + (size_t)p * N;
            fc = clip_face(c, vp[i0], vp[i1], vp[i2], near, W, H);
        }
    }
    const DepthSink sink = {depth + (size_t)p * H * W, W, near, far};
    sweep(fc.pc0, fc.pl, sink, c);
    if (__any(fc.pc1.w != 0)) sweep(fc.pc1, fc.pl, sink, c);
}

__global__ __launch_bounds__(kBlock) void k_resolve(unsigned *__restrict__ depth, size_t total)
{
    const size_t n4 = total / 4, stride = (size_t)gridDim.x * kBlock;
    uint4 *d4 = (uint4 *)depth;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        uint4 v = d4[i];
        if (v.x == kEmpty || v.y == kEmpty || v.z == kEmpty || v.w == kEmpty) {
            v.x = v.x == kEmpty ? 0u : v.x;
            v.y = v.y == kEmpty ? 0u : v.y;
            v.z = v.z == kEmpty ? 0u : v.z;
            v.w = v.w == kEmpty ? 0u : v.w;
            d4[i] = v;
        }
    }
    const size_t i = n4 * 4 + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < total && depth[i] == kEmpty) depth[i] = 0u;
}

// ------------------------------------------------------------------------------------------------------------------- VSD
template <int KIND>
__device__ double load_test(const void *p, size_t i, double scale)
{
    if (KIND == PVS_TEST_U16) return (double)((const uint16_t *)p)[i] * scale;
    if (KIND == PVS_TEST_F32) return (double)((const float *)p)[i];
    return ((const double *)p)[i];
}

// Xs = ((x - cx)*depth)*(1/fx), Ys alike, sqrt((Xs*Xs + Ys*Ys) + depth*depth)
__device__ double dist_of(double xc, double yc, double ifx, double ify, double depth)
{
    const double Xs = (xc * depth) * ifx, Ys = (yc * depth) * ify;
    return sqrt((Xs * Xs + Ys * Ys) + depth * depth);
}

__device__ bool visible(double dist_test, double dist_model, float delta)
{
    const bool valid = dist_test > 0.0 && dist_model > 0.0;
    const float d_diff = (float)dist_model - (float)dist_test;
    return d_diff <= delta && valid;
}

__device__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

template <int KIND, bool TLINEAR>
__global__ __launch_bounds__(kBlock) void k_vsd(const float *__restrict__ depth_est, const float *__restrict__ depth_gt,
                                                const void *__restrict__ depth_test, double depth_scale,
                                                const double *__restrict__ K, int K_batched, double delta, double tau,
                                                unsigned long long *__restrict__ counts, double *__restrict__ tiles, int p, int g,
                                                int W, int HW, int ntiles)
{
    __shared__ double sh[kBlock];
    __shared__ unsigned shc[3][kBlock / 64];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int i = pair / (p * g), a = (pair / g) % p, b = pair % g;
    const float *est = depth_est + ((size_t)i * p + a) * HW, *gt = depth_gt + ((size_t)i * g + b) * HW;
    const size_t test0 = (size_t)i * HW;
    const double *Kc = K + (K_batched ? (size_t)i * 9 : 0);
    const double cx = Kc[2], cy = Kc[5], ifx = 1.0 / Kc[0], ify = 1.0 / Kc[4], itau = 1.0 / tau;
    const float fdelta = (float)delta;
    unsigned n_union = 0, n_inter = 0, n_cost = 0;
    for (int k = 0; k < kTilesPerBlock; ++k) {
        const int tile = blockIdx.x * kTilesPerBlock + k;
        if (tile >= ntiles) break;                          // block-uniform
        const int pix = tile * kBlock + tid;
        double cost = 0.0;
        if (pix < HW) {
            const float dg = gt[pix], de = est[pix];
            if (dg != 0.0f || de != 0.0f) {                 // both renders empty: neither mask can hold the pixel
                const int y = pix / W, x = pix - y * W;
                const double xc = (double)x - cx, yc = (double)y - cy;
                const double dist_t = dist_of(xc, yc, ifx, ify, load_test<KIND>(depth_test, test0 + pix, depth_scale));
                const double dist_g = dist_of(xc, yc, ifx, ify, (double)dg), dist_e = dist_of(xc, yc, ifx, ify, (double)de);
                const bool vg = visible(dist_t, dist_g, fdelta);
                const bool ve = visible(dist_t, dist_e, fdelta) || (vg && dist_e > 0.0);
                n_union += (vg || ve) ? 1u : 0u;
                if (vg && ve) {
                    ++n_inter;
                    const double c = fabs(dist_g - dist_e);
                    n_cost += c >= tau ? 1u : 0u;
                    const double cl = c * itau;
                    cost = cl > 1.0 ? 1.0 : cl;
                }
            }
        }
        if (TLINEAR) {
            const double s = block_sum(cost, sh);
            if (tid == 0) tiles[(size_t)pair * ntiles + tile] = s;
        }
    }
    n_union = wave_sum(n_union);
    n_inter = wave_sum(n_inter);
    n_cost = wave_sum(n_cost);
    if ((tid & 63) == 0) {
        shc[0][tid >> 6] = n_union;
        shc[1][tid >> 6] = n_inter;
        shc[2][tid >> 6] = n_cost;
    }
    __syncthreads();
    if (tid < 3) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += shc[tid][w];
        if (s) atomicAdd(counts + (size_t)pair * 3 + tid, (unsigned long long)s);
    }
}

__global__ void k_vsd_finish(const long long *__restrict__ counts, const double *__restrict__ tiles, double *__restrict__ e,
                             int pairs, int ntiles, int tlinear)
{
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= pairs) return;
    const long long n_union = counts[(size_t)pair * 3 + PVS_UNION], n_inter = counts[(size_t)pair * 3 + PVS_INTER];
    double r = 1.0;
    if (n_union > 0) {
        if (tlinear) {
            double s = 0.0;
            for (int t = 0; t < ntiles; ++t) s += tiles[(size_t)pair * ntiles + t];
            r = (s + (double)(n_union - n_inter)) / (double)n_union;
        } else {
            r = (double)(counts[(size_t)pair * 3 + PVS_COST] + (n_union - n_inter)) / (double)n_union;
        }
    }
    e[pair] = r;
}

template <int KIND>
void launch_vsd(bool tlinear, dim3 grid, hipStream_t st, const float *est, const float *gt, const void *test, double scale,
                const double *K, int K_batched, double delta, double tau, unsigned long long *counts, double *tiles, int p, int g,
                int W, int HW, int ntiles)
{
    if (tlinear)
        hipLaunchKernelGGL((k_vsd<KIND, true>), grid, dim3(kBlock), 0, st, est, gt, test, scale, K, K_batched, delta, tau, counts,
                           tiles, p, g, W, HW, ntiles);
    else
        hipLaunchKernelGGL((k_vsd<KIND, false>), grid, dim3(kBlock), 0, st, est, gt, test, scale, K, K_batched, delta, tau, counts,
                           tiles, p, g, W, HW, ntiles);
}

bool side_ok(int v) { return v > 0 && v <= PVS_MAX_SIDE; }

}  // namespace

PVE_EXPORT size_t pvs_render_workspace_bytes(int P, int N)
{
    if (P <= 0 || N <= 0) return 0;
    return (size_t)P * N * sizeof(Vtx);
}

PVE_EXPORT int pvs_render_depth_batched(const float *d_pts, const int32_t *d_faces, const double *d_pose, const double *d_K,
                                        float *d_depth, void *d_workspace, int P, int N, int F, int K_batched, int W, int H,
                                        double near, double far, void *stream)
{
    if (P < 0 || P > 65535 || N <= 0 || F < 0 || !side_ok(W) || !side_ok(H)) return -1;
    if (N > INT_MAX / 3 || F > INT_MAX / 3) return -1;
    if (!(near > 0.0) || !(far >= near)) return -1;         // also refuses NaN
    if (P == 0) return 0;
    if (!d_pts || !d_pose || !d_K || !d_depth || !d_workspace || (F > 0 && !d_faces)) return -1;
    if (((uintptr_t)d_workspace & 15) != 0 || ((uintptr_t)d_depth & 15) != 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)P * H * W;
    hipError_t e = hipMemsetAsync(d_depth, 0xff, total * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    Vtx *vtx = (Vtx *)d_workspace;
    if (F > 0) {
        hipLaunchKernelGGL(k_vertices, dim3(ceil_div(N, kBlock), P), dim3(kBlock), 0, st, d_pts, d_pose, d_K, vtx, N, K_batched,
                           near);
        hipLaunchKernelGGL(k_raster, dim3(ceil_div(F, kBlock), P), dim3(kBlock), 0, st, d_faces, vtx, d_pose, d_K,
                           (unsigned *)d_depth, N, F, K_batched, W, H, near, far);
    }
    size_t blocks = (total / 4 + kBlock - 1) / kBlock;
    blocks = blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(k_resolve, dim3((unsigned)blocks), dim3(kBlock), 0, st, (unsigned *)d_depth, total);
    return (int)hipGetLastError();
}

PVE_EXPORT size_t pvs_vsd_workspace_bytes(int n, int p, int g, int H, int W, int cost_type)
{
    if (n <= 0 || p <= 0 || g <= 0 || H <= 0 || W <= 0 || cost_type != PVS_COST_TLINEAR) return 0;
    const size_t ntiles = ((size_t)H * W + kBlock - 1) / kBlock;
    return (size_t)n * p * g * ntiles * sizeof(double);
}

PVE_EXPORT int pvs_vsd_batched(const float *d_depth_est, const float *d_depth_gt, const void *d_depth_test, int test_kind,
                               double depth_scale, const double *d_K, int K_batched, double delta, double tau, int cost_type,
                               long long *d_counts, double *d_e, void *d_workspace, int n, int p, int g, int H, int W,
                               void *stream)
{
    if (n < 0 || p < 0 || g < 0 || !side_ok(W) || !side_ok(H)) return -1;
    if (cost_type != PVS_COST_STEP && cost_type != PVS_COST_TLINEAR) return -1;
    if (test_kind < PVS_TEST_U16 || test_kind > PVS_TEST_F64) return -1;
    const long long pairs = (long long)n * p * g;
    if (pairs > 65535) return -1;
    if (pairs == 0) return 0;
    if (!d_depth_est || !d_depth_gt || !d_depth_test || !d_K || !d_counts || !d_e) return -1;
    const bool tlinear = cost_type == PVS_COST_TLINEAR;
    if (tlinear && (!d_workspace || ((uintptr_t)d_workspace & 15) != 0)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, ntiles = ceil_div(HW, kBlock);
    hipError_t err = hipMemsetAsync(d_counts, 0, (size_t)pairs * 3 * sizeof(long long), st);
    if (err != hipSuccess) return (int)err;
    const dim3 grid(ceil_div(ntiles, kTilesPerBlock), (unsigned)pairs);
    unsigned long long *counts = (unsigned long long *)d_counts;
    double *tiles = (double *)d_workspace;
    switch (test_kind) {
    case PVS_TEST_U16:
        launch_vsd<PVS_TEST_U16>(tlinear, grid, st, d_depth_est, d_depth_gt, d_depth_test, depth_scale, d_K, K_batched, delta, tau,
                                 counts, tiles, p, g, W, HW, ntiles);
        break;
    case PVS_TEST_F32:
        launch_vsd<PVS_TEST_F32>(tlinear, grid, st, d_depth_est, d_depth_gt, d_depth_test, depth_scale, d_K, K_batched, delta, tau,
                                 counts, tiles, p, g, W, HW, ntiles);
        break;
    default:
        launch_vsd<PVS_TEST_F64>(tlinear, grid, st, d_depth_est, d_depth_gt, d_depth_test, depth_scale, d_K, K_batched, delta, tau,
                                 counts, tiles, p, g, W, HW, ntiles);
        break;
    }
    hipLaunchKernelGGL(k_vsd_finish, dim3(ceil_div((int)pairs, 64)), dim3(64), 0, st, (const long long *)d_counts, tiles, d_e,
                       (int)pairs, ntiles, tlinear ? 1 : 0);
    return (int)hipGetLastError();
}
