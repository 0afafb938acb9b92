// pvnet_pnp.hip -- uncertainty-weighted PnP refinement of clean-pvnet, batched, native HIP for gfx950.
// Replaces lib/csrc/uncertainty_pnp/src/uncertainty_pnp.cpp (Ceres, one image per call on the host):
//   residual functor  ReprojectionErrorArray::operator()   uncertainty_pnp.cpp:19-38
//   rotation          ceres::AngleAxisRotatePoint           include/ceres/rotation.h:563-622 (Rodrigues, first-order branch
//                                                            for theta^2 <= DBL_EPSILON)
//   solve             ceres::Solve, default options          uncertainty_pnp.cpp:71-89
// One wavefront per image (4 images per block): lane i owns keypoint i (PVNet: 9), computes its two residuals and their
// 2x6 Jacobian analytically in binary64, the 28 sums (JtJ upper triangle, Jt r, cost) are reduced through LDS, and every
// lane solves the damped 6x6 system by Cholesky itself (no broadcast).  Nothing here is throughput: it is a latency chain
// of ~10 iterations, which is why it lives on the GPU at all -- the keypoints and weights are already there (the voting
// layers produced them), and a batch of images costs what one image costs.
// The device code (residuals, Jacobian, damped solve, the iteration) is pnp_lm.hpp, shared with pvnet_pose.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "pnp_lm.hpp"
#include "pvnet_pnp.h"

#define PVP_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

using namespace pnp_lm;

constexpr int kWavesPerBlock = 4;

__global__ __launch_bounds__(64 * kWavesPerBlock) void k_uncertainty_pnp(
    const double *__restrict__ pts2d, const double *__restrict__ pts3d, const double *__restrict__ wgt2d,
    const double *__restrict__ Kmat, const double *__restrict__ init_rt, double *__restrict__ result_rt,
    double *__restrict__ info, int B, int pn, int pts3d_batched, int K_batched, int max_iter, double ftol)
{
    __shared__ double s_part[kWavesPerBlock][64][kSums + 1];   // per-lane contributions (one row per lane, padded)
    __shared__ double s_sum[kWavesPerBlock][kSums];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWavesPerBlock + wave;
    if (b >= B) return;                                        // whole wave: no block-level barrier below
    const double *p2 = pts2d + (size_t)b * pn * 2;
    const double *p3 = pts3d + (pts3d_batched ? (size_t)b * pn * 3 : 0);
    const double *wg = wgt2d + (size_t)b * pn * 3;
    const double *Kb = Kmat + (K_batched ? (size_t)b * 9 : 0);
    const Cam cam = {Kb[0], Kb[4], Kb[2], Kb[5]};              // uncertainty_pnp.cpp:79
    double x[6];
    for (int i = 0; i < 6; ++i) x[i] = init_rt[(size_t)b * 6 + i];

    const LmInfo r = lm_refine<false>(x, p2, p3, wg, cam, pn, max_iter, ftol, s_part[wave], s_sum[wave], lane);
    if (lane < 6) result_rt[(size_t)b * 6 + lane] = x[lane];
    if (info && lane == 0) {
        info[(size_t)b * 4] = r.initial_cost; info[(size_t)b * 4 + 1] = r.cost;
        info[(size_t)b * 4 + 2] = (double)r.iterations; info[(size_t)b * 4 + 3] = (double)r.termination;
    }
}

int launch(const double *pts2d, const double *pts3d, const double *wgt2d, const double *K, const double *init_rt,
           double *result_rt, double *info, int B, int pn, int pts3d_batched, int K_batched, int max_iter, double ftol,
           hipStream_t st)
{
    if (!pts2d || !pts3d || !wgt2d || !K || !init_rt || !result_rt || B <= 0 || pn < 1 || pn > 4096) return -1;
    hipLaunchKernelGGL(k_uncertainty_pnp, dim3((B + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0, st,
                       pts2d, pts3d, wgt2d, K, init_rt, result_rt, info, B, pn, pts3d_batched, K_batched, max_iter,
                       ftol > 0.0 ? ftol : 1e-6);
    return (int)hipGetLastError();
}

}  // namespace

PVP_EXPORT int pvp_uncertainty_pnp_batched(const double *d_pts2d, const double *d_pts3d, const double *d_wgt2d,
                                           const double *d_K, const double *d_init_rt, double *d_result_rt, double *d_info,
                                           int B, int pn, int pts3d_batched, int K_batched, int max_iterations,
                                           double function_tolerance, void *stream)
{
    return launch(d_pts2d, d_pts3d, d_wgt2d, d_K, d_init_rt, d_result_rt, d_info, B, pn, pts3d_batched, K_batched,
                  max_iterations, function_tolerance, (hipStream_t)stream);
}

PVP_EXPORT void uncertainty_pnp(double *pts2d, double *pts3d, double *wgt2d, double *K, double *init_rt, double *result_rt,
                                int pn)
{
    for (int i = 0; i < 6; ++i) result_rt[i] = init_rt[i];
    if (pn < 1) return;
    const size_t n2 = sizeof(double) * 2 * pn, n3 = sizeof(double) * 3 * pn;
    double *d = nullptr;                                       // one allocation: pts2d | pts3d | wgt2d | K | init | result
    const size_t total = n2 + n3 + n3 + sizeof(double) * (9 + 6 + 6);
    hipError_t e = hipMalloc(&d, total);
    if (e != hipSuccess) { fprintf(stderr, "uncertainty_pnp: %s\n", hipGetErrorString(e)); return; }
    double *d2 = d, *d3 = d2 + 2 * pn, *dw = d3 + 3 * pn, *dK = dw + 3 * pn, *di = dK + 9, *dr = di + 6;
    auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return r == hipSuccess; };
    if (ok(hipMemcpy(d2, pts2d, n2, hipMemcpyHostToDevice)) && ok(hipMemcpy(d3, pts3d, n3, hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(dw, wgt2d, n3, hipMemcpyHostToDevice)) && ok(hipMemcpy(dK, K, sizeof(double) * 9, hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(di, init_rt, sizeof(double) * 6, hipMemcpyHostToDevice))) {
        const int rc = launch(d2, d3, dw, dK, di, dr, nullptr, 1, pn, 0, 0, 0, 0.0, nullptr);
        if (rc == 0) ok(hipMemcpy(result_rt, dr, sizeof(double) * 6, hipMemcpyDeviceToHost));
        else fprintf(stderr, "uncertainty_pnp: bad arguments or launch failure (%d)\n", rc);
    }
    if (e != hipSuccess) fprintf(stderr, "uncertainty_pnp: %s\n", hipGetErrorString(e));
    (void)hipFree(d);
}
