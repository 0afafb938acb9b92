// eval_common.hpp -- what the evaluation libraries (pvnet_metrics.hip, pvnet_vsd.hip) share.  Included inside the anonymous
// namespace of each translation unit, after its own `#pragma clang fp contract(off)`.
#pragma once

#define PVE_EXPORT extern "C" __attribute__((visibility("default")))

constexpr int kBlock = 256;        // threads per block everywhere; also the tile of the fixed-order sums

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Sum of the 256 values of a block in a fixed order: slot j += slot j + s for s = 128, 64, ..., 1.
__device__ double block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

__device__ bool pose_finite(const double *P)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && isfinite(P[i]);
    return ok;
}
