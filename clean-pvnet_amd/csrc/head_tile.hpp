// head_tile.hpp -- the 8 x 32 output tile of PVNet's head, stated once for the three kernels that work on it (k_head_forward in
// head.hpp, k_head_stage in head_stage.hpp, k_head_forward_bf16 in head_bf16.hpp) and for k_head_upsample.  Included in
// pvnet_vote.hip in front of those files: -ffp-contract=off, so the blend rounds once per operation in the order written.
// Here: the tile's constants and HeadShape; the upsample's axis and blend; a lane's positions of the halo with the rule for
// positions outside the image; the accumulator's row mapping; BatchNorm + LeakyReLU; the float32 kernels' multiplication of one
// staged chunk of weight1; the store; the host's row ladder, LDS limit and tile grid.  Not here, each kernel's own: the LDS layout
// (channel-major floats in two, channel-innermost bf16 slots in the third), the walk over channels and chunks, how the threads
// stage a weight chunk (head.hpp: strided; head_stage.hpp: consecutive k of a row), head_bf16.hpp's halo arrays, the epilogue.
#pragma once

namespace {

constexpr int kHeadG = 2;                                   // rows of 32 pixels per wave: independent accumulators on one weight operand
constexpr int kHeadTh = 4 * kHeadG, kHeadTw = 32;           // output pixels of a workgroup: a 2-D tile, wave w its rows w*kHeadG ...
constexpr int kHeadPix = kHeadTh * kHeadTw;
constexpr int kHeadHh = kHeadTh + 2, kHeadHw = kHeadTw + 2; // the tile with its ring of one
constexpr int kHeadHalo = kHeadHh * kHeadHw;                // floats of one channel's halo in LDS
constexpr int kHeadKc = 36;                                 // k values per staged chunk of weight1: four channels, two pairs
constexpr int kHeadKs = kHeadKc + 1;                        // floats of a staged row: odd, so 32 rows fall into 32 banks
constexpr size_t kHeadMaxLds = 160 * 1024;                  // a CU's LDS; more than 64 KiB of it has to be asked for

static_assert(kBlock == 4 * 64 && kHeadTw == 32 && kHeadKc == 4 * 9, "4 waves, each kHeadG rows of 32 pixels");

struct HeadShape {
    int B, C2, C0, h, w, H, W, M1, M2;
    int C, Cpad, K, M1pad;            // C = C2 + C0 and rounded up to even, K = 9 * C, M1pad = M1 rounded up to even
    long long fm_stride, x_stride;    // elements between two images of fm / x
    float rh, rw, slope;
    int out_kind;
};

// One axis of torch's align_corners=True source index (ATen/native/UpSample.h, the CUDA bilinear kernel), float32:
// src = r * dst, i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1.  src never exceeds n_in - 1 by a whole
// step for n_in <= 2^23; the clamp keeps the address inside the plane whatever r is.
struct HeadAxis { int i0, i1; float l0, l1; };

__device__ __forceinline__ HeadAxis head_axis(float r, int dst, int n_in)
{
    HeadAxis a;
    const float src = r * (float)dst;
    a.i0 = min((int)src, n_in - 1);
    a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.f - a.l1;
    return a;
}

// The blend of the four neighbours, rows weighted hl0 / hl1 and columns wl0 / wl1: a zero weight still multiplies its sample.
__device__ __forceinline__ float head_blend(float hl0, float hl1, float wl0, float wl1, float v00, float v01, float v10, float v11)
{
    return hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11);
}

// A lane's positions r = lane + 64 i of the tile's halo, (kHeadTh + 2) x (kHeadTw + 2) with the origin (x0 - 1, y0 - 1): for
// each whether it lies in the image, its element `nx` of an [H,W] plane and, with UP, its four neighbours in an [h,w] plane and
// their weights -- computed once for every channel.  A position outside the image (the convolution's padding ring, whatever a
// partial tile overhangs, the r past the halo) loads element 0 and holds a zero: no load waits on a branch.
template <bool UP>
struct HeadHaloLane {
    static constexpr int NP = (kHeadHalo + 63) / 64, NB = UP ? NP : 1;
    int n00[NB], n01[NB], n10[NB], n11[NB], nx[NP];
    float hl0[NB], hl1[NB], wl0[NB], wl1[NB];
    bool inside[NP];

    __device__ __forceinline__ void init(const HeadShape &s, int x0, int y0, int lane)
    {
        const int H = s.H, W = s.W;                                // read ahead of the && below: no branch around a load
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int r = lane + 64 * i, hy = r / kHeadHw, gy = y0 - 1 + hy, gx = x0 - 1 + (r - hy * kHeadHw);
            inside[i] = r < kHeadHalo && gy >= 0 && gy < H && gx >= 0 && gx < W;
            if constexpr (UP) {
                const HeadAxis ay = head_axis(s.rh, inside[i] ? gy : 0, s.h), ax = head_axis(s.rw, inside[i] ? gx : 0, s.w);
                n00[i] = ay.i0 * s.w + ax.i0, n01[i] = ay.i0 * s.w + ax.i1, n10[i] = ay.i1 * s.w + ax.i0, n11[i] = ay.i1 * s.w + ax.i1;
                hl0[i] = ay.l0, hl1[i] = ay.l1, wl0[i] = ax.l0, wl1[i] = ax.l1;
            }
            nx[i] = inside[i] ? gy * W + gx : 0;
        }
    }
    // Position i's value of one channel: upsampled from the channel's [h,w] plane, or read from its [H,W] plane.
    __device__ __forceinline__ float up(const float *__restrict__ pl, int i) const
    {
        return head_blend(hl0[i], hl1[i], wl0[i], wl1[i], pl[n00[i]], pl[n01[i]], pl[n10[i]], pl[n11[i]]);
    }
    __device__ __forceinline__ float at(const float *__restrict__ pl, int i) const { return pl[nx[i]]; }
    // What the halo holds at position i, given the value loaded for it.
    __device__ __forceinline__ float held(int i, float v) const { return inside[i] ? v : 0.f; }
    // Whether position i of `lane` is one of the halo's: the last i runs past it.
    static __device__ __forceinline__ bool in_halo(int lane, int i) { return lane + 64 * i < kHeadHalo; }
};

// One thread per element of u [B, C2, H, W].
__global__ __launch_bounds__(kBlock) void k_head_upsample(HeadShape s, const float *__restrict__ fm, float *__restrict__ u)
{
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)s.B * s.C2 * s.H * s.W) return;
    const int x = (int)(idx % s.W), y = (int)(idx / s.W % s.H);
    const int c = (int)(idx / s.W / s.H % s.C2), b = (int)(idx / s.W / s.H / s.C2);
    const float *pl = fm + (size_t)b * s.fm_stride + (size_t)c * s.h * s.w;
    const HeadAxis ay = head_axis(s.rh, y, s.h), ax = head_axis(s.rw, x, s.w);
    const float *p0 = pl + ay.i0 * s.w, *p1 = pl + ay.i1 * s.w;
    u[idx] = head_blend(ay.l0, ay.l1, ax.l0, ax.l1, p0[ax.i0], p0[ax.i1], p1[ax.i0], p1[ax.i1]);
}

__device__ __forceinline__ unsigned short head_bf16(float v)     // round to nearest even; a NaN stays a quiet NaN
{
    const unsigned bits = __float_as_uint(v);
    if (v != v) return (unsigned short)((bits >> 16) | 0x40u);
    return (unsigned short)((bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ void head_store(void *__restrict__ out, int kind, size_t at, float v)
{
    if (kind == PVV_HEAD_OUT_F32) ((float *)out)[at] = v;
    else if (kind == PVV_HEAD_OUT_F16) ((_Float16 *)out)[at] = (_Float16)v;
    else ((unsigned short *)out)[at] = head_bf16(v);
}

typedef float head_f16v __attribute__((ext_vector_type(16)));

// The output row that register r of a 32 x 32 accumulator holds on a lane of half `hi` = lane >> 5, in row block n.
__device__ __forceinline__ constexpr int head_row(int n, int r, int hi) { return 32 * n + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// The folded BatchNorm and the LeakyReLU: the one fused multiply-add of the contract.
__device__ __forceinline__ float head_act(float acc, float sc, float sh, float slope)
{
    const float t = __builtin_fmaf(acc, sc, sh);
    return t > 0.f ? t : t * slope;
}

// Where k = 2j + hi of a pair of channels lies in the halo, past the pixel's window origin: channel k / 9, tap k % 9.
__device__ __forceinline__ constexpr int head_k_offset(int k)
{
    return (k / 9) * kHeadHalo + ((k % 9) / 3) * kHeadHw + (k % 9) % 3;
}

// One staged chunk times the halo: `wb` is the lane's row and half of the chunk's buffer, `hb` its window of the chunk's first
// channel.  Per pair of channels, tap and row of pixels one read of the halo, per row block one of the weights, into
// v_mfma_f32_32x32x2_f32: per output one chain over k ascending.  The chains run in a copy `c`: through the reference the compiler
// carries a second set of accumulators round the loop (N1 = 2: 26 to 62 VGPRs more; k_head_stage<4, false>: 240 bytes of scratch;
// profiles/head_tile_refactor_ab.json, isa.head_conv1_chunk_through_the_reference; tests/test_host.py holds the guard).
template <int N1>
__device__ __forceinline__ void head_conv1_chunk(const float *wb, const float *hb, int pairs, const int (&koff)[9],
                                                 head_f16v (&acc)[kHeadG][N1])
{
    head_f16v c[kHeadG][N1];
#pragma unroll
    for (int g = 0; g < kHeadG; ++g)
#pragma unroll
        for (int a = 0; a < N1; ++a) c[g][a] = acc[g][a];
    for (int p = 0; p < pairs; ++p, wb += 18, hb += 2 * kHeadHalo) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float av[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) av[a] = wb[2 * j + 32 * a * kHeadKs];
#pragma unroll
            for (int g = 0; g < kHeadG; ++g) {
                const float bv = hb[koff[j] + g * kHeadHw];
#pragma unroll
                for (int a = 0; a < N1; ++a) c[g][a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv, c[g][a], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kHeadG; ++g)
#pragma unroll
        for (int a = 0; a < N1; ++a) acc[g][a] = c[g][a];
}

// ---- host side

// f(N1, N2) with the 32-row blocks of M1 and M2 as std::integral_constant<int, 1 or 2>.
template <class F>
int head_rows(int M1, int M2, F f)
{
    const std::integral_constant<int, 1> one;
    const std::integral_constant<int, 2> two;
    if (M1 > 32) return M2 > 32 ? f(two, two) : f(two, one);
    return M2 > 32 ? f(one, two) : f(one, one);
}

// Refuses `lds` bytes of dynamic LDS a CU does not have and asks for what is above 64 KiB: per launch, the limit belongs to the
// current device's copy of the kernel.
int head_raise_lds(const void *kernel, size_t lds)
{
    if (lds > kHeadMaxLds) return fail(PVV_E_ARG, "head: C2 + C0 channels of the tile's halo do not fit 160 KiB of LDS");
    if (lds > 64 * 1024 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHeadMaxLds) != hipSuccess)
        return fail(PVV_E_ARG, "head: the kernel's LDS limit could not be raised");
    return PVV_OK;
}

int head_tiles(const HeadShape &s, int &tiles_x, int &tiles_y)
{
    tiles_x = (s.W + kHeadTw - 1) / kHeadTw, tiles_y = (s.H + kHeadTh - 1) / kHeadTh;
    if (tiles_y > 65535) return fail(PVV_E_ARG, "head: H is too large for one launch");
    return PVV_OK;
}

}  // namespace
