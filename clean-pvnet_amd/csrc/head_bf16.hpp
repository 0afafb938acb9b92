// head_bf16.hpp -- the bfloat16 matrix-core mode of PVNet's output head (include/pvnet_vote.h, "PVNet output head", compute
// mode): the function of head.hpp with every matrix operand rounded once to bfloat16 (PVV_HEAD_COMPUTE_BF16 in pvv_head_forward's
// out_kind) and multiplied by v_mfma_f32_32x32x16_bf16 with float32 accumulation.  On the head's tile (head_tile.hpp, included
// in front of this file in pvnet_vote.hip): head_axis, head_blend, the row mapping, the activation and the store are the float32
// kernel's.  A lane's halo positions are set up here, not through HeadHaloLane: with it the kernel, at the 256-register ceiling,
// spilled two or three more SGPRs and measured 0.15 % slower at B = 32.  The order of the sums is free (tests/head_bf16_twin.py
// holds the result to a bound).
#pragma once

namespace {

typedef __bf16 head_b8v __attribute__((ext_vector_type(8)));

// Eight values rounded to bfloat16 as one 16-byte fragment, element 0 in the lowest half-word.
__device__ __forceinline__ uint4 head_pack8(const float (&v)[8])
{
    unsigned h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = head_bf16(v[j]);
    return make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
}

__device__ __forceinline__ head_f16v head_mfma_bf16(uint4 a, uint4 b, head_f16v c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(head_b8v, a), __builtin_bit_cast(head_b8v, b), c, 0, 0, 0);
}

// One workgroup works on `T` consecutive tiles of kHeadTh x kHeadTw output pixels (tile = (image * tiles_y + ty) * tiles_x + tx);
// the weights are converted to bf16 pieces and staged in LDS once for all of them.  CS = 16-channel k-steps of the concatenated
// tensor, PS = 2 * CS + 1 16-byte slots per halo position (odd: the 16 lanes of a ds_read_b128 group fall into 16 slots).
// LDS, in 16-byte slots:
//   halo [kHeadHalo][PS]             channel innermost: slot 2*cs + hh holds the channels 16*cs + 8*hh .. + 7; zero past C
//   w1   [9][CS][2][32*N1]           slot ((tap*CS + cs)*2 + hh)*32*N1 + o: weight1[o, 16*cs + 8*hh + j, tap], j = 0..7
//   w2   [N2][N1][2][2][32]          slot (((n2*N1 + n)*2 + st)*2 + hh)*32 + r: weight2[32*n2 + r, 32*n + 16*st + 8*(j>>2) + 4*hh + (j&3)]
// then float scale [32*N1], shift [32*N1], bias2 [32*N2].
//  1. Per tile the halo by HeadHaloLane's rule (head_tile.hpp), eight channels of a position per 16-byte store: wave w the
//     channel groups w, w + 4, ...
//  2. Conv1, k = (tap, channel): per tap and k-step one read of the weight fragment per row block and one of the halo per row.
//  3. t = fmaf(acc, scale, shift), a = t > 0 ? t : t * slope in registers: conv1's accumulator has the pixel on the lane and the
//     channels in its registers, so registers 8*st .. 8*st + 7 are the B fragment of conv2's k-step st (w2 is staged in that
//     k order).  No activation goes through LDS.
//  4. Conv2 from bias2, and the store.
template <int N1, int N2>
__global__ __launch_bounds__(kBlock) void k_head_forward_bf16(HeadShape s, int T, long long tiles, int tiles_x, int tiles_y,
                                                              const float *__restrict__ fm, const float *__restrict__ x,
                                                              const float *__restrict__ weight1, const float *__restrict__ scale,
                                                              const float *__restrict__ shift, const float *__restrict__ weight2,
                                                              const float *__restrict__ bias2, void *__restrict__ out)
{
    constexpr int MT1 = 32 * N1, MT2 = 32 * N2;
    extern __shared__ uint4 s_hb[];
    const int CS = (s.C + 15) >> 4, PS = 2 * CS + 1;
    const int halo_u = kHeadHalo * PS, w1_u = 9 * CS * 2 * MT1;
    constexpr int w2_u = N2 * N1 * 4 * 32;
    uint4 *s_halo = s_hb, *s_w1 = s_halo + halo_u, *s_w2 = s_w1 + w1_u;
    float *s_sc = (float *)(s_w2 + w2_u), *s_sh = s_sc + MT1, *s_b2 = s_sh + MT1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hi = lane >> 5;

    // ---- 0. once per workgroup: the weights as bf16 pieces, the folded BatchNorm, the bias, the halo's all-zero channel groups
    for (int e = tid; e < w1_u; e += kBlock) {
        const int o = e % MT1, hh = e / MT1 % 2, cs = e / (2 * MT1) % CS, tap = e / (2 * MT1 * CS);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 16 * cs + 8 * hh + j;
            const bool real = o < s.M1 && c < s.C;
            const float wv = weight1[real ? ((size_t)o * s.C + c) * 9 + tap : 0];
            v[j] = real ? wv : 0.f;
        }
        s_w1[e] = head_pack8(v);
    }
    for (int e = tid; e < w2_u; e += kBlock) {
        const int r = e % 32, hh = e / 32 % 2, st = e / 64 % 2, n = e / 128 % N1, n2 = e / (128 * N1);
        const int o = 32 * n2 + r;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = 32 * n + 16 * st + 8 * (j >> 2) + 4 * hh + (j & 3);
            const bool real = o < s.M2 && m < s.M1;
            const float wv = weight2[real ? (size_t)o * s.M1 + m : 0];
            v[j] = real ? wv : 0.f;
        }
        s_w2[e] = head_pack8(v);
    }
    for (int e = tid; e < MT1; e += kBlock) s_sc[e] = e < s.M1 ? scale[e] : 0.f, s_sh[e] = e < s.M1 ? shift[e] : 0.f;
    for (int e = tid; e < MT2; e += kBlock) s_b2[e] = e < s.M2 ? bias2[e] : 0.f;
    const int groups = (s.C + 7) >> 3;                            // channel groups of eight with a real channel; 2 * CS in all
    for (int e = tid; e < kHeadHalo * (2 * CS - groups); e += kBlock) {
        const int at = (e / (2 * CS - groups)) * PS + groups + e % (2 * CS - groups);
        s_halo[at] = make_uint4(0, 0, 0, 0);
    }

    const int plane = s.h * s.w, Plane = s.H * s.W;
    for (int it = 0; it < T; ++it) {
        const long long tile = (long long)blockIdx.x * T + it;
        if (tile >= tiles) break;                                  // the same for every thread
        const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x % tiles_y), b = (int)(tile / tiles_x / tiles_y);
        const int x0 = tx * kHeadTw, y0 = ty * kHeadTh;
        const float *fmb = fm + (size_t)b * s.fm_stride, *xb = x + (size_t)b * s.x_stride;

        // ---- 1. the halo.  A lane's positions r = lane + 64 i, as HeadHaloLane<true>::init computes them
        constexpr int NP = (kHeadHalo + 63) / 64;
        int n00[NP], n01[NP], n10[NP], n11[NP], nx[NP];
        float hl0[NP], hl1[NP], wl0[NP], wl1[NP];
        bool inside[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int r = lane + 64 * i, hy = r / kHeadHw, gy = y0 - 1 + hy, gx = x0 - 1 + (r - hy * kHeadHw);
            inside[i] = r < kHeadHalo && gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
            const HeadAxis ay = head_axis(s.rh, inside[i] ? gy : 0, s.h), ax = head_axis(s.rw, inside[i] ? gx : 0, s.w);
            n00[i] = ay.i0 * s.w + ax.i0, n01[i] = ay.i0 * s.w + ax.i1, n10[i] = ay.i1 * s.w + ax.i0, n11[i] = ay.i1 * s.w + ax.i1;
            hl0[i] = ay.l0, hl1[i] = ay.l1, wl0[i] = ax.l0, wl1[i] = ax.l1;
            nx[i] = inside[i] ? gy * s.W + gx : 0;
        }
        __syncthreads();                                           // the last tile's readers are done with the halo
        for (int g8 = wave; g8 < groups; g8 += 4) {
            const int c0 = 8 * g8;
            if (c0 + 8 <= s.C2) {                                  // eight upsampled channels
                const float *pl = fmb + (size_t)c0 * plane;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float *p = pl + (size_t)j * plane;
                        const float u = head_blend(hl0[i], hl1[i], wl0[i], wl1[i], p[n00[i]], p[n01[i]], p[n10[i]], p[n11[i]]);
                        v[j] = inside[i] ? u : 0.f;
                    }
                    if (lane + 64 * i < kHeadHalo) s_halo[(lane + 64 * i) * PS + g8] = head_pack8(v);
                }
            } else {                                               // the group with fm's last channels, the image's, the zeros past C
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int c = c0 + j;                      // the same for the whole wave
                        float u = 0.f;
                        if (c < s.C2) {
                            const float *p = fmb + (size_t)c * plane;
                            u = head_blend(hl0[i], hl1[i], wl0[i], wl1[i], p[n00[i]], p[n01[i]], p[n10[i]], p[n11[i]]);
                        } else if (c < s.C) {
                            u = xb[(size_t)(c - s.C2) * Plane + nx[i]];
                        }
                        v[j] = inside[i] ? u : 0.f;
                    }
                    if (lane + 64 * i < kHeadHalo) s_halo[(lane + 64 * i) * PS + g8] = head_pack8(v);
                }
            }
        }
        __syncthreads();                                           // the halo (and, the first time, step 0) is there

        // ---- 2. conv1
        head_f16v acc[kHeadG][N1] = {};
        const uint4 *hb = s_halo + (wave * kHeadG * kHeadHw + q) * PS + hi, *wb = s_w1 + hi * MT1 + q;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const uint4 *ht = hb + ((tap / 3) * kHeadHw + tap % 3) * PS, *wt = wb + tap * CS * 2 * MT1;
            for (int cs = 0; cs < CS; ++cs) {
                uint4 av[N1];
#pragma unroll
                for (int n = 0; n < N1; ++n) av[n] = wt[cs * 2 * MT1 + 32 * n];
#pragma unroll
                for (int g = 0; g < kHeadG; ++g) {
                    const uint4 bv = ht[g * kHeadHw * PS + 2 * cs];
#pragma unroll
                    for (int n = 0; n < N1; ++n) acc[g][n] = head_mfma_bf16(av[n], bv, acc[g][n]);
                }
            }
        }

        // ---- 3. and 4. BatchNorm, LeakyReLU, conv2 from the accumulators, the store
        const int gx = x0 + q;
#pragma unroll
        for (int g = 0; g < kHeadG; ++g) {
            head_f16v acc2[N2];
#pragma unroll
            for (int n2 = 0; n2 < N2; ++n2)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[n2][r] = s_b2[head_row(n2, r, hi)];
#pragma unroll
            for (int n = 0; n < N1; ++n)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    float a[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int r = 8 * st + j, o = head_row(n, r, hi);
                        a[j] = o < s.M1 ? head_act(acc[g][n][r], s_sc[o], s_sh[o], s.slope) : 0.f;
                    }
                    const uint4 bv = head_pack8(a);
#pragma unroll
                    for (int n2 = 0; n2 < N2; ++n2)
                        acc2[n2] = head_mfma_bf16(s_w2[(((n2 * N1 + n) * 2 + st) * 2 + hi) * 32 + q], bv, acc2[n2]);
                }
            const int gy = y0 + wave * kHeadG + g;
            if (gy < s.H && gx < s.W) {
#pragma unroll
                for (int n2 = 0; n2 < N2; ++n2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = head_row(n2, r, hi);
                        if (o < s.M2) head_store(out, s.out_kind, (((size_t)b * s.M2 + o) * s.H + gy) * s.W + gx, acc2[n2][r]);
                    }
            }
        }
    }
}

template <int N1, int N2>
size_t head_bf16_lds_bytes(const HeadShape &s)
{
    const size_t CS = ((size_t)s.C + 15) / 16, PS = 2 * CS + 1;
    return 16 * (kHeadHalo * PS + 9 * CS * 2 * 32 * N1 + (size_t)N2 * N1 * 128) + sizeof(float) * (2 * 32 * N1 + 32 * N2);
}

template <int N1, int N2>
int head_bf16_launch(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                     const float *weight2, const float *bias2, void *out, hipStream_t st)
{
    const size_t lds = head_bf16_lds_bytes<N1, N2>(s);
    int tiles_x, tiles_y;
    if (int e = head_raise_lds(reinterpret_cast<const void *>(&k_head_forward_bf16<N1, N2>), lds)) return e;
    if (int e = head_tiles(s, tiles_x, tiles_y)) return e;
    const long long tiles = (long long)tiles_x * tiles_y * s.B;
    // Tiles per workgroup: one while the launch is small, up to eight once there are thousands (the weights are staged once per
    // workgroup), more only to keep the grid below 2^30 workgroups.
    long long T = std::min(8ll, std::max(1ll, tiles / 1024));
    if ((tiles + T - 1) / T > (1ll << 30)) T = (tiles + (1ll << 30) - 1) >> 30;
    const dim3 grid((unsigned)((tiles + T - 1) / T));
    hipLaunchKernelGGL((k_head_forward_bf16<N1, N2>), grid, dim3(kBlock), lds, st, s, (int)T, tiles, tiles_x, tiles_y, fm, x,
                       weight1, scale, shift, weight2, bias2, out);
    return check_launch("k_head_forward_bf16");
}

// What pvv_head_forward calls for PVV_HEAD_COMPUTE_BF16, after its own checks (declared in head.hpp).
int head_bf16_forward(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                      const float *weight2, const float *bias2, void *out, hipStream_t st)
{
    return head_rows(s.M1, s.M2, [&](auto n1, auto n2) {
        return head_bf16_launch<decltype(n1)::value, decltype(n2)::value>(s, fm, x, weight1, scale, shift, weight2, bias2, out, st);
    });
}

}  // namespace
