// head_stage_bf16.hpp -- the bfloat16 matrix-core mode of PVNet's decoder stages (include/pvnet_vote.h, "PVNet decoder stage",
// compute mode): the function of head_stage.hpp with z and weight1 rounded once to bfloat16 (PVV_HEAD_STAGE_BF16 beside
// PVV_HEAD_STAGE in pvv_head_forward's out_kind) and multiplied by v_mfma_f32_32x32x16_bf16 with float32 accumulation.  On the
// head's tile (head_tile.hpp, included in front of this file in pvnet_vote.hip): head_axis, head_blend, the rule for positions
// outside the image, the row mapping, the activation, the store and the tile grid are the float32 kernels'; head_pack8 and the
// operand layout -- channel innermost, eight channels to a 16-byte slot, k = (tap, channel) -- are head_bf16.hpp's, included in
// front of this file too.  This file's own: BOTH operands go through LDS in chunks of channels, so C2 + C0 has no limit and
// M1 goes up to 128; a halo position's indices and weights are computed by HeadHaloLane's rule when the position is filled, not
// kept (beside 128 accumulator registers six positions' worth of them do not fit 256 VGPRs).  The order of the sums is free
// (tests/decoder_bf16_twin.py holds the result to a bound).
#pragma once

namespace {

// Per 32 * N1 output rows: CH channels of a chunk, GS = CH / 8 slots of eight channels, PS slots of a halo position (odd: the
// 16 lanes of a ds_read_b128 group fall into 16 slots), WS slots between two channel groups of the weights (the pad keeps the
// staging's dword stores, 128 / CH rows of CH / 2 channel pairs per wave, in 64 banks).  `bytes` is the kernel's dynamic LDS --
// the one expression the kernel's pointers and the launch both take:
//   N1 = 4: CH = 16, 16 * (340 * 3 + 9 * 2 * 136) = 55488 bytes, two workgroups per CU by the 256 registers of a lane
//   N1 = 2: CH = 32, 16 * (340 * 5 + 9 * 4 * 68)  = 66368 bytes, two workgroups per CU (above 64 KiB: the attribute is raised)
//   N1 = 1: CH = 32, 16 * (340 * 5 + 9 * 4 * 36)  = 47936 bytes, three by LDS, two by __launch_bounds__
template <int N1>
struct StageBf16Lds {
    static constexpr int CH = N1 == 4 ? 16 : 32, GS = CH / 8, PS = GS + 1, WS = 32 * N1 + 128 / CH;
    static constexpr int halo_slots = kHeadHalo * PS, w_slots = 9 * GS * WS;
    static constexpr size_t bytes = 16 * (size_t)(halo_slots + w_slots);
};

constexpr int kStageBf16Rounds = (kHeadHalo + 63) / 64;      // a channel group's halo positions, in waves: the last is partial
constexpr int kStageBf16Fill = 256;                          // workgroups below which M1 is split over more of them (the CUs)

// One workgroup per (kHeadTh x kHeadTw output pixels, block of 32 * N1 output channels, image), as k_head_stage.  Per chunk of CH
// channels of z = cat([u, skip]):
//  1. The halo: item = (channel group g, position r), a wave's items of one group; r = 64 * round + lane as far as kHeadHalo.
//     The position's place in the image and, with UP, its four neighbours and weights by HeadHaloLane's rule; eight channels
//     -- of fm, of the skip tensor, zeros past C, or a mix where the group straddles -- rounded and stored as one slot.
//     A position outside the image loads element 0 and stores zeros.
//  2. weight1: item = (row, pair of channels), 18 consecutive floats of the caller's float32 weights, rounded and stored as one
//     dword per tap into slot (tap, channel group, row); rows past M1 and channels past C load a valid element and store zeros.
//  3. Per 16-channel k-step and tap one read of the weight fragment per row block and one of the halo per row of pixels; the
//     accumulators run across all chunks.  k-step outer, tap inner: a chunk of 32 sums as two chunks of 16, so every N1 gives
//     an output the same order.
// then t = fmaf(acc, scale, shift), a = t > 0 ? t : t * slope to global memory as k_head_stage stores it.
template <int N1, bool UP>
__global__ __launch_bounds__(kBlock, 2) void k_head_stage_bf16(HeadShape s, int tiles_x, const float *__restrict__ fm,
                                                               const float *__restrict__ x, const float *__restrict__ weight1,
                                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                                               void *__restrict__ out)
{
    using L = StageBf16Lds<N1>;
    constexpr int MT1 = 32 * N1, CH = L::CH, GS = L::GS, PS = L::PS, WS = L::WS;
    extern __shared__ uint4 s_sb[];
    uint4 *s_halo = s_sb, *s_w = s_sb + L::halo_slots;
    unsigned *s_wd = (unsigned *)s_w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hi = lane >> 5;
    const int mblock = blockIdx.x / tiles_x, o0 = mblock * MT1;
    const int x0 = (blockIdx.x - mblock * tiles_x) * kHeadTw, y0 = blockIdx.y * kHeadTh, b = blockIdx.z;
    const float *fmb = fm + (size_t)b * s.fm_stride, *xb = x + (size_t)b * s.x_stride;
    const int plane = s.h * s.w, Plane = s.H * s.W;

    head_f16v acc[kHeadG][N1] = {};
    const uint4 *hb = s_halo + (wave * kHeadG * kHeadHw + q) * PS + hi, *wb = s_w + hi * WS + q;

    for (int c0 = 0; c0 < s.C; c0 += CH) {
        if (c0) __syncthreads();                                   // every wave is done with the last chunk

        // ---- 1. the halo of the channels c0 .. c0 + CH - 1
        for (int item = wave; item < GS * kStageBf16Rounds; item += 4) {
            const int g = item / kStageBf16Rounds, r = (item - g * kStageBf16Rounds) * 64 + lane;   // g: the same for the wave
            const int hy = r / kHeadHw, gy = y0 - 1 + hy, gx = x0 - 1 + (r - hy * kHeadHw);
            const bool inside = r < kHeadHalo && gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
            const int nx = inside ? gy * s.W + gx : 0;
            int n00 = nx, n01 = nx, n10 = nx, n11 = nx;
            float hl0 = 0.f, hl1 = 0.f, wl0 = 0.f, wl1 = 0.f;
            if constexpr (UP) {
                const HeadAxis ay = head_axis(s.rh, inside ? gy : 0, s.h), ax = head_axis(s.rw, inside ? gx : 0, s.w);
                n00 = ay.i0 * s.w + ax.i0, n01 = ay.i0 * s.w + ax.i1, n10 = ay.i1 * s.w + ax.i0, n11 = ay.i1 * s.w + ax.i1;
                hl0 = ay.l0, hl1 = ay.l1, wl0 = ax.l0, wl1 = ax.l1;
            }
            auto of_fm = [&](const float *p) {                     // u at the position, of the channel whose plane is p
                if constexpr (UP) return head_blend(hl0, hl1, wl0, wl1, p[n00], p[n01], p[n10], p[n11]);
                else return p[nx];
            };
            const int c = c0 + 8 * g;
            float v[8];
            if (c + 8 <= s.C2) {                                   // eight of fm's channels
                const float *pl = fmb + (size_t)c * plane;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = of_fm(pl + (size_t)j * plane);
            } else if (c >= s.C2 && c + 8 <= s.C) {                // eight of the skip tensor's
                const float *pl = xb + (size_t)(c - s.C2) * Plane + nx;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = pl[(size_t)j * Plane];
            } else {                                               // fm's last, the skip tensor's first or last, the zeros past C
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int cj = c + j;                          // the same for the whole wave
                    v[j] = 0.f;
                    if (cj < s.C2) v[j] = of_fm(fmb + (size_t)cj * plane);
                    else if (cj < s.C) v[j] = xb[(size_t)(cj - s.C2) * Plane + nx];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = inside ? v[j] : 0.f;
            if (r < kHeadHalo) s_halo[r * PS + g] = head_pack8(v);
        }

        // ---- 2. weight1's rows o0 .. o0 + MT1 - 1 of the same channels
        for (int item = tid; item < MT1 * (CH / 2); item += kBlock) {
            const int pr = item % (CH / 2), row = item / (CH / 2), o = o0 + row, c = c0 + 2 * pr;
            const bool real0 = o < s.M1 && c < s.C, real1 = o < s.M1 && c + 1 < s.C;
            const float *p0 = weight1 + (real0 ? ((size_t)o * s.C + c) * 9 : 0);
            const float *p1 = weight1 + (real1 ? ((size_t)o * s.C + c + 1) * 9 : 0);
            float w0[9], w1[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) w0[tap] = p0[tap], w1[tap] = p1[tap];
            unsigned *dst = s_wd + (((pr >> 2) * WS + row) << 2) + (pr & 3);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                dst[tap * GS * WS * 4] = (unsigned)head_bf16(real0 ? w0[tap] : 0.f) | (unsigned)head_bf16(real1 ? w1[tap] : 0.f) << 16;
        }
        __syncthreads();                                           // the chunk is there

        // ---- 3. conv1 over the chunk
#pragma unroll
        for (int ks = 0; ks < CH / 16; ++ks) {
            if (c0 + 16 * ks >= s.C) break;                        // a k-step of zeros only
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                uint4 av[N1];
#pragma unroll
                for (int n = 0; n < N1; ++n) av[n] = wb[(tap * GS + 2 * ks) * WS + 32 * n];
#pragma unroll
                for (int g = 0; g < kHeadG; ++g) {
                    const uint4 bv = hb[((tap / 3 + g) * kHeadHw + tap % 3) * PS + 2 * ks];
#pragma unroll
                    for (int n = 0; n < N1; ++n) acc[g][n] = head_mfma_bf16(av[n], bv, acc[g][n]);
                }
            }
        }
    }

    // ---- BatchNorm, LeakyReLU and the store
    const int gx = x0 + q;
#pragma unroll
    for (int n = 0; n < N1; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + head_row(n, r, hi);
            if (o < s.M1 && gx < s.W) {
                const float sc = scale[o], sh = shift[o];
#pragma unroll
                for (int g = 0; g < kHeadG; ++g) {
                    const int gy = y0 + wave * kHeadG + g;
                    if (gy < s.H)
                        head_store(out, s.out_kind, (((size_t)b * s.M1 + o) * s.H + gy) * s.W + gx, head_act(acc[g][n][r], sc, sh, s.slope));
                }
            }
        }
}

template <int N1, bool UP>
int stage_bf16_launch(const HeadShape &s, int tiles_x, int tiles_y, const float *fm, const float *x, const float *weight1,
                      const float *scale, const float *shift, void *out, hipStream_t st)
{
    constexpr size_t lds = StageBf16Lds<N1>::bytes;
    if (int e = head_raise_lds(reinterpret_cast<const void *>(&k_head_stage_bf16<N1, UP>), lds)) return e;
    const dim3 grid(tiles_x * ((s.M1 + 32 * N1 - 1) / (32 * N1)), tiles_y, s.B);
    hipLaunchKernelGGL((k_head_stage_bf16<N1, UP>), grid, dim3(kBlock), lds, st, s, tiles_x, fm, x, weight1, scale, shift, out);
    return check_launch("k_head_stage_bf16");
}

template <bool UP>
int stage_bf16_rows(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                    void *out, hipStream_t st)
{
    int tiles_x, tiles_y;
    if (int e = head_tiles(s, tiles_x, tiles_y)) return e;
    // Row blocks per workgroup: all of M1's (1, 2 or 4), halved while the launch would leave CUs without a workgroup -- each
    // workgroup of a split builds the halo again, which only pays where they would otherwise idle.  The sums do not depend on it.
    const long long tiles = (long long)tiles_x * tiles_y * s.B;
    const int blocks = (s.M1 + 31) / 32;
    int n1 = blocks > 2 ? 4 : blocks;
    while (n1 > 1 && tiles * ((blocks + n1 - 1) / n1) < kStageBf16Fill) n1 >>= 1;
    if (n1 == 4) return stage_bf16_launch<4, UP>(s, tiles_x, tiles_y, fm, x, weight1, scale, shift, out, st);
    if (n1 == 2) return stage_bf16_launch<2, UP>(s, tiles_x, tiles_y, fm, x, weight1, scale, shift, out, st);
    return stage_bf16_launch<1, UP>(s, tiles_x, tiles_y, fm, x, weight1, scale, shift, out, st);
}

// What pvv_head_forward calls for PVV_HEAD_STAGE | PVV_HEAD_STAGE_BF16, after its own checks (declared in head.hpp).
int head_stage_bf16_forward(const HeadShape &s, bool same_res, const float *fm, const float *x, const float *weight1,
                            const float *scale, const float *shift, void *out, hipStream_t st)
{
    return same_res ? stage_bf16_rows<false>(s, fm, x, weight1, scale, shift, out, st)
                    : stage_bf16_rows<true>(s, fm, x, weight1, scale, shift, out, st);
}

}  // namespace
