// head_stage.hpp -- PVNet's decoder stages (include/pvnet_vote.h, "PVNet decoder stage"): the stage mode of pvv_head_forward,
// PVV_HEAD_STAGE in `out_kind`.  A stage is the head's front half -- bilinear 2x upsample (or none, PVV_HEAD_SAME_RES), cat
// with the skip tensor, Conv3x3 + folded BatchNorm + LeakyReLU -- stored after the activation.  Included after head.hpp in
// pvnet_vote.hip: the same tile, the same device functions (head_axis's formula, head_store), the same instruction and so
// the same chain; what differs is that the halo goes through LDS in chunks of channels, so C2 + C0 has no limit, that up to
// four 32-row blocks of outputs are accumulated, and that the epilogue writes global memory.  The numpy twin
// (tests/decoder_twin.py) gives the same bits.
//
// Reference behaviour restated: lib/networks/pvnet/resnet18.py:31-51, 81-89 of the reference.
#pragma once

namespace {

constexpr int kStageWtChannels = kHeadKc / 9;                // channels of one staged chunk of weight1

// Channels of one halo chunk: a multiple of kStageWtChannels, and with the two weight buffers below 64 KiB -- static LDS, and
// two workgroups fit a CU's 160 KiB:  N1 = 4: 16 * 1360 + 2 * 128 * 148 = 59648 bytes;  N1 = 2: 32 * 1360 + 2 * 64 * 148 = 62464;
// N1 = 1: 32 * 1360 + 2 * 32 * 148 = 52992.
template <int N1> constexpr int stage_halo_channels() { return N1 == 4 ? 16 : 32; }

// One workgroup per (kHeadTh x kHeadTw output pixels, block of 32 * N1 output channels, image): blockIdx.x = tile along W +
// tiles * (block of output channels).  As k_head_forward up to its step 3, but:
//  1. A lane's halo positions, their neighbours and blend weights (UP) or their one source element (!UP), are computed once
//     per tile.  The halo of CH channels at a time is written to LDS -- wave w the chunk's channels w, w + 4, ... --: fm's
//     channels blended or copied, then the skip tensor's, then the zero channel that fills an odd C.  A position outside the
//     image loads element 0 and stores a zero.
//  2. weight1 goes through LDS in chunks of kHeadKc values of k, double-buffered as in k_head_forward; thread t stages
//     36 / TPR consecutive k of row t / TPR.  The accumulators run across all halo chunks: per output one chain from +0 over
//     k ascending.  A halo chunk is a whole number of weight chunks.
//  3. t = fmaf(acc, scale, shift), a = t > 0 ? t : t * slope goes to global memory: for one accumulator register the 32 lanes
//     of a half wave write 32 consecutive pixels of one row of one channel.
template <int N1, bool UP>
__global__ __launch_bounds__(kBlock, 2) void k_head_stage(HeadShape s, int tiles_x, const float *__restrict__ fm,
                                                          const float *__restrict__ x, const float *__restrict__ weight1,
                                                          const float *__restrict__ scale, const float *__restrict__ shift,
                                                          void *__restrict__ out)
{
    constexpr int MT1 = 32 * N1, CH = stage_halo_channels<N1>(), WPH = CH / kStageWtChannels;
    constexpr int TPR = N1 == 4 ? 2 : 4, NE = kHeadKc / TPR;      // threads per staged row, elements of a chunk per thread
    static_assert(TPR * NE == kHeadKc && MT1 * TPR <= kBlock && CH % kStageWtChannels == 0, "a thread stages whole shares of a row");
    __shared__ float s_halo[CH * kHeadHalo];
    __shared__ float s_wt[2 * MT1 * kHeadKs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hi = lane >> 5;
    const int mblock = blockIdx.x / tiles_x, o0 = mblock * MT1;
    const int x0 = (blockIdx.x - mblock * tiles_x) * kHeadTw, y0 = blockIdx.y * kHeadTh, b = blockIdx.z;

    // ---- 1. the lane's halo positions r = lane, lane + 64, ...
    constexpr int NP = (kHeadHalo + 63) / 64;
    const float *fmb = fm + (size_t)b * s.fm_stride, *xb = x + (size_t)b * s.x_stride;
    const int plane = s.h * s.w, Plane = s.H * s.W;
    int n00[UP ? NP : 1], n01[UP ? NP : 1], n10[UP ? NP : 1], n11[UP ? NP : 1], nx[NP];
    float hl0[UP ? NP : 1], hl1[UP ? NP : 1], wl0[UP ? NP : 1], wl1[UP ? NP : 1];
    bool inside[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int r = lane + 64 * i, hy = r / kHeadHw, gy = y0 - 1 + hy, gx = x0 - 1 + (r - hy * kHeadHw);
        inside[i] = r < kHeadHalo && gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
        nx[i] = inside[i] ? gy * s.W + gx : 0;
        if constexpr (UP) {
            const HeadAxis ay = head_axis(s.rh, inside[i] ? gy : 0, s.h), ax = head_axis(s.rw, inside[i] ? gx : 0, s.w);
            n00[i] = ay.i0 * s.w + ax.i0, n01[i] = ay.i0 * s.w + ax.i1, n10[i] = ay.i1 * s.w + ax.i0, n11[i] = ay.i1 * s.w + ax.i1;
            hl0[i] = ay.l0, hl1[i] = ay.l1, wl0[i] = ax.l0, wl1[i] = ax.l1;
        }
    }
    auto fill = [&](int c0) {                                      // the halo of channels c0 .. c0 + CH - 1, as far as Cpad
        const int n = min(CH, s.Cpad - c0);
        for (int cl = wave; cl < n; cl += 4) {
            const int c = c0 + cl;
            float v[NP];
            if (c < s.C2) {
                const float *pl = fmb + (size_t)c * plane;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    if constexpr (UP)
                        v[i] = hl0[i] * (wl0[i] * pl[n00[i]] + wl1[i] * pl[n01[i]]) + hl1[i] * (wl0[i] * pl[n10[i]] + wl1[i] * pl[n11[i]]);
                    else
                        v[i] = pl[nx[i]];
                }
            } else if (c < s.C) {
                const float *pl = xb + (size_t)(c - s.C2) * Plane;
#pragma unroll
                for (int i = 0; i < NP; ++i) v[i] = pl[nx[i]];
            } else {
#pragma unroll
                for (int i = 0; i < NP; ++i) v[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (lane + 64 * i < kHeadHalo) s_halo[cl * kHeadHalo + lane + 64 * i] = inside[i] ? v[i] : 0.f;
        }
    };

    // ---- 2. conv1.  This thread's share of a weight chunk: s_wt[row][part * NE + i] = weight1[o0 + row][k0 + part * NE + i]
    const int w_row = tid / TPR, w_part = (tid - w_row * TPR) * NE;
    const bool w_mine = w_row < MT1;
    const bool w_real = w_mine && o0 + w_row < s.M1;
    const int w_lds = min(w_row, MT1 - 1) * kHeadKs + w_part;
    const int w_glb = w_real ? (o0 + w_row) * s.K + w_part : 0;
    const int w_lim = w_real ? s.K - w_part : 0;                   // element i of chunk k0 is weight1's while k0 + i < w_lim
    const int w_last = s.M1 * s.K - 1;
    float w_reg[NE];
    auto fetch = [&](int chunk) {                                  // every load is issued, at a valid address; none waits on a branch
        const int k0 = chunk * kHeadKc;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const bool real = k0 + i < w_lim;
            const float v = weight1[real ? w_glb + k0 + i : w_last];
            w_reg[i] = real ? v : 0.f;
        }
    };
    auto put = [&](int chunk) {
        float *dst = s_wt + (chunk & 1) * MT1 * kHeadKs + w_lds;
        if (w_mine) {
#pragma unroll
            for (int i = 0; i < NE; ++i) dst[i] = w_reg[i];
        }
    };
    head_f16v acc[kHeadG][N1];
#pragma unroll
    for (int g = 0; g < kHeadG; ++g)
#pragma unroll
        for (int n = 0; n < N1; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][n][r] = 0.f;

    const float *window = s_halo + wave * kHeadG * kHeadHw + q;
    int koff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) koff[j] = hi ? head_k_offset(2 * j + 1) : head_k_offset(2 * j);
    const int chunks = (s.Cpad + kStageWtChannels - 1) / kStageWtChannels;
    fetch(0);
    put(0);
    for (int chunk = 0, in_halo = 0; chunk < chunks; ++chunk, ++in_halo) {
        if (in_halo == WPH || chunk == 0) {                        // the next CH channels of the halo
            if (chunk) __syncthreads();                            // every wave is done with the last ones
            fill(chunk * kStageWtChannels);
            in_halo = 0;
        }
        __syncthreads();                                           // this chunk and the halo are there; the last chunk's readers are done
        if (chunk + 1 < chunks) fetch(chunk + 1);                  // in flight while this chunk is multiplied
        const int pairs = min(2, (s.Cpad - kStageWtChannels * chunk) / 2);
        const float *wb = s_wt + (chunk & 1) * MT1 * kHeadKs + q * kHeadKs + hi;
        const float *hb = window + kStageWtChannels * in_halo * kHeadHalo;
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
                    for (int a = 0; a < N1; ++a) acc[g][a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv, acc[g][a], 0, 0, 0);
                }
            }
        }
        if (chunk + 1 < chunks) put(chunk + 1);                    // the other buffer: its readers passed this round's barrier
    }

    // ---- 3. BatchNorm, LeakyReLU and the store
    const int gx = x0 + q;
#pragma unroll
    for (int n = 0; n < N1; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + 32 * n + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (o < s.M1 && gx < s.W) {
                const float sc = scale[o], sh = shift[o];
#pragma unroll
                for (int g = 0; g < kHeadG; ++g) {
                    const int gy = y0 + wave * kHeadG + g;
                    if (gy < s.H) {
                        const float t = __builtin_fmaf(acc[g][n][r], sc, sh);
                        head_store(out, s.out_kind, (((size_t)b * s.M1 + o) * s.H + gy) * s.W + gx, t > 0.f ? t : t * s.slope);
                    }
                }
            }
        }
}

template <int N1, bool UP>
int stage_launch(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                 void *out, hipStream_t st)
{
    const int tiles_x = (s.W + kHeadTw - 1) / kHeadTw, mblocks = (s.M1 + 32 * N1 - 1) / (32 * N1);
    const dim3 grid(tiles_x * mblocks, (s.H + kHeadTh - 1) / kHeadTh, s.B);
    if (grid.y > 65535) return fail(PVV_E_ARG, "head: H is too large for one launch");
    hipLaunchKernelGGL((k_head_stage<N1, UP>), grid, dim3(kBlock), 0, st, s, tiles_x, fm, x, weight1, scale, shift, out);
    return check_launch("k_head_stage");
}

template <bool UP>
int stage_rows(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
               void *out, hipStream_t st)
{
    // Four row blocks with the upsample's neighbours and weights of six positions alive spill (48 bytes of scratch per lane at
    // 256 VGPRs): there M1 > 64 is split over two workgroups of two row blocks, each of which builds the halo.
    if constexpr (!UP)
        if (s.M1 > 64) return stage_launch<4, UP>(s, fm, x, weight1, scale, shift, out, st);
    if (s.M1 > 32) return stage_launch<2, UP>(s, fm, x, weight1, scale, shift, out, st);
    return stage_launch<1, UP>(s, fm, x, weight1, scale, shift, out, st);
}

int head_stage_forward(const HeadShape &s, bool same_res, const float *fm, const float *x, const float *weight1, const float *scale,
                       const float *shift, void *out, hipStream_t st)
{
    return same_res ? stage_rows<false>(s, fm, x, weight1, scale, shift, out, st)
                    : stage_rows<true>(s, fm, x, weight1, scale, shift, out, st);
}

}  // namespace
