// head_stage.hpp -- PVNet's decoder stages (include/pvnet_vote.h, "PVNet decoder stage"): the stage mode of pvv_head_forward,
// PVV_HEAD_STAGE in `out_kind`.  A stage is the head's front half -- bilinear 2x upsample (or none, PVV_HEAD_SAME_RES), cat
// with the skip tensor, Conv3x3 + folded BatchNorm + LeakyReLU -- stored after the activation.  On the head's tile
// (head_tile.hpp, included in front of this file in pvnet_vote.hip): the same halo positions, the same conv1 chunk and so the
// same chain as k_head_forward; what is this file's own is that the halo goes through LDS in chunks of channels, so C2 + C0
// has no limit, that up to four 32-row blocks of outputs are accumulated, and that the epilogue writes global memory.  The
// numpy twin (tests/decoder_twin.py) gives the same bits.
//
// Reference behaviour restated: lib/networks/pvnet/resnet18.py:31-51, 81-89 of the reference.
#pragma once

namespace {

constexpr int kStageWtChannels = kHeadKc / 9;                // channels of one staged chunk of weight1

// Channels of one halo chunk: a multiple of kStageWtChannels, and with the two weight buffers below 64 KiB -- static LDS, and
// two workgroups fit a CU's 160 KiB:  N1 = 4: 16 * 1360 + 2 * 128 * 148 = 59648 bytes;  N1 = 2: 32 * 1360 + 2 * 64 * 148 = 62464;
// N1 = 1: 32 * 1360 + 2 * 32 * 148 = 52992.
template <int N1> constexpr int stage_halo_channels() { return N1 == 4 ? 16 : 32; }

// A thread's share of a staged chunk of weight1 -- kHeadKc values of k of the MT1 rows from o0 on, as rows of kHeadKs floats --:
// TPR threads per row, kHeadKc / TPR consecutive k each, so s_wt[row][part + i] = weight1[o0 + row][k0 + part + i]; rows past M1
// and k past K are zeros.  fetch() loads the share into registers -- every load is issued, at a valid address; none waits on a
// branch -- and put() writes it to the chunk's buffer of the two.  A struct, not lambdas over locals: beside head_conv1_chunk
// the lambdas' form made conv4s 0.4 % slower than before the tile was shared (profiles/head_tile_refactor_ab.json, session 4).
template <int MT1, int TPR>
struct StageWeightShare {
    static constexpr int NE = kHeadKc / TPR;
    static_assert(TPR * NE == kHeadKc && MT1 * TPR <= kBlock, "a thread stages a whole share of one row");
    int lds, glb, lim, last;          // element i of chunk k0 is weight1's while k0 + i < lim
    bool mine;
    float reg[NE];

    __device__ __forceinline__ void init(const HeadShape &s, int o0, int tid)
    {
        const int row = tid / TPR, part = (tid - row * TPR) * NE;
        mine = row < MT1;
        const bool real = mine && o0 + row < s.M1;
        lds = min(row, MT1 - 1) * kHeadKs + part;
        glb = real ? (o0 + row) * s.K + part : 0;
        lim = real ? s.K - part : 0;
        last = s.M1 * s.K - 1;
    }
    __device__ __forceinline__ void fetch(const float *__restrict__ weight1, int chunk)
    {
        const int k0 = chunk * kHeadKc;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const bool real = k0 + i < lim;
            const float v = weight1[real ? glb + k0 + i : last];
            reg[i] = real ? v : 0.f;
        }
    }
    __device__ __forceinline__ void put(float *s_wt, int chunk) const
    {
        float *dst = s_wt + (chunk & 1) * MT1 * kHeadKs + lds;
        if (mine) {
#pragma unroll
            for (int i = 0; i < NE; ++i) dst[i] = reg[i];
        }
    }
};

// One workgroup per (kHeadTh x kHeadTw output pixels, block of 32 * N1 output channels, image): blockIdx.x = tile along W +
// tiles * (block of output channels).  As k_head_forward up to its step 3, but:
//  1. The halo (HeadHaloLane<UP>: without the upsample a position has its one source element) of CH channels at a time is
//     written to LDS -- wave w the chunk's channels w, w + 4, ... --: fm's channels blended or copied, then the skip tensor's,
//     then the zero channel that fills an odd C.
//  2. weight1 goes through LDS in chunks of kHeadKc values of k, double-buffered as in k_head_forward; thread t stages
//     36 / TPR consecutive k of row t / TPR (StageWeightShare).  The accumulators run across all halo chunks: per output one
//     chain from +0 over k ascending.  A halo chunk is a whole number of weight chunks.
//  3. t = fmaf(acc, scale, shift), a = t > 0 ? t : t * slope goes to global memory: for one accumulator register the 32 lanes
//     of a half wave write 32 consecutive pixels of one row of one channel.
template <int N1, bool UP>
__global__ __launch_bounds__(kBlock, 2) void k_head_stage(HeadShape s, int tiles_x, const float *__restrict__ fm,
                                                          const float *__restrict__ x, const float *__restrict__ weight1,
                                                          const float *__restrict__ scale, const float *__restrict__ shift,
                                                          void *__restrict__ out)
{
    constexpr int MT1 = 32 * N1, CH = stage_halo_channels<N1>(), WPH = CH / kStageWtChannels;
    static_assert(CH % kStageWtChannels == 0, "a halo chunk is a whole number of weight chunks");
    __shared__ float s_halo[CH * kHeadHalo];
    __shared__ float s_wt[2 * MT1 * kHeadKs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hi = lane >> 5;
    const int mblock = blockIdx.x / tiles_x, o0 = mblock * MT1;
    const int x0 = (blockIdx.x - mblock * tiles_x) * kHeadTw, y0 = blockIdx.y * kHeadTh, b = blockIdx.z;

    // ---- 1. the halo
    const float *fmb = fm + (size_t)b * s.fm_stride, *xb = x + (size_t)b * s.x_stride;
    const int plane = s.h * s.w, Plane = s.H * s.W;
    HeadHaloLane<UP> halo;
    halo.init(s, x0, y0, lane);
    auto fill = [&](int c0) {                                      // the halo of channels c0 .. c0 + CH - 1, as far as Cpad
        const int n = min(CH, s.Cpad - c0);
        for (int cl = wave; cl < n; cl += 4) {
            const int c = c0 + cl;
            float v[halo.NP];
            if (c < s.C2) {
                const float *pl = fmb + (size_t)c * plane;
#pragma unroll
                for (int i = 0; i < halo.NP; ++i) {
                    if constexpr (UP) v[i] = halo.up(pl, i);
                    else v[i] = halo.at(pl, i);
                }
            } else if (c < s.C) {
                const float *pl = xb + (size_t)(c - s.C2) * Plane;
#pragma unroll
                for (int i = 0; i < halo.NP; ++i) v[i] = halo.at(pl, i);
            } else {
#pragma unroll
                for (int i = 0; i < halo.NP; ++i) v[i] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < halo.NP; ++i)
                if (halo.in_halo(lane, i)) s_halo[cl * kHeadHalo + lane + 64 * i] = halo.held(i, v[i]);
        }
    };

    // ---- 2. conv1
    StageWeightShare<MT1, N1 == 4 ? 2 : 4> wt;
    wt.init(s, o0, tid);
    head_f16v acc[kHeadG][N1] = {};

    const float *window = s_halo + wave * kHeadG * kHeadHw + q;
    int koff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) koff[j] = hi ? head_k_offset(2 * j + 1) : head_k_offset(2 * j);
    const int chunks = (s.Cpad + kStageWtChannels - 1) / kStageWtChannels;
    wt.fetch(weight1, 0);
    wt.put(s_wt, 0);
    for (int chunk = 0, in_halo = 0; chunk < chunks; ++chunk, ++in_halo) {
        if (in_halo == WPH || chunk == 0) {                        // the next CH channels of the halo
            if (chunk) __syncthreads();                            // every wave is done with the last ones
            fill(chunk * kStageWtChannels);
            in_halo = 0;
        }
        __syncthreads();                                           // this chunk and the halo are there; the last chunk's readers are done
        if (chunk + 1 < chunks) wt.fetch(weight1, chunk + 1);                  // in flight while this chunk is multiplied
        head_conv1_chunk<N1>(s_wt + (chunk & 1) * MT1 * kHeadKs + q * kHeadKs + hi, window + kStageWtChannels * in_halo * kHeadHalo,
                             min(2, (s.Cpad - kStageWtChannels * chunk) / 2), koff, acc);
        if (chunk + 1 < chunks) wt.put(s_wt, chunk + 1);                    // the other buffer: its readers passed this round's barrier
    }

    // ---- 3. BatchNorm, LeakyReLU and the store
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
int stage_launch(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                 void *out, hipStream_t st)
{
    int tiles_x, tiles_y;
    if (int e = head_tiles(s, tiles_x, tiles_y)) return e;
    const dim3 grid(tiles_x * ((s.M1 + 32 * N1 - 1) / (32 * N1)), tiles_y, s.B);
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
