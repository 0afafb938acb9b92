// head.hpp -- PVNet's full-resolution output head in one launch (include/pvnet_vote.h, "PVNet output head"): the bilinear 2x
// upsample of the half-resolution feature map, the concatenation with the image, Conv3x3 + folded BatchNorm + LeakyReLU and the
// Conv1x1 with its bias.  Included at the end of pvnet_vote.hip, after head_tile.hpp -- the tile's
// shared pieces -- and the two modes' files: built with -ffp-contract=off, so the upsample rounds once per
// operation in the order written; the only fused multiply-adds are the ones the contract asks for, inside v_mfma_f32_32x32x2_f32
// and the one fmaf of the BatchNorm.  The numpy twin (tests/head_twin.py) gives the same bits.
// pvv_head_forward below also dispatches the modes of its `out_kind`: the bfloat16 matrix-core mode (head_bf16.hpp), the
// stage mode, PVNet's decoder stages (head_stage.hpp), and the stage's own bfloat16 mode (head_stage_bf16.hpp); all branch off
// after the checks they share.
//
// Reference behaviour restated: lib/networks/pvnet/resnet18.py:53-59, 90-94 of the reference.
#pragma once

namespace {

// One workgroup per (kHeadTh x kHeadTw output pixels, image); N1 / N2 = 32-row blocks of M1 / M2.  A wave owns kHeadG rows of 32
// pixels: kHeadG accumulators per row block, independent of each other, multiplied by one read of the weight operand.
//  1. The tile's halo (HeadHaloLane) of all C channels of the concatenated tensor -- the upsampled fm channels, then the image's,
//     zeros in the channel that fills an odd C -- is written to LDS once: wave w takes the channels c = w, w + 4, ..., its lanes
//     the positions.  weight2 is staged transposed.
//  2. Conv1: weight1 goes through LDS in chunks of kHeadKc values of k -- four channels -- as rows of kHeadKs floats, in two
//     buffers (the next chunk is loaded into registers before this one is multiplied and written after: one barrier per
//     chunk; each thread's share of a chunk has the same offsets in every chunk, computed once).  Each wave feeds its pixels --
//     read from the halo by address: per pair of channels the nine offsets of k = 2j + (lane >> 5) are constants of the lane
//     -- and the N1 row blocks to v_mfma_f32_32x32x2_f32: per output one accumulator from +0 to the last k, ascending.  The k
//     past 9 * C are zeros.
//  3. t = fmaf(acc, scale, shift), a = t > 0 ? t : t * slope go to LDS over the halo (after a barrier: every wave is done with
//     it), rows >= M1 as zeros; each wave reads back only the columns it wrote.
//  4. Conv2: the same instruction with K = M1 from bias2; the store rounds to the output type.
// Dynamic LDS: max(halo [Cpad][kHeadHalo], act [M1pad][kHeadPix]), wt [2][32*N1][kHeadKs], w2 [M1pad][32*N2 + 1].
template <int N1, int N2>
__global__ __launch_bounds__(kBlock) void k_head_forward(HeadShape s, const float *__restrict__ fm, const float *__restrict__ x,
                                                         const float *__restrict__ weight1, const float *__restrict__ scale,
                                                         const float *__restrict__ shift, const float *__restrict__ weight2,
                                                         const float *__restrict__ bias2, void *__restrict__ out)
{
    constexpr int MT1 = 32 * N1, MT2 = 32 * N2, WS2 = MT2 + 1;
    constexpr int NE = (MT1 * kHeadKc + kBlock - 1) / kBlock;      // elements of a weight chunk per thread
    extern __shared__ float s_head[];
    const int region = max(s.Cpad * kHeadHalo, s.M1pad * kHeadPix);
    float *s_halo = s_head, *s_act = s_head, *s_wt = s_head + region, *s_w2 = s_wt + 2 * MT1 * kHeadKs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, hi = lane >> 5;
    const int x0 = blockIdx.x * kHeadTw, y0 = blockIdx.y * kHeadTh, b = blockIdx.z;

    // ---- 1. the halo and weight2
    const float *fmb = fm + (size_t)b * s.fm_stride, *xb = x + (size_t)b * s.x_stride;
    const int plane = s.h * s.w, Plane = s.H * s.W;
    HeadHaloLane<true> halo;
    halo.init(s, x0, y0, lane);
#pragma unroll 2
    for (int c = wave; c < s.C2; c += 4) {
        const float *pl = fmb + (size_t)c * plane;
#pragma unroll
        for (int i = 0; i < halo.NP; ++i) {
            const float u = halo.up(pl, i);
            if (halo.in_halo(lane, i)) s_halo[c * kHeadHalo + lane + 64 * i] = halo.held(i, u);
        }
    }
    for (int c = s.C2 + wave; c < s.Cpad; c += 4) {                // the image's channels; zeros in the one that fills an odd C
        const bool real = c < s.C;
        const float *pl = xb + (size_t)(real ? c - s.C2 : 0) * Plane;
#pragma unroll
        for (int i = 0; i < halo.NP; ++i) {
            const float v = real ? halo.at(pl, i) : 0.f;
            if (halo.in_halo(lane, i)) s_halo[c * kHeadHalo + lane + 64 * i] = halo.held(i, v);
        }
    }
    for (int e = tid; e < s.M1pad * MT2; e += kBlock) {
        const int k = e % s.M1pad, o = e / s.M1pad;
        s_w2[k * WS2 + o] = (k < s.M1 && o < s.M2) ? weight2[(size_t)o * s.M1 + k] : 0.f;
    }

    // ---- 2. conv1
    int w_lds[NE], w_glb[NE], w_lim[NE];                           // this thread's elements of a chunk: s_wt[o][kl] = weight1[o][k0 + kl]
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = tid + i * kBlock, o = e / kHeadKc, kl = e - o * kHeadKc;
        w_lds[i] = min(o, MT1 - 1) * kHeadKs + kl, w_glb[i] = o * s.K + kl;
        w_lim[i] = (e < MT1 * kHeadKc && o < s.M1) ? s.K - kl : 0;  // the element is weight1's while k0 < w_lim; a zero otherwise
    }
    const int w_last = s.M1 * s.K - 1;
    float w_reg[NE];
    auto fetch = [&](int chunk) {                                  // every load is issued, at a valid address; none waits on a branch
        const int k0 = chunk * kHeadKc;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const float v = weight1[k0 < w_lim[i] ? w_glb[i] + k0 : w_last];
            w_reg[i] = k0 < w_lim[i] ? v : 0.f;
        }
    };
    auto put = [&](int chunk) {
        float *dst = s_wt + (chunk & 1) * MT1 * kHeadKs;
#pragma unroll
        for (int i = 0; i < NE; ++i)
            if (tid + i * kBlock < MT1 * kHeadKc) dst[w_lds[i]] = w_reg[i];
    };
    head_f16v acc[kHeadG][N1] = {};

    const int pix = wave * kHeadG * 32 + q;                        // this lane's pixel of its wave's first row; + 32 per row
    const float *window = s_halo + wave * kHeadG * kHeadHw + q;
    int koff[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) koff[j] = hi ? head_k_offset(2 * j + 1) : head_k_offset(2 * j);
    const int chunks = (s.Cpad + 3) / 4;
    fetch(0);
    put(0);
    for (int chunk = 0; chunk < chunks; ++chunk) {
        __syncthreads();                                           // this chunk (and the halo) is there; the last chunk's readers are done
        if (chunk + 1 < chunks) fetch(chunk + 1);                  // in flight while this chunk is multiplied
        head_conv1_chunk<N1>(s_wt + (chunk & 1) * MT1 * kHeadKs + q * kHeadKs + hi, window + 4 * chunk * kHeadHalo,
                             min(2, (s.Cpad - 4 * chunk) / 2), koff, acc);
        if (chunk + 1 < chunks) put(chunk + 1);                    // the other buffer: its readers passed this round's barrier
    }

    // ---- 3. BatchNorm and LeakyReLU into LDS, over the halo
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N1; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = head_row(n, r, hi);
            if (o < s.M1pad) {
                const float sc = o < s.M1 ? scale[o] : 0.f, sh = o < s.M1 ? shift[o] : 0.f;
#pragma unroll
                for (int g = 0; g < kHeadG; ++g)
                    s_act[o * kHeadPix + pix + 32 * g] = o < s.M1 ? head_act(acc[g][n][r], sc, sh, s.slope) : 0.f;
            }
        }
    __builtin_amdgcn_wave_barrier();                               // a wave reads only the columns it wrote: no workgroup barrier

    // ---- 4. conv2 and the store
    head_f16v acc2[kHeadG][N2];
#pragma unroll
    for (int n = 0; n < N2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = head_row(n, r, hi);
            const float bs = o < s.M2 ? bias2[o] : 0.f;
#pragma unroll
            for (int g = 0; g < kHeadG; ++g) acc2[g][n][r] = bs;
        }
    const float *ab = s_act + hi * kHeadPix + pix, *w2b = s_w2 + hi * WS2 + q;
    for (int kk = 0; kk < s.M1pad; kk += 2) {
        float av[N2];
#pragma unroll
        for (int a = 0; a < N2; ++a) av[a] = w2b[kk * WS2 + 32 * a];
#pragma unroll
        for (int g = 0; g < kHeadG; ++g) {
            const float bv = ab[kk * kHeadPix + 32 * g];
#pragma unroll
            for (int a = 0; a < N2; ++a) acc2[g][a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv, acc2[g][a], 0, 0, 0);
        }
    }
    const int gx = x0 + q;
#pragma unroll
    for (int g = 0; g < kHeadG; ++g) {
        const int gy = y0 + wave * kHeadG + g;
        if (gy < s.H && gx < s.W) {
#pragma unroll
            for (int n = 0; n < N2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = head_row(n, r, hi);
                    if (o < s.M2) head_store(out, s.out_kind, (((size_t)b * s.M2 + o) * s.H + gy) * s.W + gx, acc2[g][n][r]);
                }
        }
    }
}

template <int N1, int N2>
size_t head_lds_bytes(const HeadShape &s)
{
    const size_t region = std::max((size_t)s.Cpad * kHeadHalo, (size_t)s.M1pad * kHeadPix);
    return sizeof(float) * (region + 2 * (size_t)kHeadKs * 32 * N1 + (size_t)s.M1pad * (32 * N2 + 1));
}

// The checks the two entry points share; fills `s`.  M1 = M2 = 1 for the upsample alone.  `stage`: the stage mode's limits --
// M1 up to PVV_HEAD_STAGE_MAX_M, the output is [M1,H,W] (the caller passes M2 = 1) -- and with `same_res` H = h, W = w.
int head_shape(HeadShape &s, int B, int C2, int C0, int h, int w, int H, int W, int M1, int M2, long long fm_stride, long long x_stride,
               float slope, int out_kind, bool stage = false, bool same_res = false)
{
    if (B <= 0 || C2 <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || M1 <= 0 || M2 <= 0 || C0 < 0)
        return fail(PVV_E_ARG, "head: B, C2, h, w, H, W, M1, M2 must be positive and C0 not negative");
    if (B > 65535) return fail(PVV_E_ARG, "head: B > 65535: split the batch");
    if (stage && M1 > PVV_HEAD_STAGE_MAX_M) return fail(PVV_E_ARG, "head: a stage's M1 must be <= 128");
    if (!stage && (M1 > PVV_HEAD_MAX_M || M2 > PVV_HEAD_MAX_M)) return fail(PVV_E_ARG, "head: M1 and M2 must be <= 64");
    if (same_res && (H != h || W != w)) return fail(PVV_E_ARG, "head: with PVV_HEAD_SAME_RES H must be h and W must be w");
    if (!same_res && (H != 2ll * h || W != 2ll * w)) return fail(PVV_E_ARG, "head: H must be 2*h and W must be 2*w");
    const long long lim = 1ll << 31, P = (long long)H * W, C = (long long)C2 + C0;
    if (C2 * P >= lim || C0 * P >= lim || C * 9 >= lim || (long long)M2 * P >= lim || (long long)M1 * C * 9 >= lim ||
        (stage && (long long)M1 * P >= lim))
        return fail(PVV_E_ARG, "head: a per-image tensor has 2^31 elements or more (int32 indexing)");
    if (fm_stride < (long long)C2 * h * w || (C0 > 0 && x_stride < C0 * P))
        return fail(PVV_E_ARG, "head: an image stride of fm / x is smaller than its planes");
    if (out_kind != PVV_HEAD_OUT_F32 && out_kind != PVV_HEAD_OUT_F16 && out_kind != PVV_HEAD_OUT_BF16)
        return fail(PVV_E_ARG, "head: unknown output dtype code");
    s.B = B, s.C2 = C2, s.C0 = C0, s.h = h, s.w = w, s.H = H, s.W = W, s.M1 = M1, s.M2 = M2;
    s.C = (int)C, s.Cpad = (int)((C + 1) & ~1ll), s.K = (int)(9 * C), s.M1pad = (M1 + 1) & ~1;
    s.fm_stride = fm_stride, s.x_stride = x_stride;
    s.rh = (h > 1 && H > 1) ? (float)(h - 1) / (float)(H - 1) : 0.f;
    s.rw = (w > 1 && W > 1) ? (float)(w - 1) / (float)(W - 1) : 0.f;
    s.slope = slope, s.out_kind = out_kind;
    return PVV_OK;
}

template <int N1, int N2>
int head_launch(const HeadShape &s, const float *fm, const float *x, const float *weight1, const float *scale, const float *shift,
                const float *weight2, const float *bias2, void *out, hipStream_t st)
{
    const size_t lds = head_lds_bytes<N1, N2>(s);
    int tiles_x, tiles_y;
    if (int e = head_raise_lds(reinterpret_cast<const void *>(&k_head_forward<N1, N2>), lds)) return e;
    if (int e = head_tiles(s, tiles_x, tiles_y)) return e;
    const dim3 grid(tiles_x, tiles_y, s.B);
    hipLaunchKernelGGL((k_head_forward<N1, N2>), grid, dim3(kBlock), lds, st, s, fm, x, weight1, scale, shift, weight2, bias2, out);
    return check_launch("k_head_forward");
}

}  // namespace

PVV_EXPORT int pvv_head_forward(const float *d_fm, long long fm_image_stride, const float *d_x, long long x_image_stride,
                                const float *d_weight1, const float *d_scale, const float *d_shift, const float *d_weight2,
                                const float *d_bias2, int B, int C2, int C0, int h, int w, int H, int W, int M1, int M2,
                                float negative_slope, int out_kind, void *d_out, void *stream)
{
    HeadShape s;
    const int flags = out_kind & ~0xFF;
    const bool bf16 = flags == PVV_HEAD_COMPUTE_BF16;                 // any other bit above the dtype code stays and is refused with it
    const int stage_flags = flags & ~PVV_HEAD_STAGE_BF16;             // PVV_HEAD_STAGE_BF16 counts only beside PVV_HEAD_STAGE
    const bool stage = stage_flags == PVV_HEAD_STAGE || stage_flags == (PVV_HEAD_STAGE | PVV_HEAD_SAME_RES);
    const bool same_res = stage && (flags & PVV_HEAD_SAME_RES), stage_bf16 = stage && (flags & PVV_HEAD_STAGE_BF16);
    if (bf16 || stage) out_kind &= 0xFF;
    if (int e = head_shape(s, B, C2, C0, h, w, H, W, M1, stage ? 1 : M2, fm_image_stride, x_image_stride, negative_slope, out_kind,
                           stage, same_res))
        return e;
    if (!d_fm || (C0 > 0 && !d_x) || !d_weight1 || !d_scale || !d_shift || (!stage && (!d_weight2 || !d_bias2)) || !d_out)
        return fail(PVV_E_ARG, "head: NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    if (stage_bf16) return head_stage_bf16_forward(s, same_res, d_fm, d_x, d_weight1, d_scale, d_shift, d_out, st);
    if (stage) return head_stage_forward(s, same_res, d_fm, d_x, d_weight1, d_scale, d_shift, d_out, st);
    if (bf16) return head_bf16_forward(s, d_fm, d_x, d_weight1, d_scale, d_shift, d_weight2, d_bias2, d_out, st);
    return head_rows(M1, M2, [&](auto n1, auto n2) {
        return head_launch<decltype(n1)::value, decltype(n2)::value>(s, d_fm, d_x, d_weight1, d_scale, d_shift, d_weight2, d_bias2, d_out, st);
    });
}

PVV_EXPORT int pvv_head_upsample(const float *d_fm, long long fm_image_stride, int B, int C2, int h, int w, int H, int W, float *d_u,
                                 void *stream)
{
    HeadShape s;
    if (int e = head_shape(s, B, C2, 0, h, w, H, W, 1, 1, fm_image_stride, 0, 0.f, PVV_HEAD_OUT_F32)) return e;
    if (!d_fm || !d_u) return fail(PVV_E_ARG, "head: NULL device pointer");
    const long long total = (long long)B * C2 * H * W;
    if (total > (1ll << 28)) return fail(PVV_E_ARG, "head: the upsampled tensor has more than 2^28 elements");
    hipLaunchKernelGGL(k_head_upsample, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, d_fm, d_u);
    return check_launch("k_head_upsample");
}
