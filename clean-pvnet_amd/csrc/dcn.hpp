// dcn.hpp -- DCNv2 modulated deformable convolution, forward (include/pvnet_vote.h, "Modulated deformable convolution").
// Included at the end of pvnet_vote.hip: built with -ffp-contract=off, so the sampling below rounds once per operation in the
// order written; the only fused multiply-adds are the ones the contract asks for, inside v_mfma_f32_32x32x2_f32.  The numpy
// twin (tests/dcn_twin.py) gives the same bits.
//
// Reference behaviour restated (paths relative to /root/reference):
//   I = lib/csrc/dcn_v2/src/cuda/dcn_v2_im2col_cuda.cu        C = lib/csrc/dcn_v2/src/cuda/dcn_v2_cuda.cu
#pragma once

namespace {

constexpr int kDcnPix = 128;          // output pixels of a workgroup: 32 per wave
constexpr int kDcnKc = 32;            // rows of the column tile in LDS (k values per chunk); even: the MFMA takes two
constexpr int kDcnCacheTaps = 9;      // kh*kw up to which the per-(tap, pixel) sampling state of a tile is kept in LDS
constexpr int kDcnTapWords = 7;

static_assert(kBlock == 2 * kDcnPix && kDcnPix == 4 * 32 && kDcnKc % 2 == 0, "4 waves of 32 pixels; two threads per pixel gather");

struct DcnShape {
    int B, C, H, W, M, kh, kw, sh, sw, ph, pw, dh, dw, dg;
    int Ho, Wo, P, KK, Cg, K;         // P = Ho*Wo, KK = kh*kw, Cg = C/dg, K = C*KK
    long long off_stride, mask_stride;   // elements between two images of offset / mask
};

// What one (deformable group, tap, output pixel) contributes to every channel of the group: the four blend weights, the mask,
// the flat index of the upper left neighbour in a plane and which of the four neighbours lie inside it (bit 0..3 = v1..v4).
struct DcnTap { float w1, w2, w3, w4, mask; int base, in; };

// I:143-180 and I:28-50 for tap (i, j) at output pixel (y, x).  A sample outside (-1, H) x (-1, W) -- a NaN offset too -- has no
// neighbour and zero weights, which blends to the +0 of I:176.
__device__ __forceinline__ DcnTap dcn_tap(const DcnShape &s, int y, int x, int i, int j, float off_h, float off_w, float mask)
{
    DcnTap t;
    t.w1 = t.w2 = t.w3 = t.w4 = 0.f, t.mask = mask, t.base = 0, t.in = 0;
    const float h = (float)(y * s.sh - s.ph + i * s.dh) + off_h;
    const float w = (float)(x * s.sw - s.pw + j * s.dw) + off_w;
    if (h > -1.f && w > -1.f && h < (float)s.H && w < (float)s.W) {
        const float hf = floorf(h), wf = floorf(w);
        const int h0 = (int)hf, w0 = (int)wf;
        const float lh = h - hf, lw = w - wf, hh = 1.f - lh, hw = 1.f - lw;
        t.w1 = hh * hw, t.w2 = hh * lw, t.w3 = lh * hw, t.w4 = lh * lw;
        t.base = h0 * s.W + w0;
        const bool top = h0 >= 0, left = w0 >= 0, bottom = h0 + 1 <= s.H - 1, right = w0 + 1 <= s.W - 1;
        t.in = (top && left ? 1 : 0) | (top && right ? 2 : 0) | (bottom && left ? 4 : 0) | (bottom && right ? 8 : 0);
    }
    return t;
}

// The column element of one channel plane (I:37-52, I:189): the blend summed left to right, then the mask.
__device__ __forceinline__ float dcn_col(const float *__restrict__ plane, int W, const DcnTap &t)
{
    const float v1 = (t.in & 1) ? plane[t.base] : 0.f;
    const float v2 = (t.in & 2) ? plane[t.base + 1] : 0.f;
    const float v3 = (t.in & 4) ? plane[t.base + W] : 0.f;
    const float v4 = (t.in & 8) ? plane[t.base + W + 1] : 0.f;
    const float val = ((t.w1 * v1 + t.w2 * v2) + t.w3 * v3) + t.w4 * v4;
    return val * t.mask;
}

// dcn_tap for group g, tap t at pixel p of image b, with its offsets and mask read (I:162-175).  p < P.
__device__ __forceinline__ DcnTap dcn_tap_at(const DcnShape &s, const float *__restrict__ offset, const float *__restrict__ mask, int b,
                                             int g, int t, int p)
{
    const float *o = offset + (size_t)b * s.off_stride + ((size_t)g * 2 * s.KK + 2 * t) * s.P + p;
    const float m = mask[(size_t)b * s.mask_stride + ((size_t)g * s.KK + t) * s.P + p];
    const int y = p / s.Wo, i = t / s.kw;
    return dcn_tap(s, y, p - y * s.Wo, i, t - i * s.kw, o[0], o[s.P], m);
}

// One thread per element of col [B, K, P].
__global__ __launch_bounds__(kBlock) void k_dcn_columns(DcnShape s, const float *__restrict__ input, const float *__restrict__ offset,
                                                        const float *__restrict__ mask, float *__restrict__ col)
{
    const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (long long)s.B * s.K * s.P) return;
    const int p = (int)(idx % s.P);
    const int k = (int)(idx / s.P % s.K), b = (int)(idx / s.P / s.K);
    const int c = k / s.KK, t = k - c * s.KK;
    const DcnTap tap = dcn_tap_at(s, offset, mask, b, c / s.Cg, t, p);
    col[idx] = dcn_col(input + ((size_t)b * s.C + c) * s.H * s.W, s.W, tap);
}

typedef float dcn_f16v __attribute__((ext_vector_type(16)));

// One workgroup per (128 output pixels, 32 * NACC output channels, image).  Per deformable group the sampling state of the
// tile's (tap, pixel) pairs goes to LDS once (`cache`; computed per element otherwise); then, per chunk of kDcnKc values of k:
// every thread gathers and blends its share of the column tile into LDS and stages the [32 * NACC, chunk] slice of the weights
// transposed, and each wave feeds its 32 pixels and the NACC row blocks to v_mfma_f32_32x32x2_f32 -- per output one
// accumulator from the bias to the last k, in ascending k (the instruction is fma(a_k1, b_k1, fma(a_k0, b_k0, c))).  A chunk
// of odd length is filled with one zero row, rows of channels >= M and columns of pixels >= P are zeros.
// Dynamic LDS: col [kDcnKc][kDcnPix], wt [kDcnKc][32 * NACC + 1], then tap words [kDcnTapWords][KK][kDcnPix] when `cache`.
template <int NACC>
__global__ __launch_bounds__(kBlock) void k_dcn_forward(DcnShape s, int cache, const float *__restrict__ input,
                                                        const float *__restrict__ weight, const float *__restrict__ bias,
                                                        const float *__restrict__ offset, const float *__restrict__ mask,
                                                        float *__restrict__ out)
{
    constexpr int MT = 32 * NACC, WS = MT + 1;
    extern __shared__ float s_dcn[];
    float *s_col = s_dcn, *s_wt = s_col + kDcnKc * kDcnPix, *s_tap = s_wt + kDcnKc * WS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * kDcnPix, o0 = blockIdx.y * MT, b = blockIdx.z;
    const int pl = tid & (kDcnPix - 1), half = tid >> 7;          // the gather's pixel and which rows of a chunk (even / odd)
    const int pg = p0 + pl;
    const int tap_stride = s.KK * kDcnPix;

    dcn_f16v acc[NACC];
#pragma unroll
    for (int n = 0; n < NACC; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + 32 * n + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            acc[n][r] = (bias && o < s.M) ? bias[o] : 0.f;
        }

    for (int g = 0; g < s.dg; ++g) {
        if (cache) {                                               // (the last group's readers passed the barrier before their MFMAs)
            for (int e = tid; e < tap_stride; e += kBlock) {
                const int t = e / kDcnPix, q = e - t * kDcnPix;
                DcnTap tap;
                tap.w1 = tap.w2 = tap.w3 = tap.w4 = tap.mask = 0.f, tap.base = tap.in = 0;
                if (p0 + q < s.P) tap = dcn_tap_at(s, offset, mask, b, g, t, p0 + q);
                s_tap[e] = tap.w1, s_tap[tap_stride + e] = tap.w2, s_tap[2 * tap_stride + e] = tap.w3, s_tap[3 * tap_stride + e] = tap.w4;
                s_tap[4 * tap_stride + e] = tap.mask;
                s_tap[5 * tap_stride + e] = __int_as_float(tap.base), s_tap[6 * tap_stride + e] = __int_as_float(tap.in);
            }
        }
        const int kgroup = s.Cg * s.KK;                            // the group's k values: global k = g * kgroup + kg
        int cl = half / s.KK, t = half - cl * s.KK;                // this thread's next row kg = kg0 + half, + 2, ...: channel and tap
        for (int kg0 = 0; kg0 < kgroup; kg0 += kDcnKc) {
            const int n = min(kDcnKc, kgroup - kg0), npad = (n + 1) & ~1;
            __syncthreads();                                       // the taps are there; the last chunk's MFMAs are done
            for (int e = tid; e < kDcnKc * MT; e += kBlock) {      // weights, transposed: s_wt[row][channel]
                const int kl = e % kDcnKc, ol = e / kDcnKc;
                const int o = o0 + ol;
                s_wt[kl * WS + ol] = (kl < n && o < s.M) ? weight[(size_t)o * s.K + (size_t)g * kgroup + kg0 + kl] : 0.f;
            }
            for (int kl = half; kl < npad; kl += 2) {              // columns: s_col[row][pixel]
                float v = 0.f;
                if (kl < n) {
                    if (pg < s.P) {
                        DcnTap tap;
                        if (cache) {
                            const float *q = s_tap + t * kDcnPix + pl;
                            tap.w1 = q[0], tap.w2 = q[tap_stride], tap.w3 = q[2 * tap_stride], tap.w4 = q[3 * tap_stride];
                            tap.mask = q[4 * tap_stride];
                            tap.base = __float_as_int(q[5 * tap_stride]), tap.in = __float_as_int(q[6 * tap_stride]);
                        } else {
                            tap = dcn_tap_at(s, offset, mask, b, g, t, pg);
                        }
                        v = dcn_col(input + ((size_t)b * s.C + (size_t)g * s.Cg + cl) * s.H * s.W, s.W, tap);
                    }
                    t += 2;
                    while (t >= s.KK) t -= s.KK, ++cl;
                }
                s_col[kl * kDcnPix + pl] = v;
            }
            __syncthreads();
            const float *cb = s_col + (lane >> 5) * kDcnPix + wave * 32 + (lane & 31);
            const float *wb = s_wt + (lane >> 5) * WS + (lane & 31);
            for (int kk = 0; kk < npad; kk += 2) {
                const float bv = cb[kk * kDcnPix];
#pragma unroll
                for (int a = 0; a < NACC; ++a)
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[kk * WS + 32 * a], bv, acc[a], 0, 0, 0);
            }
        }
    }

    const int p = p0 + wave * 32 + (lane & 31);
    if (p < s.P) {
#pragma unroll
        for (int n = 0; n < NACC; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + 32 * n + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (o < s.M) out[((size_t)b * s.M + o) * s.P + p] = acc[n][r];
            }
    }
}

template <int NACC>
size_t dcn_lds_bytes(int cache, int KK)
{
    return sizeof(float) * ((size_t)kDcnKc * kDcnPix + (size_t)kDcnKc * (32 * NACC + 1) + (cache ? (size_t)kDcnTapWords * KK * kDcnPix : 0));
}

// The checks the two entry points share; fills `s`.  M = 1 for the columns.
int dcn_shape(DcnShape &s, int B, int C, int H, int W, int M, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg,
              long long off_stride, long long mask_stride)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || M <= 0) return fail(PVV_E_ARG, "dcn: B, C, H, W, M must be positive");
    if (B > 65535) return fail(PVV_E_ARG, "dcn: B > 65535: split the batch");
    if (H > (1 << 24) || W > (1 << 24)) return fail(PVV_E_ARG, "dcn: H, W must be <= 2^24 (the range test compares with float(H), float(W))");
    if (kh <= 0 || kw <= 0 || kh > 64 || kw > 64) return fail(PVV_E_ARG, "dcn: kh, kw must lie in [1, 64]");
    if (sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || ph < 0 || pw < 0) return fail(PVV_E_ARG, "dcn: stride and dilation must be positive, padding not negative");
    if (sh > 65535 || sw > 65535 || dh > 65535 || dw > 65535 || ph > 65535 || pw > 65535) return fail(PVV_E_ARG, "dcn: stride, padding, dilation must be <= 65535");
    if (dg <= 0 || C % dg != 0) return fail(PVV_E_ARG, "dcn: deformable_groups must be positive and divide C");
    const long long nh = (long long)H + 2ll * ph - ((long long)dh * (kh - 1) + 1), nw = (long long)W + 2ll * pw - ((long long)dw * (kw - 1) + 1);
    if (nh < 0 || nw < 0) return fail(PVV_E_ARG, "dcn: the kernel is larger than the padded input");
    const long long Ho = nh / sh + 1, Wo = nw / sw + 1, P = Ho * Wo, KK = (long long)kh * kw, K = (long long)C * KK;
    const long long lim = 1ll << 31;
    if ((long long)H * W >= lim || (long long)C * H * W >= lim || P >= lim || K >= lim || (long long)M * K >= lim ||
        (long long)M * P >= lim || (long long)dg * 2 * KK * P >= lim)
        return fail(PVV_E_ARG, "dcn: a per-image tensor has 2^31 elements or more (int32 indexing)");
    if ((Ho - 1) * sh + (long long)(kh - 1) * dh >= lim / 2 || (Wo - 1) * sw + (long long)(kw - 1) * dw >= lim / 2)
        return fail(PVV_E_ARG, "dcn: sampling positions overflow int32");
    if (off_stride < dg * 2 * KK * P || mask_stride < dg * KK * P)
        return fail(PVV_E_ARG, "dcn: an image stride of offset / mask is smaller than its image");
    s.B = B, s.C = C, s.H = H, s.W = W, s.M = M, s.kh = kh, s.kw = kw, s.sh = sh, s.sw = sw, s.ph = ph, s.pw = pw, s.dh = dh, s.dw = dw,
    s.dg = dg, s.Ho = (int)Ho, s.Wo = (int)Wo, s.P = (int)P, s.KK = (int)KK, s.Cg = C / dg, s.K = (int)K;
    s.off_stride = off_stride, s.mask_stride = mask_stride;
    return PVV_OK;
}

template <int NACC>
int dcn_launch(const DcnShape &s, const float *input, const float *weight, const float *bias, const float *offset, const float *mask,
               float *out, hipStream_t st)
{
    const int cache = s.KK <= kDcnCacheTaps;
    const dim3 grid((s.P + kDcnPix - 1) / kDcnPix, (s.M + 32 * NACC - 1) / (32 * NACC), s.B);
    if (grid.y > 65535) return fail(PVV_E_ARG, "dcn: M is too large for one launch");
    hipLaunchKernelGGL(k_dcn_forward<NACC>, grid, dim3(kBlock), dcn_lds_bytes<NACC>(cache, s.KK), st, s, cache, input, weight, bias, offset,
                       mask, out);
    return check_launch("k_dcn_forward");
}

}  // namespace

PVV_EXPORT int pvv_dcn_forward(const float *d_input, const float *d_weight, const float *d_bias, const float *d_offset,
                               long long offset_image_stride, const float *d_mask, long long mask_image_stride, int B, int C, int H,
                               int W, int M, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                               int deformable_groups, float *d_out, void *stream)
{
    DcnShape s;
    if (int e = dcn_shape(s, B, C, H, W, M, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, deformable_groups, offset_image_stride,
                          mask_image_stride))
        return e;
    if (!d_input || !d_weight || !d_offset || !d_mask || !d_out) return fail(PVV_E_ARG, "dcn: NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    if (M > 64) return dcn_launch<4>(s, d_input, d_weight, d_bias, d_offset, d_mask, d_out, st);
    if (M > 32) return dcn_launch<2>(s, d_input, d_weight, d_bias, d_offset, d_mask, d_out, st);
    return dcn_launch<1>(s, d_input, d_weight, d_bias, d_offset, d_mask, d_out, st);
}

PVV_EXPORT int pvv_dcn_columns(const float *d_input, const float *d_offset, long long offset_image_stride, const float *d_mask,
                               long long mask_image_stride, int B, int C, int H, int W, int kh, int kw, int stride_h, int stride_w,
                               int pad_h, int pad_w, int dil_h, int dil_w, int deformable_groups, float *d_col, void *stream)
{
    DcnShape s;
    if (int e = dcn_shape(s, B, C, H, W, 1, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, deformable_groups, offset_image_stride,
                          mask_image_stride))
        return e;
    if (!d_input || !d_offset || !d_mask || !d_col) return fail(PVV_E_ARG, "dcn: NULL device pointer");
    const long long total = (long long)s.B * s.K * s.P;
    if (total >= (1ll << 31)) return fail(PVV_E_ARG, "dcn: the column tensor has 2^31 elements or more");
    hipLaunchKernelGGL(k_dcn_columns, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, d_input,
                       d_offset, d_mask, d_col);
    return check_launch("k_dcn_columns");
}
