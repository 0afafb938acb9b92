// dcn_train.hpp -- DCNv2 modulated deformable convolution, backward (include/pvnet_vote.h, "Modulated deformable convolution,
// backward").  Included at the end of pvnet_vote.hip after dcn.hpp, whose DcnShape, dcn_shape, dcn_tap, dcn_tap_at and dcn_col it
// reuses: built with -ffp-contract=off, so every line below rounds once per operation in the order written, and the only fused
// multiply-adds are the ones the contract asks for, inside v_mfma_f32_32x32x2_f32.  Every gradient is the same bits on every
// run: no float atomic anywhere; the one scatter (grad_input) adds integers.  tests/dcn_train_twin.py is this file in numpy.
//
// Reference behaviour restated (paths relative to the reference's checkout):
//   I = lib/csrc/dcn_v2/src/cuda/dcn_v2_im2col_cuda.cu        C = lib/csrc/dcn_v2/src/cuda/dcn_v2_cuda.cu
#pragma once

namespace {

constexpr int kDcnSlab = 512;         // S: pixels of one grad_weight chain (PVV_DCN_SLAB)
constexpr int kDcnGwPix = 32;         // pixels of a slab staged in LDS at a time
constexpr int kDcnGwK = 128;          // k values of a grad_weight / gcol workgroup: 32 per wave
constexpr int kDcnFixBits = 40;       // a contribution to grad_input is a multiple of 2^(e_b - 40)
constexpr int kDcnScTy = 8, kDcnScTx = 32;          // the scatter's tile of output pixels: one per thread
constexpr int kDcnScHalo = 4;                       // rows / columns of the input kept in LDS around the tile's undeformed footprint
constexpr size_t kDcnScLdsBytes = 56 * 1024;        // LDS the scatter's windows may take
constexpr long long kDcnBwdDefaultBytes = 256ll << 20;   // what the per-image parts of a default workspace may take (one image at least)
constexpr long long kDcnMaxTapPixels = 1ll << 22;        // kh*kw*P up to which the backward runs: the int64 sums cannot overflow

static_assert(kDcnScTy * kDcnScTx == kBlock, "one thread per pixel of the scatter's tile");
static_assert(PVV_DCN_SLAB == kDcnSlab && kDcnSlab % kDcnGwPix == 0 && kDcnGwPix % 2 == 0 && kBlock == 2 * kDcnGwK, "the contract's S");

// The workspace: fixed parts, then per-image parts for `chunk` images at a time.  Byte offsets, every part 256-byte aligned.
struct DcnBwdLayout {
    int chunk, nslab;
    size_t wacc, bacc, maxbits, gcol, part, plane, total;     // f64 [M,K]; f64 [M]; u32 [chunk]; f32 [chunk,K,P]; f32 [chunk,nslab,M,K]; i64 [chunk,C,H,W]
    size_t fixed, per_image;
};

inline size_t dcn_up256(size_t n) { return (n + 255) & ~(size_t)255; }

void dcn_bwd_layout(const DcnShape &s, int chunk, DcnBwdLayout &L)
{
    L.nslab = (s.P + kDcnSlab - 1) / kDcnSlab;
    const size_t gcol = dcn_up256(sizeof(float) * (size_t)s.K * s.P), part = dcn_up256(sizeof(float) * (size_t)L.nslab * s.M * s.K),
                 plane = dcn_up256(sizeof(long long) * (size_t)s.C * s.H * s.W);
    L.fixed = dcn_up256(sizeof(double) * (size_t)s.M * s.K) + dcn_up256(sizeof(double) * (size_t)s.M) + dcn_up256(sizeof(unsigned) * 65536);
    L.per_image = gcol + part + plane;
    L.chunk = chunk;
    L.wacc = 0;
    L.bacc = L.wacc + dcn_up256(sizeof(double) * (size_t)s.M * s.K);
    L.maxbits = L.bacc + dcn_up256(sizeof(double) * (size_t)s.M);
    L.gcol = L.fixed;
    L.part = L.gcol + gcol * chunk;
    L.plane = L.part + part * chunk;
    L.total = L.plane + plane * chunk;
}

// The checks the two backward entry points add to dcn_shape's.
int dcn_bwd_shape(const DcnShape &s)
{
    if ((long long)s.K * s.P >= (1ll << 31) - kBlock || (long long)s.C * s.H * s.W >= (1ll << 31) - kBlock)   // (a grid's last block counts past the end in int32)
        return fail(PVV_E_ARG, "dcn backward: an image's column gradient or its input has 2^31 elements or more");
    if (s.K > 65535 * kDcnGwK) return fail(PVV_E_ARG, "dcn backward: C*kh*kw is too large for one launch");
    if ((long long)s.KK * s.P > kDcnMaxTapPixels) return fail(PVV_E_ARG, "dcn backward: kh*kw*Ho*Wo > 2^22 (the int64 sums of grad_input could overflow)");
    return PVV_OK;
}

// ---------------------------------------------------------------------------------------------------------------- 3.1 gcol
// gcol[bl, k, p] = the fmaf chain over o ascending from +0 of weight[o, k] * grad_out[b, o, p]  (the SGEMM of C:289-297).
// One workgroup per (128 pixels, 128 values of k, image of the chunk); a wave takes 32 pixels and four 32-row blocks of k.
// Both operands come straight from global memory: lane l holds weight[o + (l >> 5), k0 + 32a + (l & 31)] (A, contiguous over
// the lanes of a half) and grad_out[b, o + (l >> 5), p] (B, contiguous alike).  An odd M ends in one step of zeros.
__global__ __launch_bounds__(kBlock) void k_dcn_gcol(DcnShape s, int b0, const float *__restrict__ weight,
                                                     const float *__restrict__ gout, float *__restrict__ gcol)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int p = blockIdx.x * kDcnPix + wave * 32 + (lane & 31), k0 = blockIdx.y * kDcnGwK, bl = blockIdx.z;
    const float *go = gout + (size_t)(b0 + bl) * s.M * s.P;
    dcn_f16v acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    for (int o = 0; o < s.M; o += 2) {
        const int oo = o + half;
        const bool ov = oo < s.M;
        const float bv = (ov && p < s.P) ? go[(size_t)oo * s.P + p] : 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int k = k0 + 32 * a + (lane & 31);
            const float av = (ov && k < s.K) ? weight[(size_t)oo * s.K + k] : 0.f;
            acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[a], 0, 0, 0);
        }
    }
    if (p < s.P) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (k < s.K) gcol[((size_t)bl * s.K + k) * s.P + p] = acc[a][r];
            }
    }
}

// ------------------------------------------------------------------------------------------- 3.2 grad_offset, grad_mask, max
// One thread per (image of the chunk, group, tap, pixel): I:269-326 restated on the forward's window test and the forward's
// blend.  Over the channels c of the group, ascending:
//   gc = gcol[k = c*KK + t, p];  top = gc * mask;  the image's maximum takes |top| (bit patterns: a NaN ranks above inf)
//   inside the window only:  mval += gc * val,  val the forward's blend without the mask (dcn_col's first line)
//                            ch = 0 + (-wl)*v1 + (-wh)*v2 + wl*v3 + wh*v4     wl = float(w0 + 1) - w, wh = w - float(w0)   (I:101-108)
//                            cw = 0 + (-hl)*v1 + hl*v2 + (-hh)*v3 + hh*v4     hl = float(h0 + 1) - h, hh = h - float(h0)   (I:112-119)
//                            grad_h += (ch * gc) * mask;  grad_w += (cw * gc) * mask                                       (I:318)
// with v1..v4 the forward's neighbours (0 where outside the plane).  Outside the window nothing is added: exactly +0.
// `sample` = 0 takes the maximum alone (grad_input is wanted, grad_offset and grad_mask are not).
__global__ __launch_bounds__(kBlock) void k_dcn_coord(DcnShape s, int b0, int sample, const float *__restrict__ input,
                                                      const float *__restrict__ offset, const float *__restrict__ mask,
                                                      const float *__restrict__ gcol, float *__restrict__ goff, float *__restrict__ gmask,
                                                      unsigned *__restrict__ maxbits)
{
    __shared__ unsigned s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int idx = blockIdx.x * kBlock + threadIdx.x, bl = blockIdx.y, b = b0 + bl;
    unsigned mx = 0;
    if (idx < s.dg * s.KK * s.P) {
        const int p = idx % s.P, gt = idx / s.P, g = gt / s.KK, t = gt - g * s.KK;
        const float *o = offset + (size_t)b * s.off_stride + ((size_t)g * 2 * s.KK + 2 * t) * s.P + p;
        const float m = mask[(size_t)b * s.mask_stride + ((size_t)g * s.KK + t) * s.P + p];
        const int y = p / s.Wo, x = p - y * s.Wo, i = t / s.kw, j = t - i * s.kw;
        const float off_h = o[0], off_w = o[s.P];
        const DcnTap tap = dcn_tap(s, y, x, i, j, off_h, off_w, m);
        const float h = (float)(y * s.sh - s.ph + i * s.dh) + off_h, w = (float)(x * s.sw - s.pw + j * s.dw) + off_w;
        const bool inside = h > -1.f && w > -1.f && h < (float)s.H && w < (float)s.W;
        float hl = 0.f, hh = 0.f, wl = 0.f, wh = 0.f;
        if (inside) {
            const int h0 = (int)floorf(h), w0 = (int)floorf(w);
            hl = (float)(h0 + 1) - h, hh = h - (float)h0, wl = (float)(w0 + 1) - w, wh = w - (float)w0;
        }
        float gh = 0.f, gw = 0.f, gm = 0.f;
        const float *gc_p = gcol + ((size_t)bl * s.K + (size_t)g * s.Cg * s.KK + t) * s.P + p;
        const float *plane = input + ((size_t)b * s.C + (size_t)g * s.Cg) * s.H * s.W;
        for (int c = 0; c < s.Cg; ++c, gc_p += (size_t)s.KK * s.P, plane += (size_t)s.H * s.W) {
            const float gc = *gc_p;
            const float top = gc * m;
            mx = max(mx, (unsigned)__float_as_int(top) & 0x7fffffffu);
            if (sample && inside) {
                const float v1 = (tap.in & 1) ? plane[tap.base] : 0.f;
                const float v2 = (tap.in & 2) ? plane[tap.base + 1] : 0.f;
                const float v3 = (tap.in & 4) ? plane[tap.base + s.W] : 0.f;
                const float v4 = (tap.in & 8) ? plane[tap.base + s.W + 1] : 0.f;
                const float val = ((tap.w1 * v1 + tap.w2 * v2) + tap.w3 * v3) + tap.w4 * v4;
                gm = gm + gc * val;
                float ch = 0.f, cw = 0.f;
                ch = ch + (-wl) * v1, ch = ch + (-wh) * v2, ch = ch + wl * v3, ch = ch + wh * v4;
                cw = cw + (-hl) * v1, cw = cw + hl * v2, cw = cw + (-hh) * v3, cw = cw + hh * v4;
                gh = gh + (ch * gc) * m;
                gw = gw + (cw * gc) * m;
            }
        }
        if (goff) {
            float *q = goff + ((size_t)b * s.dg * 2 * s.KK + (size_t)g * 2 * s.KK + 2 * t) * s.P + p;
            q[0] = gh, q[s.P] = gw;
        }
        if (gmask) gmask[((size_t)b * s.dg * s.KK + (size_t)g * s.KK + t) * s.P + p] = gm;
    }
    atomicMax(&s_max, mx);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(maxbits + bl, s_max);
}

// ------------------------------------------------------------------------------------------------------ 3.3 grad_input
// e_b: 2^e_b is the smallest power of two >= the image's maximum, given as the bits of a finite float > 0.
__device__ __forceinline__ int dcn_pow2_exp(unsigned bits)
{
    const int E = (int)(bits >> 23);
    const unsigned F = bits & 0x7fffffu;
    if (E) return E - 127 + (F ? 1 : 0);
    return (31 - __clz(F)) - 149 + ((F & (F - 1)) ? 1 : 0);
}

__device__ __forceinline__ double dcn_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }   // e in [-1022, 1023]

// One thread per (image of the chunk, k, pixel): what I:209-253 scatters, as integers.  For each of the sample's neighbours
// inside the plane: the contribution float32(w_i * float32(gcol * mask)), w_i the forward's blend weight of that neighbour
// (its derivative; I:56-80 is the same quantity), scaled by 2^(40 - e_b) in binary64 -- exact --, rounded to the nearest
// integer, ties to even, and added into the image's int64 plane.  Integer addition is associative: the order of arrival
// cannot change a bit.  |n| <= 2^40 and at most kh*kw*P <= 2^22 samples reach one element.
__global__ __launch_bounds__(kBlock) void k_dcn_scatter(DcnShape s, int b0, const float *__restrict__ offset,
                                                        const float *__restrict__ mask, const float *__restrict__ gcol,
                                                        const unsigned *__restrict__ maxbits, long long *__restrict__ planes)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x, bl = blockIdx.y, b = b0 + bl;
    if (idx >= s.K * s.P) return;
    const unsigned mb = maxbits[bl];
    if (mb == 0 || mb >= 0x7f800000u) return;                      // all zeros; or not finite: the finishing pass writes NaN
    const int p = idx % s.P, k = idx / s.P, c = k / s.KK, t = k - c * s.KK;
    const DcnTap tap = dcn_tap_at(s, offset, mask, b, c / s.Cg, t, p);
    if (!tap.in) return;
    const float top = gcol[(size_t)bl * s.K * s.P + idx] * tap.mask;
    const double scale = dcn_pow2(kDcnFixBits - dcn_pow2_exp(mb));
    unsigned long long *pl = (unsigned long long *)planes + ((size_t)bl * s.C + c) * s.H * s.W;
    const float wt[4] = {tap.w1, tap.w2, tap.w3, tap.w4};
    const int at[4] = {0, 1, s.W, s.W + 1};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (tap.in & (1 << q)) {
            const long long n = __double2ll_rn((double)(wt[q] * top) * scale);
            if (n) atomicAdd(pl + (tap.base + at[q]), (unsigned long long)n);   // (base alone may be negative; a guarded neighbour's index is not)
        }
}

// The same sums with most of the additions kept on the chip.  One workgroup per (tile of 8 x 32 output pixels, `cc` channels
// of one deformable group, image of the chunk), one thread per pixel.  The tile's samples land near its undeformed footprint,
// so that part of the input plane -- the footprint and kDcnScHalo rows and columns around it, WR x WC elements per channel --
// is an int64 window in LDS: a contribution inside it is an LDS atomic, one outside goes to the plane in memory as in
// k_dcn_scatter, and at the end every window element that is not zero is added to the plane once.  Integers again: where an
// addition happens does not change the sum.  A tap's sampling state is computed once for the `cc` channels.
// Dynamic LDS: u64 [cc][WR * WC].
__global__ __launch_bounds__(kBlock) void k_dcn_scatter_tiled(DcnShape s, int b0, int cc, int WR, int WC, const float *__restrict__ offset,
                                                              const float *__restrict__ mask, const float *__restrict__ gcol,
                                                              const unsigned *__restrict__ maxbits, long long *__restrict__ planes)
{
    extern __shared__ unsigned long long s_win[];
    const int tid = threadIdx.x, bl = blockIdx.z, b = b0 + bl;
    const unsigned mb = maxbits[bl];
    if (mb == 0 || mb >= 0x7f800000u) return;                      // (the whole workgroup: one image)
    const int tiles_x = (s.Wo + kDcnScTx - 1) / kDcnScTx, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int chunks = (s.Cg + cc - 1) / cc, g = blockIdx.y / chunks, cbeg = (blockIdx.y - g * chunks) * cc, cn = min(cc, s.Cg - cbeg);
    const int y = ty * kDcnScTy + tid / kDcnScTx, x = tx * kDcnScTx + tid % kDcnScTx, p = y * s.Wo + x;
    const int r0 = ty * kDcnScTy * s.sh - s.ph - kDcnScHalo, c0 = tx * kDcnScTx * s.sw - s.pw - kDcnScHalo, nwin = WR * WC;
    const int hw = s.H * s.W;
    unsigned long long *pl = (unsigned long long *)planes + ((size_t)bl * s.C + (size_t)g * s.Cg + cbeg) * hw;
    for (int e = tid; e < cn * nwin; e += kBlock) s_win[e] = 0;
    __syncthreads();
    if (y < s.Ho && x < s.Wo) {
        const double scale = dcn_pow2(kDcnFixBits - dcn_pow2_exp(mb));
        for (int t = 0; t < s.KK; ++t) {
            const float *o = offset + (size_t)b * s.off_stride + ((size_t)g * 2 * s.KK + 2 * t) * s.P + p;
            const float m = mask[(size_t)b * s.mask_stride + ((size_t)g * s.KK + t) * s.P + p];
            const int i = t / s.kw;
            const DcnTap tap = dcn_tap(s, y, x, i, t - i * s.kw, o[0], o[s.P], m);
            if (!tap.in) continue;
            const int at[4] = {0, 1, s.W, s.W + 1};
            const float wt[4] = {tap.w1, tap.w2, tap.w3, tap.w4};
            const int q0 = __ffs(tap.in) - 1, idx0 = tap.base + at[q0], row0 = idx0 / s.W;      // a neighbour inside the plane gives the rest their rows and columns
            const int wr0 = row0 - (q0 >> 1) - r0, wc0 = idx0 - row0 * s.W - (q0 & 1) - c0;
            const float *gc = gcol + ((size_t)bl * s.K + ((size_t)g * s.Cg + cbeg) * s.KK + t) * s.P + p;
            for (int c = 0; c < cn; ++c, gc += (size_t)s.KK * s.P) {
                const float top = *gc * tap.mask;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (tap.in & (1 << q)) {
                        const long long n = __double2ll_rn((double)(wt[q] * top) * scale);
                        if (!n) continue;
                        const int wr = wr0 + (q >> 1), wc = wc0 + (q & 1);
                        if ((unsigned)wr < (unsigned)WR && (unsigned)wc < (unsigned)WC) atomicAdd(s_win + c * nwin + wr * WC + wc, (unsigned long long)n);
                        else atomicAdd(pl + (size_t)c * hw + (tap.base + at[q]), (unsigned long long)n);
                    }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < cn * nwin; e += kBlock) {
        const unsigned long long v = s_win[e];
        if (!v) continue;                                          // (every element that is not zero was reached from inside the plane)
        const int c = e / nwin, w = e - c * nwin, wr = w / WC;
        atomicAdd(pl + (size_t)c * hw + (size_t)(r0 + wr) * s.W + (c0 + w - wr * WC), v);
    }
}

// grad_input[b, c, y, x] = float32(double(sum) * 2^(e_b - 40)); NaN everywhere in an image whose maximum is not finite.
__global__ __launch_bounds__(kBlock) void k_dcn_scatter_finish(DcnShape s, int b0, const unsigned *__restrict__ maxbits,
                                                               const long long *__restrict__ planes, float *__restrict__ gin)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x, bl = blockIdx.y;
    const int chw = s.C * s.H * s.W;
    if (idx >= chw) return;
    const unsigned mb = maxbits[bl];
    float v = 0.f;
    if (mb >= 0x7f800000u) v = __int_as_float(0x7fc00000);
    else if (mb) v = (float)((double)planes[(size_t)bl * chw + idx] * dcn_pow2(dcn_pow2_exp(mb) - kDcnFixBits));
    gin[(size_t)(b0 + bl) * chw + idx] = v;
}

// ----------------------------------------------------------------------------------------------------- 3.4 grad_weight
// part[bl, slab, o, k] = the fmaf chain over the slab's pixels ascending from +0 of grad_out[b, o, p] * col[b, k, p]  (the
// SGEMM of C:311-319 on the columns of C:300-307, which are sampled again here and never leave the chip).
// One workgroup per (slab of S pixels, 128 values of k, 32 * NACC output channels, image of the chunk).  32 pixels at a time:
// every thread samples its 16 elements of the column tile into LDS (s_col [pixel][k], through the forward's dcn_tap_at and
// dcn_col) and stages grad_out (s_go [pixel][channel]); a wave then feeds its 32 values of k (B) and the NACC channel blocks
// (A) to v_mfma_f32_32x32x2_f32, two pixels a step.  Pixels past the slab's end, channels >= M and k >= K are zeros.
// Dynamic LDS: s_col [32][129], s_go [32][32 * NACC + 1]; the odd row lengths keep the pixel-major writes off one bank.
template <int NACC>
__global__ __launch_bounds__(kBlock) void k_dcn_gweight(DcnShape s, int b0, int nslab, const float *__restrict__ input,
                                                        const float *__restrict__ offset, const float *__restrict__ mask,
                                                        const float *__restrict__ gout, float *__restrict__ part)
{
    constexpr int MT = 32 * NACC, GS = MT + 1, CS = kDcnGwK + 1;
    extern __shared__ float s_dcn[];
    float *s_col = s_dcn, *s_go = s_col + kDcnGwPix * CS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int slab = blockIdx.x % nslab, k0 = (blockIdx.x / nslab) * kDcnGwK, o0 = blockIdx.y * MT, bl = blockIdx.z, b = b0 + bl;
    const int pbeg = slab * kDcnSlab, pend = min(s.P, pbeg + kDcnSlab);
    const int pl = tid & (kDcnGwPix - 1), krow = tid / kDcnGwPix;

    dcn_f16v acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    for (int pp = pbeg; pp < pend; pp += kDcnGwPix) {
        __syncthreads();                                           // the last step's MFMAs have read the tiles
        for (int e = tid; e < kDcnGwPix * MT; e += kBlock) {
            const int q = e & (kDcnGwPix - 1), ol = e / kDcnGwPix;
            s_go[q * GS + ol] = (o0 + ol < s.M && pp + q < pend) ? gout[((size_t)b * s.M + o0 + ol) * s.P + pp + q] : 0.f;
        }
        const int p = pp + pl;
        for (int kl = krow; kl < kDcnGwK; kl += kBlock / kDcnGwPix) {
            const int k = k0 + kl;
            float v = 0.f;
            if (k < s.K && p < pend) {
                const int c = k / s.KK, t = k - c * s.KK;
                const DcnTap tap = dcn_tap_at(s, offset, mask, b, c / s.Cg, t, p);
                v = dcn_col(input + ((size_t)b * s.C + c) * s.H * s.W, s.W, tap);
            }
            s_col[pl * CS + kl] = v;
        }
        __syncthreads();
        const float *cb = s_col + half * CS + wave * 32 + (lane & 31);
        const float *gb = s_go + half * GS + (lane & 31);
#pragma unroll 4
        for (int kk = 0; kk < kDcnGwPix; kk += 2) {
            const float bv = cb[kk * CS];
#pragma unroll
            for (int a = 0; a < NACC; ++a) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(gb[kk * GS + 32 * a], bv, acc[a], 0, 0, 0);
        }
    }

    const int k = k0 + wave * 32 + (lane & 31);
    if (k < s.K) {
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (o < s.M) part[(((size_t)bl * nslab + slab) * s.M + o) * s.K + k] = acc[a][r];
            }
    }
}

// grad_weight[o, k] = float32 of the binary64 sum of part over (image, slab) ascending: the accumulator lives in the workspace
// between the chunks, so the order -- and the result -- does not depend on the chunk size.
__global__ __launch_bounds__(kBlock) void k_dcn_gweight_reduce(int mk, int nb, int nslab, int first, int last,
                                                               const float *__restrict__ part, double *__restrict__ wacc,
                                                               float *__restrict__ gw)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mk) return;
    double a = first ? 0.0 : wacc[i];
    for (int e = 0; e < nb * nslab; ++e) a = a + (double)part[(size_t)e * mk + i];
    wacc[i] = a;
    if (last) gw[i] = (float)a;
}

// ------------------------------------------------------------------------------------------------------- 3.5 grad_bias
// One workgroup per output channel (C:322-329 in binary64).  Per image: thread l adds grad_out[b, o, p] for p = l, l + 256, ...
// ascending from +0; the 256 sums fold as s[i] += s[i + w] for w = 128, 64, ..., 1; the images' sums are added ascending to
// the accumulator kept in the workspace, which is rounded to float32 once after the last image.
__global__ __launch_bounds__(kBlock) void k_dcn_gbias(DcnShape s, int b0, int nb, int first, int last, const float *__restrict__ gout,
                                                      double *__restrict__ bacc, float *__restrict__ gb)
{
    __shared__ double s_sum[kBlock];
    const int o = blockIdx.x, tid = threadIdx.x;
    double tot = first ? 0.0 : bacc[o];
    for (int bl = 0; bl < nb; ++bl) {
        const float *g = gout + ((size_t)(b0 + bl) * s.M + o) * s.P;
        double a = 0.0;
        for (int p = tid; p < s.P; p += kBlock) a = a + (double)g[p];
        s_sum[tid] = a;
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if (tid < w) s_sum[tid] = s_sum[tid] + s_sum[tid + w];
            __syncthreads();
        }
        tot = tot + s_sum[0];
        __syncthreads();
    }
    if (tid == 0) {
        bacc[o] = tot;
        if (last) gb[o] = (float)tot;
    }
}

template <int NACC>
int dcn_gweight_launch(const DcnShape &s, int b0, int nb, int nslab, const float *input, const float *offset, const float *mask,
                       const float *gout, float *part, hipStream_t st)
{
    const size_t lds = sizeof(float) * ((size_t)kDcnGwPix * (kDcnGwK + 1) + (size_t)kDcnGwPix * (32 * NACC + 1));
    const long long gx = (long long)nslab * ((s.K + kDcnGwK - 1) / kDcnGwK);
    const dim3 grid((unsigned)gx, (s.M + 32 * NACC - 1) / (32 * NACC), nb);
    if (gx >= (1ll << 31) || grid.y > 65535) return fail(PVV_E_ARG, "dcn backward: M or K is too large for one launch");
    hipLaunchKernelGGL(k_dcn_gweight<NACC>, grid, dim3(kBlock), lds, st, s, b0, nslab, input, offset, mask, gout, part);
    return check_launch("k_dcn_gweight");
}

int dcn_bwd_args(DcnShape &s, int B, int C, int H, int W, int M, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg,
                 long long off_stride, long long mask_stride)
{
    if (int e = dcn_shape(s, B, C, H, W, M, kh, kw, sh, sw, ph, pw, dh, dw, dg, off_stride, mask_stride)) return e;
    return dcn_bwd_shape(s);
}

}  // namespace

// Replaces the allocations of C:206-335 (`ones`, `columns`): what pvv_dcn_backward needs, host only.
PVV_EXPORT long long pvv_dcn_backward_workspace_bytes(int B, int C, int H, int W, int M, int kh, int kw, int stride_h, int stride_w,
                                                      int pad_h, int pad_w, int dil_h, int dil_w, int deformable_groups, int chunk_images)
{
    DcnShape s;
    if (int e = dcn_bwd_args(s, B, C, H, W, M, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, deformable_groups, 1ll << 62, 1ll << 62))
        return e;
    DcnBwdLayout L;
    dcn_bwd_layout(s, 1, L);
    long long chunk = chunk_images;
    if (chunk <= 0) chunk = kDcnBwdDefaultBytes / (long long)L.per_image;
    chunk = chunk < 1 ? 1 : (chunk > B ? B : chunk);
    dcn_bwd_layout(s, (int)chunk, L);
    return (long long)L.total;
}

// Replaces dcn_v2_cuda_backward (C:206-335) with its three kernels' work: modulated_deformable_col2im_coord_cuda (I:256-327
// with the coordinate weight of I:82-123), modulated_deformable_col2im_cuda (I:197-254 with the gradient weight of I:56-80),
// the two SGEMMs and the bias SGEMV.
PVV_EXPORT int pvv_dcn_backward(const float *d_input, const float *d_weight, const float *d_offset, long long offset_image_stride,
                                const float *d_mask, long long mask_image_stride, const float *d_grad_out, int B, int C, int H, int W,
                                int M, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                                int deformable_groups, float *d_grad_input, float *d_grad_offset, float *d_grad_mask,
                                float *d_grad_weight, float *d_grad_bias, void *d_workspace, size_t workspace_bytes, void *stream)
{
    DcnShape s;
    if (int e = dcn_bwd_args(s, B, C, H, W, M, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, deformable_groups,
                             offset_image_stride, mask_image_stride))
        return e;
    if (!d_input || !d_weight || !d_offset || !d_mask || !d_grad_out) return fail(PVV_E_ARG, "dcn backward: NULL device pointer");
    if (!d_workspace || ((uintptr_t)d_workspace & 255)) return fail(PVV_E_ARG, "dcn backward: the workspace must be 256-byte aligned");
    DcnBwdLayout L;
    dcn_bwd_layout(s, 1, L);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "dcn backward: the workspace is smaller than one image needs");
    long long chunk = (long long)((workspace_bytes - L.fixed) / L.per_image);
    chunk = chunk > s.B ? s.B : chunk;
    dcn_bwd_layout(s, (int)chunk, L);

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)d_workspace;
    double *wacc = (double *)(ws + L.wacc), *bacc = (double *)(ws + L.bacc);
    unsigned *maxbits = (unsigned *)(ws + L.maxbits);
    float *gcol = (float *)(ws + L.gcol), *part = (float *)(ws + L.part);
    long long *planes = (long long *)(ws + L.plane);
    const bool coord = d_grad_offset || d_grad_mask, need_gcol = coord || d_grad_input;
    const int chw = s.C * s.H * s.W;

    for (int b0 = 0; b0 < s.B; b0 += L.chunk) {
        const int nb = min(L.chunk, s.B - b0), first = b0 == 0, last = b0 + nb == s.B;
        if (need_gcol) {
            if (hipMemsetAsync(maxbits, 0, sizeof(unsigned) * nb, st) != hipSuccess) return check_launch("hipMemsetAsync");
            hipLaunchKernelGGL(k_dcn_gcol, dim3((s.P + kDcnPix - 1) / kDcnPix, (s.K + kDcnGwK - 1) / kDcnGwK, nb), dim3(kBlock), 0, st, s, b0,
                               d_weight, d_grad_out, gcol);
            if (int e = check_launch("k_dcn_gcol")) return e;
            hipLaunchKernelGGL(k_dcn_coord, dim3((s.dg * s.KK * s.P + kBlock - 1) / kBlock, nb), dim3(kBlock), 0, st, s, b0, coord ? 1 : 0,
                               d_input, d_offset, d_mask, gcol, d_grad_offset, d_grad_mask, maxbits);
            if (int e = check_launch("k_dcn_coord")) return e;
        }
        if (d_grad_input) {
            if (hipMemsetAsync(planes, 0, sizeof(long long) * (size_t)nb * chw, st) != hipSuccess) return check_launch("hipMemsetAsync");
            // the windows of the tiled form: the tile's footprint, the row and column below and right of a sample, the halo
            const long long WR = (long long)(kDcnScTy - 1) * s.sh + (long long)(s.kh - 1) * s.dh + 2 + 2 * kDcnScHalo,
                            WC = (long long)(kDcnScTx - 1) * s.sw + (long long)(s.kw - 1) * s.dw + 2 + 2 * kDcnScHalo;
            const long long cc = min((long long)s.Cg, (long long)(kDcnScLdsBytes / sizeof(long long)) / (WR * WC));
            const long long tiles = (long long)((s.Ho + kDcnScTy - 1) / kDcnScTy) * ((s.Wo + kDcnScTx - 1) / kDcnScTx);
            if (cc >= 1 && (long long)s.dg * ((s.Cg + cc - 1) / cc) <= 65535) {
                hipLaunchKernelGGL(k_dcn_scatter_tiled, dim3((unsigned)tiles, (unsigned)(s.dg * ((s.Cg + cc - 1) / cc)), nb), dim3(kBlock),
                                   sizeof(long long) * (size_t)(cc * WR * WC), st, s, b0, (int)cc, (int)WR, (int)WC, d_offset, d_mask, gcol,
                                   maxbits, planes);
                if (int e = check_launch("k_dcn_scatter_tiled")) return e;
            } else {                                               // a footprint too large for LDS (a huge stride or dilation)
                hipLaunchKernelGGL(k_dcn_scatter, dim3((s.K * s.P + kBlock - 1) / kBlock, nb), dim3(kBlock), 0, st, s, b0, d_offset, d_mask,
                                   gcol, maxbits, planes);
                if (int e = check_launch("k_dcn_scatter")) return e;
            }
            hipLaunchKernelGGL(k_dcn_scatter_finish, dim3((chw + kBlock - 1) / kBlock, nb), dim3(kBlock), 0, st, s, b0, maxbits, planes,
                               d_grad_input);
            if (int e = check_launch("k_dcn_scatter_finish")) return e;
        }
        if (d_grad_weight) {
            int e;
            if (s.M > 64) e = dcn_gweight_launch<4>(s, b0, nb, L.nslab, d_input, d_offset, d_mask, d_grad_out, part, st);
            else if (s.M > 32) e = dcn_gweight_launch<2>(s, b0, nb, L.nslab, d_input, d_offset, d_mask, d_grad_out, part, st);
            else e = dcn_gweight_launch<1>(s, b0, nb, L.nslab, d_input, d_offset, d_mask, d_grad_out, part, st);
            if (e) return e;
            const int mk = s.M * s.K;
            hipLaunchKernelGGL(k_dcn_gweight_reduce, dim3((mk + kBlock - 1) / kBlock), dim3(kBlock), 0, st, mk, nb, L.nslab, first, last, part,
                               wacc, d_grad_weight);
            if (int e2 = check_launch("k_dcn_gweight_reduce")) return e2;
        }
        if (d_grad_bias) {
            hipLaunchKernelGGL(k_dcn_gbias, dim3(s.M), dim3(kBlock), 0, st, s, b0, nb, first, last, d_grad_out, bacc, d_grad_bias);
            if (int e = check_launch("k_dcn_gbias")) return e;
        }
    }
    return PVV_OK;
}
