// count_tile.hpp -- stage 3: the split-bf16 matrix-core count tile, stated once for the two kernels that run it
// (k_count_bf16 in count_bf16.hpp, k_count_filter_runs in count_filter_runs.hpp).
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace, in front of count_bf16.hpp);
// see that file for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py).
#pragma once

// ---------------------------------------------------------------------------------------------
// Stage 3, matrix-core prefilter form (k_count_bf16).
//
// The sqrt/divide-free VALU kernel of round 1 (k_count_fast, removed) was bound by VALU issue (7.35 VALU instructions per evaluation, 84 % VALU busy); 4 of the 6.5
// useful ones are the two dot products a = d.nh and b' = kappa d x nh.  Those are bilinear in (hx,hy,1) and the
// pixel's (nh, -c.nh) / (B, -c.B): a rank-3 form.  The f32 MFMA shares the fp32 VALU datapath on gfx950
// (round 1's mfma_valu_overlap microbenchmark, profiles/r01_microbench.txt: no overlap), but the bf16 matrix core is a separate
// pipe that does overlap (tools/microbench/bf16_mfma_overlap.hip; how much: tools/microbench/count_pipe3.hip, round 6).  So every fp32 operand is split EXACTLY into three bf16
// pieces x = x0 + x1 + x2 (+ <= 2^-27 |x|), the six leading piece products of hx*nhx and of hy*nhy plus the three
// pieces of the constant are the 15 terms of a K=16 dot product, and ONE v_mfma_f32_32x32x16_bf16 delivers a
// (rows 0-15) and b' (rows 16-31) for 16 pixels x 32 hypotheses.  The VALU keeps t = a - |b'|, the sign-bit
// queue and the guard-band test: 21 instructions per 512 evaluations instead of 56 x 4.
//
// The MFMA result is only a PREFILTER: the decision is taken from it when |t| - beta*a > eps, otherwise that
// evaluation is redone with the exact binary32 sequence (K:100-125).  The hot loop tests a whole 16x32 tile against
// a per-hypothesis upper bound of beta*a + eps (one v_min3 chain); tiles that fail mark their in-band evaluations
// while a and t are in registers, and only those are re-decided after the 8 tiles of the hypothesis tile.
// Bound, with u = 2^-24, d = fl(h-c) as the exact path sees it, o = the block's integer origin, c' = c-o (exact),
// h' = fl(h-o), C1 = max |c'|_1 of the block:
//     piece residuals and dropped piece products          <= 0.5 u S,   S = |hx' nhx| + |hy' nhy| + |c'.nh|
//     bf16 MFMA accumulation (products exact in f32; 15 f32 roundings in any order)  <= 15 u S
//     (measured on MI355X: 3.9 u S including the split, bf16_mfma_overlap.hip)
//     fl(h-o), the exact path's fl(h-c), f32 unit normal (4u: v_rsq_f32, see pixel_records), f32 c'.nh   
//  => |a_mfma - a_true| <= u (31 |d| + 35 C1);  for b' the operand B = kappa perp(nh) carries 6u instead of 4u:
//     kappa u (33 |d| + 35 C1);
//     beta = 1.25 (33 (1+kappa) + 8/(1-T^2)) u / T,     eps = 1.25 (1+kappa) 35 u C1 + eps_abs.
// Inlier counts stay bit-exact (tests/test_gpu_parity.py, every parity test runs through this kernel by default).
//
// Layout (MI355X_MICROARCH / verified in the microbenchmark): A operand lane l = row l%32, k = 8*(l/32)..+7;
// B operand lane l = column l%32, same k; D register r of lane l = row 4*(l/32) + r%4 + 8*(r/4), column l%32.
// Rows = (form, pixel) of a 16-pixel tile, columns = 32 hypotheses: every lane owns ONE hypothesis and 8 of the
// 16 pixels; lanes l and l^32 share a hypothesis and are merged in LDS.
//
// A kernel that counts with it holds, in LDS, sB (B operands of up to kBfMaxHt hypothesis tiles), sP (a 512-pixel chunk's
// records), sCnt (a counter per staging slot), sRed and s_keep, and walks, per chunk: pixel_records + stage_b_operand, a
// barrier, build_a_operands, then count_tiles -- or count_group_exact when stage_b_operand flagged a hypothesis.
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

#define kDdAlive __uint_as_float(0x2b8cbcceu)   // 1.0000002e-12f: the smallest dd with (double)sqrtf(dd) >= 1e-6
constexpr int kBfPixPerWave = 128;   // 8 tiles of 16 pixels, A operands live in 32 VGPRs
constexpr int kBfMaxHt = 16;         // 32-hypothesis tiles per work item (512 hypotheses)

struct Bf16Consts {
    float beta;    // relative half-width of the guard band (units of a)
    float eps_c;   // absolute half-width per pixel of block extent C1
    float eps0;    // absolute floor (covers the exact path's norm2 < 1e-6 reject)
    float kappa;
    float beta2;   // band of the second-level (f32, un-translated) test used on flagged evaluations
};

// x = p[0] + p[1] + p[2] + r, |r| <= 2^-27 |x|; every piece is a bf16 value (round to nearest even)
__device__ __forceinline__ void split3(float x, __bf16 (&p)[3])
{
    p[0] = (__bf16)x;
    float r = x - (float)p[0];
    p[1] = (__bf16)r;
    r = r - (float)p[1];
    p[2] = (__bf16)r;
}

// B operand of the hypothesis in staging slot i: lane l of tile ht holds column l%32, k = 8*(l/32)..+7 of
//   (qx0,qy0,qx1,qx2,qx0,qy1,qy2,qy0 || qx0,qy0,qx1,qy1, 1,1,1,0),   q = pieces of h' = fl(h - o).
// The slot's counter is the caller's.  Returns 1 for a hypothesis that is non-finite or astronomically far (the whole
// group then takes the exact loop, count_group_exact).
__device__ __forceinline__ int stage_b_operand(bf16x8 *sB, int i, float2 hp, float2 org)
{
    __bf16 qx[3], qy[3];
    split3(hp.x - org.x, qx);
    split3(hp.y - org.y, qy);
    const __bf16 one = (__bf16)1.f, zero = (__bf16)0.f;
    const bf16x8 lo8 = {qx[0], qy[0], qx[1], qx[2], qx[0], qy[1], qy[2], qy[0]};
    const bf16x8 hi8 = {qx[0], qy[0], qx[1], qy[1], one, one, one, zero};
    sB[(i >> 5) * 64 + (i & 31)] = lo8;
    sB[(i >> 5) * 64 + 32 + (i & 31)] = hi8;
    return !(fabsf(hp.x) < 1e15f && fabsf(hp.y) < 1e15f);
}

// The count a hypothesis must still be able to reach to matter.  ransac_voting_layer_v3 keeps the arg-max: L* itself.  The
// estimate zeroes every ratio below  max ratio - 0.1  in binary32 (k_covariance: thr = fl(fl(mx)/fl(tn)) - 0.1f, r = fl(c / tn),
// r < thr -> 0): a hypothesis whose full count is below  L* - 0.1 tn - margin  has weight zero with its full count and with any
// partial count (r is monotone in c), so it may be dropped.  margin: 0.1f = 0.1000000015 and three binary32 roundings of
// ratios <= 1 are < 4e-7 in ratio units = tn * 4e-7 counts; ceil(tn / 10) + 2 + tn / 2^20 covers both for every tn.
__device__ __forceinline__ int stage_bound(int lstar, int tn, int sub_tenth)
{
    if (sub_tenth && lstar >= 0) lstar -= (tn + 9) / 10 + 2 + (tn >> 20);
    return lstar;
}

// L* of an (image, keypoint) from k_lead's eight words (count_prune.hpp), lane l holding leader l%4's partial count (-1: none)
// and its sure inliers among the pixels the first launch did not count: the larger of the leaders' lower bounds, lowered for
// the estimate (stage_bound).  The two loads stay with the caller's other loads.
__device__ __forceinline__ int leaders_bound(int lead_p, int lead_r, int tn, int sub_tenth)
{
    int full = lead_p >= 0 ? lead_p + lead_r : -1;
    full = max(full, PVV_DPP(full, full, 0xB1, 0xf, false));   // quad_perm [1,0,3,2]
    full = max(full, PVV_DPP(full, full, 0x4E, 0xf, false));   // quad_perm [2,3,0,1]: lanes 0-3 hold the four leaders' maximum
    return stage_bound(__builtin_amdgcn_readfirstlane(full), tn, sub_tenth);
}

// The kept-slot compaction: every thread decides for its two candidates (i = thread + q * kBlock) whether they are kept;
// slot[q] becomes the rank of candidate q among the kept ones in the order (q, wave, lane), and the return value their number
// (block-uniform).  Contains ONE barrier, between the waves' popcounts in s_keep[8] and the prefix over them; the caller's next
// barrier is what frees s_keep for the next compaction.
__device__ __forceinline__ int compact_kept(int *s_keep, const bool (&keep)[2], int lane, int wave, int (&slot)[2])
{
    unsigned long long m[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        m[q] = __ballot(keep[q]);
        if (lane == 0) s_keep[q * 4 + wave] = __popcll(m[q]);
    }
    __syncthreads();
    int tot = 0;
    slot[0] = slot[1] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int v = s_keep[j];
        tot += v;
        if (j < wave) slot[0] += v;
        if (j < 4 + wave) slot[1] += v;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
        slot[q] += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m[q] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m[q], 0u));
    return tot;
}

// ---- per pixel (two per thread, prefetched by the caller: pc = coordinates, pd = directions of pixels pb + tid + q * kBlock):
//      the f32 unit normal and the translated coordinates (16 bytes of LDS; the
//      kappa-scaled perpendicular and the constants -(c-o).nh, -(c-o).B are formed where they are used).  A pixel
//      the exact test can never accept (K:121 norm1 < 1e-6, a non-finite norm1) or beyond tn is marked by
//      nhx = NaN and becomes nh = B = 0, constant -1e30 in the A operand: a = -1e30, b' = 0, t < 0.
//      Leaves each wave's max |c'|_1 in sRed[wave]; C1 is their maximum, after the caller's barrier.
__device__ __forceinline__ void pixel_records(float4 *sP, float *sRed, const float2 (&pc)[2], const float2 (&pd)[2], float2 org,
                                              int tid, int pb, int tn, int lane, int wave)
{
    float c1 = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int pl = tid + q * kBlock, p = pb + pl;
        float4 rec = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
        if (p < tn) {
            const float2 c = pc[q], d = pd[q];
            const float cx = c.x - org.x, cy = c.y - org.y;  // exact (integers)
            c1 = fmaxf(c1, fabsf(cx) + fabsf(cy));
            // unit normal by v_rsq_f32 (one transcendental and two multiplies instead of a correctly rounded square root
            // and two divisions: ~60 VALU instructions less per wave and item, -1.6 % per call).  Its components are
            // within 4u of the true ones (dd 2u -> 1u, v_rsq_f32 <= 0.8633 ulp = 1.73u measured over ALL normal inputs,
            // the product 1u; 2.72u measured over 4e9 directions: tools/microbench/rsq_accuracy.hip), which is what
            // the guard bands assume (bf16_consts).  The exact test's reject  (double)sqrtf(dd) < 1e-6  (K:121) is a
            // threshold on dd itself, sqrtf being monotone: kDdAlive is the smallest binary32 it accepts
            // (tests/test_band_model.py recomputes it).
            const float dd = d.x * d.x + d.y * d.y;
            if (dd >= kDdAlive && dd < INFINITY) {
                const float rinv = __builtin_amdgcn_rsqf(dd);
                rec = make_float4(d.x * rinv, d.y * rinv, cx, cy);
            }
        }
        sP[pl] = rec;
    }
    c1 = wave_max(c1);
    if (lane == 0) sRed[wave] = c1;
}

// ---- A operands: lane l = row l%32 (form = row/16, pixel = row%16), k = 8*(l/32)..+7 of
//      (vx0,vy0,vx0,vx0,vx1,vy0,vy0,vy1 || vx2,vy2,vx1,vy1, cv0,cv1,cv2, 0); built once per chunk.  The order of
//      the 15 terms is free; this one puts (qx0,qy0) first in BOTH k halves of the B operand (band width below).
//      Lanes l and l+32 need the two k halves of the SAME row, so they share the work: the lower lane splits the
//      row for tiles 0-3, the upper one for tiles 4-7, each forms both halves, and one v_permlane32_swap per
//      register hands the partner its half.  ntile_w = this wave's share of the chunk's 16-pixel tiles (0..8; tile
//      4*j + wave is its j-th, A[j]).
__device__ __forceinline__ void build_a_operands(const float4 *sP, const Bf16Consts &fc, int wave, int lane, int ntile_w, bf16x8 (&A)[8])
{
    if (ntile_w > 0) {
        const int kslice = lane >> 5, form = (lane >> 4) & 1, prow = lane & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = kslice * 4 + i;
            const float4 rec = sP[(j * 4 + wave) * 16 + prow];
            // row of the a-form: (nh, -c'.nh); of the b'-form: (B, -c'.B) with B = kappa perp(nh)
            const bool dead = rec.x != rec.x;
            float rx = form ? -fc.kappa * rec.y : rec.x;
            float ry = form ? fc.kappa * rec.x : rec.y;
            float rz = -(rec.z * rx + rec.w * ry);
            if (dead) { rx = 0.f; ry = 0.f; rz = form ? 0.f : -1e30f; }
            __bf16 vx[3], vy[3], cv[3];
            split3(rx, vx);
            split3(ry, vy);
            split3(rz, cv);
            const __bf16 zero = (__bf16)0.f;
            const bf16x8 lo8 = {vx[0], vy[0], vx[0], vx[0], vx[1], vy[0], vy[0], vy[1]};
            const bf16x8 hi8 = {vx[2], vy[2], vx[1], vy[1], cv[0], cv[1], cv[2], zero};
            uint4 x = __builtin_bit_cast(uint4, lo8), y = __builtin_bit_cast(uint4, hi8);
            // swap(x, y): lanes 32-63 of x <-> lanes 0-31 of y.  Afterwards x = this lane's k half of tile i (own lo8
            // below 32, the partner's hi8 above), y = this lane's k half of tile 4 + i
            {
                const auto r0 = __builtin_amdgcn_permlane32_swap(x.x, y.x, false, false);
                const auto r1 = __builtin_amdgcn_permlane32_swap(x.y, y.y, false, false);
                const auto r2 = __builtin_amdgcn_permlane32_swap(x.z, y.z, false, false);
                const auto r3 = __builtin_amdgcn_permlane32_swap(x.w, y.w, false, false);
                x = make_uint4(r0[0], r1[0], r2[0], r3[0]);
                y = make_uint4(r0[1], r1[1], r2[1], r3[1]);
            }
            A[i] = __builtin_bit_cast(bf16x8, x);
            A[4 + i] = __builtin_bit_cast(bf16x8, y);
        }
    }
}

// The exact loop (K:100-125) over the nht staged tiles of a group in which some hypothesis is non-finite / astronomically
// far: lane l counts slot ht*32 + l%32 over every eighth pixel of the chunk [pb, pb + 512) below tn.  hyp_of(slot) = the
// slot's un-translated hypothesis.
template <class HypOf>
__device__ __forceinline__ void count_group_exact(int *sCnt, int nht, int nslot, int wave, int lane, int pb, int tn,
                                                  const float2 *crd, const float2 *dir_k, float thresh, HypOf hyp_of)
{
    const int col = lane & 31, kslice = lane >> 5;
    for (int ht = 0; ht < nht; ++ht) {
        const int slot = ht * 32 + col;
        if (slot >= nslot) continue;
        const float2 hp = hyp_of(slot);
        int inl = 0;
        for (int p = pb + wave * 2 + kslice; p < min(tn, pb + 4 * kBfPixPerWave); p += 8) {
            const float2 c = crd[p], d = dir_k[p];
            inl += vote_exact(c.x, c.y, hp.x, hp.y, d.x, d.y, thresh) ? 1 : 0;
        }
        if (inl) atomicAdd(&sCnt[slot], inl);
    }
}

// The matrix-core loop: this wave's ntile_w (> 0) pixel tiles (A) against the nht staged hypothesis tiles (sB), the inliers
// added to sCnt[slot].  eps = eps0 + eps_c C1, epsw = beta 1.02 C1 + eps (the band half-width at |h'| = 0) of the chunk;
// hyp_of(slot) = the slot's un-translated hypothesis, fetched only for the rare second-level test.
template <class HypOf>
__device__ __forceinline__ void count_tiles(const bf16x8 *sB, const float4 *sP, int *sCnt, const bf16x8 (&A)[8], const Bf16Consts &fc,
                                            float eps, float epsw, int nht, int nslot, int ntile_w, int wave, int lane, int pb, int tn,
                                            float2 org, const float2 *crd, const float2 *dir_k, float thresh, HypOf hyp_of)
{
    const int col = lane & 31;
    const int ebase = (lane >> 5) * 4;                       // this lane's pixels of a tile: ebase + e%4 + 8*(e/4)
    const float16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ht = 0; ht < nht; ++ht) {
        const bf16x8 Bop = sB[ht * 64 + lane];
        unsigned flagged = 0u;                            // wave-uniform: tiles with an evaluation in the band
        // conservative band half-width of this lane's hypothesis for the whole chunk: a = d.nh <= |d|_2 <=
        // |h'|_1 + |c'|_1 <= (|qx0| + |qy0|) (1 + 2^-8) + C1 -- the leading bf16 pieces are the first two elements
        // of either half of the B operand; the 2 % slack covers that and the roundings of a
        const unsigned q01 = __builtin_bit_cast(uint4, Bop).x;
        const float wband = __builtin_fmaf(fc.beta * 1.02f,
                                           fabsf(__uint_as_float(q01 << 16)) + fabsf(__uint_as_float(q01 & 0xffff0000u)),
                                           epsw);
        unsigned qs[2] = {0u, 0u};                        // sign-bit queues, one per 4 tiles (newest evaluation = bit 0)
        unsigned mb[2] = {0u, 0u};                        // in-band evaluations of flagged tiles: bit 8*(j%4) + e
        // ntile_w made opaque per hypothesis tile: the seven "j < ntile_w" below are then scalar compares in
        // place instead of seven SGPR pairs computed per item and kept alive across the loop (26 instead of 41
        // spilled scalars in the full kernel, 53 instead of 64 in the filter kernel; -0.1 ... -1.4 % per call)
        int ntw = ntile_w;
        asm volatile("" : "+s"(ntw));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < ntw) {
                const float16v acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[j], Bop, zero16, 0, 0, 0);
                // conservative band test per tile: min |t|  vs  beta * (bound on a) + eps
                float tmin = INFINITY;
                float t[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    t[e] = acc[e] - fabsf(acc[8 + e]);
                    qs[j >> 2] = __builtin_amdgcn_alignbit(qs[j >> 2], __float_as_uint(t[e]), 31);
                    tmin = fminf(tmin, fabsf(t[e]));
                }
                if (__builtin_expect(__ballot(tmin <= wband) != 0, 0)) {
                    // rare (a few % of the tiles): mark the evaluations that really are inside the band,
                    // |t| - beta a <= eps, while a and t are still in registers; they are re-decided below
                    // (sign bit of eps - z is set exactly when z > eps: the same bit queue as for t, 3 VALU per
                    // evaluation; evaluation e of the tile ends up in bit 7 - e, set = NOT in the band)
                    unsigned out_of_band = 0u;
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        out_of_band = __builtin_amdgcn_alignbit(
                            out_of_band, __float_as_uint(eps - __builtin_fmaf(-fc.beta, acc[e], fabsf(t[e]))), 31);
                    mb[j >> 2] |= (~out_of_band & 0xffu) << (8 * (j & 3));
                    flagged |= 1u << j;
                }
            }
        }
        int inl = 8 * ntile_w - __popc(qs[0]) - __popc(qs[1]);   // sign bit set = not an inlier
        // flagged tiles (a third of the iterations has one) mostly hold no evaluation that really is in the band;
        // only then the un-translated hypothesis is fetched (not ahead of the tiles either: that prefetch costs
        // more issue slots in every iteration than the stall does in a sixth of them, measured +1.6 %)
        if (__builtin_expect(flagged != 0u, 0) && __any((mb[0] | mb[1]) != 0u)) {
            const int slot = ht * 32 + col;
            const float2 hp = slot < nslot ? hyp_of(slot) : make_float2(0.f, 0.f);
            do {
                // re-decide the marked evaluations of tile j exactly (K:100-125)
                const int j = __builtin_ctz(flagged);
                flagged &= flagged - 1;
                const unsigned m = mb[j >> 2] >> (8 * (j & 3));
                if (!__any((m & 0xffu) != 0u)) continue;
                // position of evaluation (j, e) in its sign queue: tiles pushed after it, 8 bits each, then 7 - e
                const int after = min(ntile_w - (j & 4), 4) - 1 - (j & 3);
                const unsigned sgn = qs[j >> 2] >> (8 * after);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const bool marked = (m >> (7 - e)) & 1u;
                    if (!__any(marked)) continue;
                    const int prow = (j * 4 + wave) * 16 + ebase + (e & 3) + 8 * (e >> 2);
                    const int p = pb + prow;
                    const int fast = ((sgn >> (7 - e)) & 1u) ? 0 : 1;
                    // second level: the sqrt/divide-free test of round 1 (k_count_fast) on d = fl(h - c) (the exact path's own
                    // d) with the f32 unit normal from LDS; its band (beta2, eps0) is ~10x narrower than the MFMA's
                    const float4 rec = sP[prow];
                    const float dx = hp.x - (rec.z + org.x), dy = hp.y - (rec.w + org.y);
                    const float a2 = __builtin_fmaf(dx, rec.x, dy * rec.y);
                    const float b2 = __builtin_fmaf(dx, -fc.kappa * rec.y, dy * (fc.kappa * rec.x));
                    const float t2 = a2 - fabsf(b2);
                    int decided = t2 > 0.f ? 1 : 0;
                    const bool unsure = marked && (!(__builtin_fmaf(-fc.beta2, a2, fabsf(t2)) > fc.eps0) || rec.x != rec.x);
                    if (__any(unsure)) {
                        int exact = 0;
                        if (unsure && p < tn) {
                            const float2 c = crd[p], d = dir_k[p];
                            exact = vote_exact(c.x, c.y, hp.x, hp.y, d.x, d.y, thresh) ? 1 : 0;
                        }
                        if (unsure) decided = exact;
                    }
                    if (p >= tn) decided = 0;
                    if (marked) inl += decided - fast;
                }
            } while (flagged != 0u);
        }
        if (inl) atomicAdd(&sCnt[ht * 32 + col], inl);    // LDS: 2 lanes x 4 waves per hypothesis
    }
}
