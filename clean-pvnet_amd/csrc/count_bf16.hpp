// count_bf16.hpp -- stage 3: split-bf16 matrix-core prefilter inlier-count kernel (default).
// Part of the single translation unit pvnet_vote.hip (included inside its anonymous namespace, after count_tile.hpp); see that file
// for the numerical contract and the reference citations (K = ransac_voting_kernel.cu, P = ransac_voting_gpu.py), and
// count_tile.hpp for the matrix-core tile itself: operand layout, error bound, pixel records, the loop, the compaction.
#pragma once

// phase timestamps of a few blocks, instrumented builds only (tools/build_variant.sh -DPVV_TUNING -DPVV_STAMPS +
// tools/phase_stamps.py); they cost registers, so timing sweeps use -DPVV_TUNING alone
#ifdef PVV_STAMPS
#define PVV_STAMP(i) do { if (dbg && threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == 97 || blockIdx.x == 401)) \
    dbg[((blockIdx.x == 0 ? 0 : (blockIdx.x == 97 ? 1 : 2)) * 16) + (i)] = wall_clock64(); } while (0)
// per-block census behind the three timelines, 16 words per block at dbg[64 + 16 * block]:
//   [0] entry, [1] exit (wall_clock64: the 100 MHz real-time counter), [2] hardware id (HW_ID | XCC_ID << 32), [3] items processed,
//   [4..11] SHADER cycles (s_memtime) thread 0 spent per phase -- kCensusPhases below --, [12] real-time ticks of the matrix-core
//   loop phase, [13] matrix-core tiles wave 0 multiplied.  Shader cycles / real time = the clock the chip ran at INSIDE the phase
//   (round 6, VERDICT r5 #1: the roofline's 2.4 GHz was never checked inside the kernels).
enum { kCsTable = 0, kCsItemPrologue, kCsAOperands, kCsNextGroup, kCsLoop, kCsLoopWait, kCsFlush, kCsOther, kCensusPhases };
#define PVV_CENSUS_IN() long long cs_last = 0; __shared__ long long s_cs[16]; \
    do { if (threadIdx.x == 0) { for (int i_ = 0; i_ < 16; ++i_) s_cs[i_] = 0; s_cs[0] = wall_clock64(); \
    s_cs[2] = (long long)__builtin_amdgcn_s_getreg(63492) | ((long long)__builtin_amdgcn_s_getreg(63508) << 32); \
    cs_last = (long long)__builtin_readcyclecounter(); } } while (0)
#define PVV_CS(i) do { if (threadIdx.x == 0) { const long long t_ = (long long)__builtin_readcyclecounter(); s_cs[4 + (i)] += t_ - cs_last; cs_last = t_; } } while (0)
#define PVV_CS_RT_IN() long long cs_rt = 0; do { if (threadIdx.x == 0) cs_rt = wall_clock64(); } while (0)
#define PVV_CS_RT_OUT(tiles) do { if (threadIdx.x == 0) { s_cs[12] += wall_clock64() - cs_rt; s_cs[13] += (tiles); } } while (0)
#define PVV_CENSUS_OUT(n) do { if (dbg && threadIdx.x == 0) { s_cs[1] = wall_clock64(); s_cs[3] = (n); \
    for (int i_ = 0; i_ < 16; ++i_) dbg[64 + 16 * (size_t)blockIdx.x + i_] = s_cs[i_]; } } while (0)
#else
#define PVV_STAMP(i) do { } while (0)
#define PVV_CENSUS_IN() do { } while (0)
#define PVV_CS(i) do { } while (0)
#define PVV_CS_RT_IN() do { } while (0)
#define PVV_CS_RT_OUT(tiles) do { } while (0)
#define PVV_CENSUS_OUT(n) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// Staged counting (ransac_voting_layer_v3 only): the layer needs the ARG-MAX of the counts and the winner's count
// (P:160-167), not the counts.  Two launches instead of one:
//   k_count_bf16<kCountFirst>   every hypothesis over the 512-pixel chunks whose index has a residue (mod M) in `mask`
//                               -- a quarter of an image's chunks, spread over the object;
//   k_lead (count_prune.hpp)    two leaders per (image, keypoint): their partial counts plus their SURE inliers among all
//                               the other pixels = lower bounds of two full counts; L* = the larger;
//   k_count_bf16<kCountFilter>  the other chunks, but only for hypotheses h with  partial(h) + R >= L*  (R = pixels not
//                               counted by the first launch): every other hypothesis has full(h) <= partial(h) + R < L*
//                               <= max and can neither win nor tie.  The filter is evaluated on the fly while a block
//                               stages its hypotheses (count, bound and four leader numbers per (image, keypoint): no
//                               survivor lists in memory); it reads counters that other blocks of the same launch are
//                               adding to, which is benign: a dropped hypothesis is never counted, so its counter never
//                               moves, and a kept one only grows -- the predicate is the same for every reader.
// Kept hypotheses end with their exact full count, dropped ones with a partial count below the maximum: winner, first-index
// tie rule and winner count are those of the full pass, bit for bit.  Images of fewer than n_min chunks are counted
// completely by the first launch (nothing to gain from a bound taken after half of their pixels).
// ---------------------------------------------------------------------------------------------
enum { kCountFull = 0, kCountFirst = 1, kCountFilter = 2 };

// The chunk schedule, compile-time (every index computation below is then shifts and constant multiplies; as run-time
// parameters they were a dozen integer divisions per work item): the first launch counts the 512-pixel chunks c with
// (c mod 8) in {1, 5} -- a quarter of the chunks, spread over the object (rows of the compacted list = raster order) --,
// the second launch the other residues; images of fewer than kStageMinChunks chunks are counted completely by the first.
// (kStageM, kStageMinChunks and the chunk length are stated in vote_common.hpp: the compaction needs them too.)
static_assert(4 * kBfPixPerWave == kStageChunkRows, "a chunk is what one block of the count kernels walks per item");
constexpr uint32_t kStageFirst = PVV_STAGE_FIRST;
// Round 4: with the second launch eliminating as it goes (count_filter_runs.hpp) a SMALLER first stage pays once its runs are
// long: an eighth of the chunks ({1} of 8) instead of a quarter is -4 % per call at config 3 / B = 128 and -9 % on config 5 /
// B = 16, +3 % at B = 64 and below (one-process A/B, profiles/DESIGN_rounds_1-4.md 4.7).  The schedule is a template parameter of the three kernels
// of the pass; the host picks it from the problem's size (launch_count_bf16).
constexpr uint32_t kStageFirstEighth = 0x02u;
constexpr uint32_t stage_rest_of(uint32_t first) { return ((1u << kStageM) - 1u) & ~first; }

struct StageArgs {
    const int *lead;      // kCountFilter: [B,K,8] leaders' partial counts [0..3] (-1: none) and their SURE inliers among the
                          // pixels the first launch did not count [4..7] (k_lead)
    int *any_staged;      // one word: kCountFirst writes whether ANY image is staged; k_lead and kCountFilter leave at once
                          // when none is (a batch of small masks then pays two empty launches, not two table builds)
    int *miss;            // k_count_filter_runs: [B,K,hn] misses proven so far among the pixels the first launch did not count
                          // (zeroed by k_compact_hyp; count_filter_runs.hpp)
    int sub_tenth;        // 1: the caller is estimate_voting_distribution_with_mean, which weighs every hypothesis whose ratio is
                          // within 0.1 of the best (P:262-264): the elimination bound is lowered accordingly (stage_bound)
    const float2 *mean;   // k_count_filter_runs, the estimate: [B,K] the keypoints the covariance is taken about, or nullptr.  Not
                          // nullptr: a run walks its chunks NEAREST (in y) to the keypoint first -- see the chunk order there
    int hstride;          // row length of hyps / counts / miss when the hn hypotheses counted are a column range of longer rows (the
                          // fused un_pnp call counts its 512 + 4096 hypotheses as two passes over one compaction); 0: hn
#ifdef PVV_STAMPS
    long long *dbg;       // instrumented builds: the phase census of k_count_filter_runs (count_filter_runs.hpp)
#endif
};

// chunks with a residue in `mask` among the first n chunks, and the j-th of them (residues present in a last, partial
// period are a prefix of the sorted residues, so the j-th chunk does not depend on n)
template <uint32_t MASK>
__device__ __forceinline__ int stage_chunks(int n)
{
    return (n / kStageM) * __builtin_popcount(MASK) + __popc(MASK & ((1u << (n % kStageM)) - 1u));
}
template <uint32_t MASK>
__device__ __forceinline__ int stage_chunk_at(int j)
{
    constexpr int m = __builtin_popcount(MASK);
    const int per = j / m;
    uint32_t t = MASK;
    for (int k = j - per * m; k > 0; --k) t &= t - 1u;
    return per * kStageM + __builtin_ctz(t);
}
// pixels of an image of tn pixels (nch chunks of PC) that lie in chunks with a residue in MASK
template <uint32_t MASK>
__device__ __forceinline__ int stage_pixels(int tn, int nch, int PC)
{
    return stage_chunks<MASK>(nch) * PC - (((MASK >> ((nch - 1) % kStageM)) & 1u) ? nch * PC - tn : 0);
}

// ---------------------------------------------------------------------------------------------
// Gather blocks of the first count launch.  Its count blocks read only the rows of their own chunks, and from about half of its span
// on a growing part of the chip's block slots is empty (1728 items on 1280 slots at config 3 / B = 64); k_lead, the second launch and
// the refit read the other rows one launch later.  So for the images k_compact_hyp marked (HypArgs.deferred: staged, not subsampled)
// the rows of the REST chunks are gathered here instead of in front of the count pass: the host adds G blocks to the grid, which leave
// through gather_deferred_rows before the item loop.  A unit is one rest chunk of one image, all K keypoints, two rows per thread;
// gather block i walks units i, i + G, ...  Nothing in the launch waits for another of its blocks: count blocks never read a rest
// chunk of a deferred image, gather blocks never write anything else.
// Where in the grid: right behind the first resident generation of count blocks (k_count_bf16: g_first), not at the top.  At the top
// they queue behind the ~2500 count blocks of the 15-per-CU grid that only pass through, start in the launch's last quarter and
// lengthen it by 9-13 us where k_compact_hyp saves 6.4; at the bottom they hold back 256 count blocks per G / CU (+6.4 us at one
// per CU); behind the first generation they take the first slots it frees: +3.3 ... 4.4 us (profiles/deferred_rows_kernel_stats.json).
// ---------------------------------------------------------------------------------------------
struct GatherArgs {
    int G;                // gather blocks in the grid; 0: none (every row was gathered by k_compact_hyp)
    int vt;               // element type of the vertex field (kElem*): a run-time switch, the branch is cold
    const int *deferred;  // [B] k_compact_hyp's flags
    float2 *dirs;         // the planar rows (the kernel's own `dirs` is its read-only view of the first-stage rows)
    VertexArgs v;
};

// rows [pb, pb + 512) of image b below tn: coords -> pixel (exact integers) -> the K vertex pairs -> dirs
template <int VT>
__device__ __forceinline__ void gather_unit(const GatherArgs &ga, const float2 *__restrict__ crd, int b, int pb, int tn, int cap)
{
    // An f32 gather in flight holds four registers (a 64-bit address: the strides are the caller's; the pair): the two rows of a thread
    // go one after the other, kKeys gathers each, so that the branch stays far below the count kernel's 96 (no scratch).
    constexpr int kKeys = 10;                                            // gathers in flight (K = 9: one trip per row)
    const int r0 = pb + (int)threadIdx.x, r1 = r0 + kBlock;
    const float2 c0 = r0 < tn ? crd[r0] : make_float2(0.f, 0.f), c1 = r1 < tn ? crd[r1] : make_float2(0.f, 0.f);
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        const int row = q ? r1 : r0;
        if (row >= tn) break;
        const int x = (int)(q ? c1.x : c0.x), y = (int)(q ? c1.y : c0.y);
        float2 *drow = ga.dirs + (size_t)b * ga.v.K * cap + row;
        for (int v0 = 0; v0 < ga.v.K; v0 += kKeys) {
            typename VertexRaw<VT>::type d[kKeys];
#pragma unroll
            for (int u = 0; u < kKeys; ++u)
                if (v0 + u < ga.v.K) d[u] = load_vertex<VT>(ga.v, b, y, x, v0 + u);
#pragma unroll
            for (int u = 0; u < kKeys; ++u)
                if (v0 + u < ga.v.K) drow[(size_t)(v0 + u) * cap] = widen_vertex<VT>(ga.v, d[u]);
        }
    }
}

// A gather block's whole life (gi: its index among the G).  chunk_end: the count kernel's table, here the inclusive prefix of the
// deferred images' rest chunks.
template <uint32_t REST>
__device__ __forceinline__ void gather_deferred_rows(const GatherArgs &ga, int gi, int *chunk_end, const float2 *__restrict__ coords,
                                                     const int *__restrict__ tn_arr, int B, int cap)
{
    const int lane = lane_id();
    if (wave_id() == 0) {
        int carry = 0;
        for (int b0 = 0; b0 < B; b0 += 64) {
            const int b = b0 + lane;
            int inc = 0;
            if (b < B && ga.deferred[b] != 0) inc = stage_chunks<REST>((tn_arr[b] + kStageChunkRows - 1) >> kStageChunkShift);
            inc = wave_incl_scan(inc) + carry;
            if (b < B) chunk_end[b] = inc;
            carry = __builtin_amdgcn_readlane(inc, 63);
        }
    }
    __syncthreads();
    const int units = chunk_end[B - 1];
    for (int u = gi; u < units; u += ga.G) {
        int local;
        const int b = locate_item(chunk_end, B, u, &local);
        const int pb = stage_chunk_at<REST>(local) << kStageChunkShift;
        const int tn = tn_arr[b];
        const float2 *crd = coords + (size_t)b * cap;
        if (ga.vt == kElemF16) gather_unit<kElemF16>(ga, crd, b, pb, tn, cap);
        else if (ga.vt == kElemBF16) gather_unit<kElemBF16>(ga, crd, b, pb, tn, cap);
        else gather_unit<kElemF32>(ga, crd, b, pb, tn, cap);
    }
}

// 5 blocks (= 5 waves per SIMD) per CU: <= 96 VGPRs and 30 KB of LDS per block; measured -4.4 % against 4
// GATHER (first launch only): the launch carries gather blocks.  A launch without deferred rows runs the instantiation without
// the branch, whose code is the one the kernel had before there were gather blocks (the branch costs the item prologue a dozen
// SGPR spill moves: the register allocation is one for the whole kernel).
// `dirs` is __restrict__ and read-only here while gather blocks write the same array through GatherArgs.dirs: that holds because no
// thread does both -- a gather block leaves before anything reads `dirs`, and must never read it -- and because count blocks read
// only first-stage chunks of a deferred image, gather blocks write only its rest chunks.
template <int MODE, uint32_t FIRST = kStageFirst, bool GATHER = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_count_bf16(
    const float2 *__restrict__ coords /*[B,cap]*/, const float2 *__restrict__ dirs /*[B,K,cap]*/,
    const float2 *__restrict__ hyps /*[B,K,hn]*/, int *__restrict__ counts /*[B,K,hn]*/,
    const int *__restrict__ tn_arr, int B, int K, int hn, int cap, float thresh, Bf16Consts fc, int target_items,
    long long *__restrict__ dbg /*tuning builds: phase timestamps; nullptr otherwise*/, StageArgs sa, GatherArgs ga /*GATHER only*/)
{
    PVV_STAMP(0);
    PVV_CENSUS_IN();
    int n_items_done = 0;
    __shared__ int chunk_end[kMaxBatchLds];         // inclusive prefix of the 512-pixel chunks per image
    __shared__ int s_htpi, s_gpi, s_chunks;
    __shared__ bf16x8 sB[kBfMaxHt * 64];            // B operands of the current hypothesis group (16 KB)
    __shared__ float4 sP[4 * kBfPixPerWave];        // per pixel: (nhx, nhy, c'x, c'y); nhx = NaN: can never vote  (8 KB)
    __shared__ int sCnt[kBfMaxHt * 32];
    __shared__ float sRed[4];
    __shared__ unsigned long long s_small[kMaxBatchLds / 64];   // staged: images counted completely by the first launch
    __shared__ int s_keep[8];                                   // kCountFilter: kept hypotheses per (pass, wave) of a group
    constexpr bool STAGED = MODE != kCountFull;
    constexpr bool FILTER = MODE == kCountFilter;
    constexpr uint32_t REST = stage_rest_of(FIRST);
    const int lane = lane_id(), wave = wave_id();
    constexpr int PC = 4 * kBfPixPerWave;
    const int nt = (hn + 31) >> 5;                  // 32-hypothesis tiles per keypoint
    const int hs = sa.hstride > 0 ? sa.hstride : hn; // row length of hyps / counts
    if constexpr (FILTER) if (*sa.any_staged == 0) return;
    // The count grid: the launch's blocks less the gather blocks, which leave here; bid: a count block's index in it.  The gather
    // blocks follow the first target_items count blocks -- one resident generation (5 per CU) -- in dispatch order, so they take the
    // first slots that generation frees, ahead of the count grid's other blocks, most of which only pass through (nblk below).
    static_assert(!GATHER || MODE == kCountFirst, "only the first launch of a staged pass gathers");
    const int n_gather = GATHER ? ga.G : 0;
    const int ngrid = (int)gridDim.x - n_gather;
    const int g_first = min(target_items, ngrid);
    const int bid = (int)blockIdx.x - ((int)blockIdx.x >= g_first ? n_gather : 0);
    if constexpr (GATHER) {
        if ((int)blockIdx.x >= g_first && bid < g_first) {
            gather_deferred_rows<REST>(ga, (int)blockIdx.x - g_first, chunk_end, coords, tn_arr, B, cap);
            return;
        }
    }

    // Work item = (image, keypoint, 512-pixel chunk, a run of hypothesis groups).  A group is up to 16 tiles (512
    // hypotheses, what fits the LDS staging); an item walks as many groups as possible (the pixel operands are
    // built once per item), fewer -- and smaller groups -- when the batch is too small to fill the chip.
    // ONE pass over tn[] by wave 0 gives the chunk prefix of the images (the item table: every block derives the same
    // one, no host sync) and, from the total, the item size.
    if (wave == 0) {
        int carry = 0;
        [[maybe_unused]] bool any_staged = false;
        for (int b0 = 0; b0 < B; b0 += 64) {
            const int b = b0 + lane;
            int inc = b < B ? (tn_arr[b] + PC - 1) / PC : 0;
            if constexpr (STAGED) {                                // this launch's chunks of the image
                const bool small = inc < kStageMinChunks;
                const unsigned long long sm = __ballot(small);
                any_staged |= sm != ~0ull;
                if (lane == 0) s_small[b0 >> 6] = sm;
                inc = small ? (MODE == kCountFirst ? inc : 0) : stage_chunks<MODE == kCountFirst ? FIRST : REST>(inc);
            }
            inc = wave_incl_scan(inc) + carry;
            if (b < B) chunk_end[b] = inc;
            carry = __builtin_amdgcn_readlane(inc, 63);
        }
        const long long chunks = (long long)carry * K;
        int htpi = min(nt, kBfMaxHt);
        int nhg = (nt + htpi - 1) / htpi;
        int gpi = nhg;                                              // groups per item
        // Long items (several 512-hypothesis groups behind one pixel-operand build) are split until there are THREE generations'
        // worth of them when the grid has that many blocks (B > 8: 15 or 48 per CU) -- 1296 eight-group items on 1280 block slots
        // (the 4096-hypothesis estimate at B = 12) leave 16 items a second round to themselves.  One-process A/B, count kernel,
        // 480x640, K = 9 (profiles/r04_experiments.txt (19)): 4096 hypotheses -19 % at B = 12, -10 % at 16, -7 % at 24, -4 % at 32,
        // +-0 from 48 on; 2048 hypotheses -7.5 % at B = 16; config 5's staged first launch -3 % at B = 16.  Not below B = 9 (the
        // one-generation grid walks its items round-robin: twice as many half-length items cost +9 % on config 5 at B = 2, and the
        // estimate at B = 8) and not for two groups (1024 hypotheses at B = 16: +1.6 %).
#ifndef PVV_GPI_FACTOR
#define PVV_GPI_FACTOR 3
#endif
        const long long gpi_target = (B > 8 && nhg >= 4) ? (long long)PVV_GPI_FACTOR * target_items : (long long)target_items;
        while (gpi > 1 && chunks * ((nhg + gpi - 1) / gpi) < gpi_target) gpi = (gpi + 1) >> 1;
        // groups below 4 tiles only for very small problems (< 128 (chunk, keypoint) pairs: every item they add is another
        // CU put to work); otherwise the prologue of an item is worth more than the 16 matrix-core tiles of a 2-tile group
        const int htpi_min = chunks < 128 ? 2 : 4;
        if (gpi == 1 && !FILTER)                                    // (the filter compacts groups of 512 hypotheses: no smaller ones)
            while (htpi > htpi_min && chunks * ((nt + htpi - 1) / htpi) < target_items) htpi = (htpi + 1) >> 1;
        if (lane == 0) { s_htpi = htpi; s_gpi = gpi; s_chunks = carry; }
        if constexpr (MODE == kCountFirst) if (bid == 0 && lane == 0) *sa.any_staged = any_staged ? 1 : 0;
    }
    __syncthreads();
    PVV_STAMP(1);
    const int htpi = __builtin_amdgcn_readfirstlane(s_htpi);
    const int gpi = __builtin_amdgcn_readfirstlane(s_gpi);
    const int nhg = (nt + htpi - 1) / htpi;          // hypothesis groups per keypoint
    const int nruns = (nhg + gpi - 1) / gpi;         // runs of groups = items per (chunk, keypoint)
    const int per_chunk = K * nruns;
    const int total = __builtin_amdgcn_readfirstlane(s_chunks) * per_chunk;
    PVV_STAMP(2);
    PVV_CS(kCsTable);

    // The host sizes the grid without knowing tn.  With few items (up to 7/4 of the one-generation grid = target_items)
    // only the first target_items blocks of a 15-per-CU grid take part -- one generation, a few blocks with two items,
    // measured faster than spreading them over three generations (B = 16: 54.9 vs 57.9 us) -- and the others leave here
    // (they pass through the slots the working blocks free: no measurable tail).  With many items every block works
    // (config 5 at B = 16: 1.43 vs 1.70 ms), and so does the 48-per-CU grid of the long-hypothesis configurations
    // (11 000 leaving blocks would be a tail: +10 % on config 4 at B = 16).
    const int nblk = (total <= target_items + (target_items >> 1) + (target_items >> 2) && ngrid > target_items &&
                      ngrid <= 3 * target_items) ? target_items : ngrid;
    if (bid >= nblk) return;
    // item -> (chunk over the whole batch, rest) without a division per item: both advance by a constant step
    const int step_q = nblk / per_chunk, step_r = nblk - step_q * per_chunk;
    int gchunk = bid / per_chunk, rem = bid - gchunk * per_chunk;
    for (int item = bid; item < total;
         item += nblk, gchunk += step_q + (rem + step_r >= per_chunk ? 1 : 0), rem += step_r - (rem + step_r >= per_chunk ? per_chunk : 0)) {
        int local;
        const int b = locate_item(chunk_end, B, gchunk, &local);   // image, and the chunk's index within it (this stage's)
        int chunk = local;
        if constexpr (STAGED)
            if (!((s_small[b >> 6] >> (b & 63)) & 1ull)) chunk = stage_chunk_at<MODE == kCountFirst ? FIRST : REST>(local);
        const int vi = nruns == 1 ? rem : rem / nruns;          // (one run per (chunk, keypoint) unless the batch is tiny)
        const int run = rem - vi * nruns;
        const int bk = b * K + vi;
        const float2 *hyp_k = hyps + (size_t)bk * hs;
        const float2 *crd = coords + (size_t)b * cap;
        const float2 *dir_k = dirs + (size_t)bk * cap;
        const int pb = chunk * PC;                              // first pixel of the block's chunk (< tn)
        const int g0 = run * gpi, g1 = min(nhg, g0 + gpi);

        __syncthreads();                                        // previous item's LDS fully consumed
        // The thread index, made opaque once per item: everything the prologue derives from it (addresses, row / slot
        // indices) is then recomputed per item instead of being hoisted out of the item loop and kept alive -- spilled --
        // across the matrix-core loop.  At the 96-register cap this removes every scratch access from the full and the
        // first-stage kernels (16 B -> 0) and a few from the filter kernel (52 B -> 44 B); -0.6 % per call at B = 64, -1 % at B = 1.
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        PVV_STAMP(3);
        PVV_CS(kCsOther);
        ++n_items_done;
        // ---- every global load of the item is issued here, before anything waits: tn, the chunk's origin, two pixels
        //      per thread (rows beyond tn are read -- the arrays reserve cap rows -- and masked below) and the
        //      hypotheses of the first group.  One memory round trip instead of three.
        const int tn_v = tn_arr[b];
        int lead_p = -1, lead_r = 0;                            // kCountFilter: a leader's partial count and its sure inliers in the rest
        if constexpr (FILTER) {
            lead_p = sa.lead[(size_t)bk * 8 + (lane & 3)];
            lead_r = sa.lead[(size_t)bk * 8 + 4 + (lane & 3)];
        }
        const float2 org = crd[pb];                             // integer origin: the chunk's first pixel
        float2 pc[2], pd[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = min(pb + tid + q * kBlock, cap - 1);
            pc[q] = crd[p];
            pd[q] = dir_k[p];
        }
        const int nht0 = min(nt, (g0 + 1) * htpi) - g0 * htpi;  // tiles of the first group
        float2 hp0[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + q * kBlock;
            const int h = (g0 * htpi + (i >> 5)) * 32 + (i & 31);
            hp0[q] = (i < nht0 * 32 && h < hn) ? hyp_k[h] : make_float2(0.f, 0.f);
        }
        int cnt0[2] = {0, 0};                                   // kCountFilter: the first launch's counts of those hypotheses
        if constexpr (FILTER) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = tid + q * kBlock;
                const int h = g0 * htpi * 32 + i;
                if (i < nht0 * 32 && h < hn) cnt0[q] = counts[(size_t)bk * hs + h];
            }
        }
        const int tn = __builtin_amdgcn_readfirstlane(tn_v);
        // kCountFilter: R = pixels of the image the first launch did not count; L* = the larger of the leaders' lower bounds (k_lead)
        int R_rem = 0, lstar = 0, ns_g = 0;
        if constexpr (FILTER) {
            R_rem = stage_pixels<REST>(tn, (tn + PC - 1) / PC, PC);
            lstar = leaders_bound(lead_p, lead_r, tn, sa.sub_tenth);
        }
        // kCountFilter: stage only the hypotheses of group g that can still reach L*, densely from slot 0 (order = pass,
        // wave, lane: irrelevant, the counter word carries the hypothesis' index within the group in its high half); pads
        // the last tile with (0,0) hypotheses.  Contains one barrier (compact_kept); returns the far flag of stage_b_operand.
        auto stage_kept = [&](int g, const int (&cnt)[2], const float2 (&hp)[2]) -> int {
            bool keep[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = tid + q * kBlock;
                keep[q] = i < htpi * 32 && g * htpi * 32 + i < hn && cnt[q] + R_rem >= lstar;
            }
            int slot[2];
            const int tot = compact_kept(s_keep, keep, lane, wave, slot);
            int f = 0;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (keep[q]) {
                    f |= stage_b_operand(sB, slot[q], hp[q], org);
                    sCnt[slot[q]] = (int)(tid + q * kBlock) << 16;
                }
            const int pad = ((tot + 31) & ~31) - tot;
            if (tid < pad) {
                stage_b_operand(sB, tot + tid, make_float2(0.f, 0.f), org);
                sCnt[tot + tid] = 0;
            }
            ns_g = tot;
            return f;
        };

        // ---- per pixel (two per thread): the f32 unit normal and the translated coordinates in sP, the waves' c1 in sRed
        pixel_records(sP, sRed, pc, pd, org, tid, pb, tn, lane, wave);
        // ---- B operands of the first group (stage_b_operand; a hypothesis' LDS counter starts at zero and is flushed by
        //      the same thread later)
        int far = 0;
        if constexpr (FILTER) {
            far = stage_kept(g0, cnt0, hp0);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = tid + q * kBlock;
                if (i < nht0 * 32) {
                    far |= stage_b_operand(sB, i, hp0[q], org);
                    sCnt[i] = 0;
                }
            }
        }
        far = __syncthreads_or(far);
        PVV_STAMP(4);
        PVV_CS(kCsItemPrologue);
        const float C1 = fmaxf(fmaxf(sRed[0], sRed[1]), fmaxf(sRed[2], sRed[3]));
        const float eps = fc.eps0 + fc.eps_c * C1;
        const float epsw = __builtin_fmaf(fc.beta * 1.02f, C1, eps);   // band half-width at |h'| = 0

        // 16-pixel tiles of the chunk go round-robin to the 4 waves (tile 4*j + wave is this wave's j-th): a partial
        // chunk keeps all four waves busy and nobody multiplies tiles that hold no pixel
        const int ntile_c = (min(tn - pb, PC) + 15) >> 4;       // tiles of the chunk with at least one pixel (1..32)
        const int ntile_w = (ntile_c - wave + 3) >> 2;          // this wave's share (0..8)

        // ---- A operands, built once per item
        bf16x8 A[8];
        build_a_operands(sP, fc, wave, lane, ntile_w, A);
        PVV_STAMP(5);
        PVV_CS(kCsAOperands);

        for (int g = g0; g < g1; ++g) {
            const int ht0 = g * htpi;
            if (g > g0) {
                // ---- B operands of the next group (the first group's were staged with the pixels)
                far = 0;
                if constexpr (FILTER) {
                    int cnt[2] = {0, 0};
                    float2 hp[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int i = threadIdx.x + q * kBlock;
                        const int h = ht0 * 32 + i;
                        if (i < htpi * 32 && h < hn) { cnt[q] = counts[(size_t)bk * hs + h]; hp[q] = hyp_k[h]; }
                    }
                    far = stage_kept(g, cnt, hp);
                } else {
                    const int nhtg = min(nt, ht0 + htpi) - ht0;
                    for (int i = threadIdx.x; i < nhtg * 32; i += kBlock) {
                        const int h = (ht0 + (i >> 5)) * 32 + (i & 31);
                        far |= stage_b_operand(sB, i, h < hn ? hyp_k[h] : make_float2(0.f, 0.f), org);
                        sCnt[i] = 0;
                    }
                }
                far = __syncthreads_or(far);
            }
            // tiles of this group: its kept hypotheses (filter) or all of them; slot s of the staging holds hypothesis
            // ht0*32 + s, or -- filter -- ht0*32 + (sCnt[s] >> 16)
            const int nht = FILTER ? (ns_g + 31) >> 5 : min(nt, ht0 + htpi) - ht0;
            const int nslot = FILTER ? ns_g : min(hn - ht0 * 32, nht * 32);
            PVV_STAMP(6);
            PVV_CS(kCsNextGroup);
            PVV_CS_RT_IN();

            // slot s of the staging -> its un-translated hypothesis
            const auto hyp_of = [&](int slot) -> float2 { return hyp_k[ht0 * 32 + (FILTER ? sCnt[slot] >> 16 : slot)]; };
            if (__builtin_expect(far, 0))   // some hypothesis of the group is non-finite / astronomically far: exact loop (K:100-125)
                count_group_exact(sCnt, nht, nslot, wave, lane, pb, tn, crd, dir_k, thresh, hyp_of);
            else if (ntile_w > 0)
                count_tiles(sB, sP, sCnt, A, fc, eps, epsw, nht, nslot, ntile_w, wave, lane, pb, tn, org, crd, dir_k, thresh, hyp_of);
            PVV_STAMP(7);
            PVV_CS(kCsLoop);
            PVV_CS_RT_OUT(nht * ntile_w);
            __syncthreads();
            PVV_CS(kCsLoopWait);
            for (int i = threadIdx.x; i < nslot; i += kBlock) {
                const int v = sCnt[i];
                const int c = FILTER ? v & 0xffff : v;               // (filter: index within the group << 16 | count <= 512)
                if (c != 0) atomicAdd(&counts[(size_t)bk * hs + ht0 * 32 + (FILTER ? v >> 16 : i)], c);
            }
            PVV_STAMP(8);
            PVV_CS(kCsFlush);
        }
    }
    PVV_STAMP(9);
    PVV_CS(kCsOther);
    PVV_CENSUS_OUT(n_items_done);
    (void)n_items_done;
}
