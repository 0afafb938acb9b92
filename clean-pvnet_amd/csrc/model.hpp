// model.hpp -- from a mesh's vertices to the metadata every later stage consumes (include/pvnet_vote.h, "Model metadata"):
// farthest point sampling, the bounding box and the diameter, for a padded batch of clouds.
// Included at the end of pvnet_vote.hip: built with -ffp-contract=off, so d2 below rounds once per operation in the order
// written, in float32 for the sampling and in binary64 for the diameter.  The numpy twin (tests/model_twin.py) gives the
// same bits.
//
// Reference behaviour restated (paths relative to the reference's root):
//   F = lib/csrc/fps/src/farthest_point_sampling.cpp    M = lib/utils/vsd/misc.py    H = tools/handle_custom_dataset.py
//
// No workgroup waits for another anywhere in this file: stream order between launches is the only synchronisation across
// workgroups, every __syncthreads() sits in control flow that is uniform over its workgroup (n_b, sn, cur, the tile numbers
// and the kernel arguments are), and every global index is formed under its bound (a point index < n_b <= N, a tile < T).
#pragma once

#include <cfloat>
#include <limits>

namespace {

constexpr int kModelPer = 4;                          // points of a lane in the tiled kernels
constexpr int kModelTile = kBlock * kModelPer;        // 1024 points per workgroup
constexpr int kFpsBlock = 1024;                       // the ONE_BLOCK workgroup: 16 waves
constexpr int kFpsWaves = kFpsBlock / 64;
constexpr int kFpsPer = PVV_FPS_ONE_BLOCK_MAX / kFpsBlock;   // points of a lane at the largest cloud ONE_BLOCK takes
constexpr int kModelWaves = kBlock / 64;

static_assert(kModelTile == PVV_MODEL_TILE && kFpsPer == 8 && kFpsPer * kFpsBlock == PVV_FPS_ONE_BLOCK_MAX, "the header states these");
static_assert(PVV_MODEL_MAX_N % kModelTile == 0 && PVV_MODEL_MAX_N / kModelTile <= 1024, "grid.y of the pair kernel");

typedef unsigned long long model_u64;

// n_b: the length of cloud b, held to [1, N] whatever the array says (the wrapper validated it; a bound is a bound).
__device__ __forceinline__ int model_len(const int *__restrict__ n, int b, int N)
{
    return n ? min(max(n[b], 1), N) : N;
}

// F:25, 51: (p - q).squared_norm(), float32.
__device__ __forceinline__ float fps_d2(float px, float py, float pz, float qx, float qy, float qz)
{
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// min_dist is not negative, so its bit pattern orders as its value; the complemented index makes the lowest index win a tie
// (F:66: only a strictly larger distance replaces the running maximum).  A chosen point contributes key 0.
__device__ __forceinline__ model_u64 fps_key(float d, int i)
{
    return ((model_u64)__float_as_uint(d) << 32) | (unsigned)~i;
}

// F:61-62, 66: nothing is larger than 0 => index 0, chosen or not.
__device__ __forceinline__ int fps_pick(model_u64 key, int nb)
{
    if ((key >> 32) == 0) return 0;
    const unsigned i = ~(unsigned)key;
    return i < (unsigned)nb ? (int)i : 0;
}

__device__ __forceinline__ model_u64 u64_max(model_u64 a, model_u64 b) { return a > b ? a : b; }

// The maximum over the workgroup, in every lane.  `s` [WAVES] must not be written again before every lane has read it: the
// callers alternate two buffers or use each buffer once.
template <int WAVES>
__device__ __forceinline__ model_u64 block_max_u64(model_u64 v, model_u64 *s)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = u64_max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    model_u64 r = s[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = u64_max(r, s[w]);
    return r;
}

// The box over the workgroup, in every lane; `s` [WAVES * 6] is used once per kernel.
template <typename T, int WAVES>
__device__ __forceinline__ void block_box(T (&lo)[3], T (&hi)[3], T *s)
{
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const T a = __shfl_xor(lo[c], o), b = __shfl_xor(hi[c], o);
            lo[c] = a < lo[c] ? a : lo[c], hi[c] = b > hi[c] ? b : hi[c];
        }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[(threadIdx.x >> 6) * 6 + c] = lo[c], s[(threadIdx.x >> 6) * 6 + 3 + c] = hi[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = s[c], hi[c] = s[3 + c];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const T a = s[w * 6 + c], b = s[w * 6 + 3 + c];
            lo[c] = a < lo[c] ? a : lo[c], hi[c] = b > hi[c] ? b : hi[c];
        }
    }
}

// F:138: (max + min) / 2.f is written there as * (1.f / 2.f).      F:141: std::min(d, FLT_MAX) keeps d unless FLT_MAX < d.
__device__ __forceinline__ float fps_centre_dist(float px, float py, float pz, const float (&lo)[3], const float (&hi)[3])
{
    const float d = fps_d2(px, py, pz, (hi[0] + lo[0]) * 0.5f, (hi[1] + lo[1]) * 0.5f, (hi[2] + lo[2]) * 0.5f);
    return FLT_MAX < d ? FLT_MAX : d;
}

// ---------------------------------------------------------------------------------------------------- FPS, ONE_BLOCK
// One workgroup per cloud, one launch: point j * kFpsBlock + tid and its min_dist live in lane tid's registers, bit j of
// `alive` says that the point exists and is not chosen.  Every round ends in block_max_u64 of the lanes' keys.
template <int PER>
__global__ __launch_bounds__(kFpsBlock) void k_fps_one_block(const float *__restrict__ pts, const int *__restrict__ n,
                                                             const int *__restrict__ start, int N, int sn, int *__restrict__ idx)
{
    __shared__ float s_box[kFpsWaves * 6];
    __shared__ model_u64 s_key[2][kFpsWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int nb = model_len(n, b, N);
    const float *p = pts + (size_t)b * N * 3;

    float px[PER], py[PER], pz[PER], md[PER];
    unsigned alive = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * kFpsBlock + tid;
        px[j] = py[j] = pz[j] = 0.f, md[j] = FLT_MAX;
        if (i < nb) px[j] = p[3 * (size_t)i], py[j] = p[3 * (size_t)i + 1], pz[j] = p[3 * (size_t)i + 2], alive |= 1u << j;
    }

    int cur;
    if (start) {
        cur = min(max(start[b], 0), nb - 1);
    } else {
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (alive >> j & 1) {
                lo[0] = fminf(lo[0], px[j]), lo[1] = fminf(lo[1], py[j]), lo[2] = fminf(lo[2], pz[j]);
                hi[0] = fmaxf(hi[0], px[j]), hi[1] = fmaxf(hi[1], py[j]), hi[2] = fmaxf(hi[2], pz[j]);
            }
        block_box<float, kFpsWaves>(lo, hi, s_box);
        model_u64 key = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (alive >> j & 1) {
                md[j] = fps_centre_dist(px[j], py[j], pz[j], lo, hi);
                key = u64_max(key, fps_key(md[j], j * kFpsBlock + tid));
            }
        cur = fps_pick(block_max_u64<kFpsWaves>(key, s_key[1]), nb);       // round 0 writes s_key[0]
    }

    for (int k = 0; k < sn; ++k) {
        if (tid == 0) idx[(size_t)b * sn + k] = cur;
        if (k == sn - 1) break;
        const float cx = p[3 * (size_t)cur], cy = p[3 * (size_t)cur + 1], cz = p[3 * (size_t)cur + 2];      // cur < nb
        model_u64 key = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = j * kFpsBlock + tid;
            if (i == cur) alive &= ~(1u << j);
            if (alive >> j & 1) {
                const float d = fps_d2(px[j], py[j], pz[j], cx, cy, cz);
                if (d < md[j]) md[j] = d;
                key = u64_max(key, fps_key(md[j], i));
            }
        }
        cur = fps_pick(block_max_u64<kFpsWaves>(key, s_key[k & 1]), nb);
    }
}

// ---------------------------------------------------------------------------------------------------- boxes
// boxes [B][T][6]: lo then hi of tile t of cloud b; a tile that lies beyond n_b holds (+max, -max).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_box_tiles(const T *__restrict__ pts, const int *__restrict__ n, int N, int tiles,
                                                      T *__restrict__ boxes)
{
    __shared__ T s_box[kModelWaves * 6];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int nb = model_len(n, b, N);
    const T *p = pts + (size_t)b * N * 3;
    constexpr T big = std::numeric_limits<T>::max();
    T lo[3] = {big, big, big}, hi[3] = {-big, -big, -big};
#pragma unroll
    for (int r = 0; r < kModelPer; ++r) {
        const int i = tile * kModelTile + r * kBlock + tid;
        if (i < nb)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T v = p[3 * (size_t)i + c];
                lo[c] = v < lo[c] ? v : lo[c], hi[c] = v > hi[c] ? v : hi[c];
            }
    }
    block_box<T, kModelWaves>(lo, hi, s_box);
    if (tid == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) boxes[((size_t)b * tiles + tile) * 6 + c] = lo[c], boxes[((size_t)b * tiles + tile) * 6 + 3 + c] = hi[c];
}

// The box of cloud b from its tiles' boxes, in every lane.
template <typename T>
__device__ __forceinline__ void box_of_tiles(const T *__restrict__ boxes, int b, int tiles, T (&lo)[3], T (&hi)[3], T *s)
{
    constexpr T big = std::numeric_limits<T>::max();
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = big, hi[c] = -big;
    for (int q = threadIdx.x; q < tiles; q += kBlock)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T a = boxes[((size_t)b * tiles + q) * 6 + c], h = boxes[((size_t)b * tiles + q) * 6 + 3 + c];
            lo[c] = a < lo[c] ? a : lo[c], hi[c] = h > hi[c] ? h : hi[c];
        }
    block_box<T, kModelWaves>(lo, hi, s);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_box_finish(const T *__restrict__ boxes, int tiles, T *__restrict__ out_lo, T *__restrict__ out_hi)
{
    __shared__ T s_box[kModelWaves * 6];
    const int b = blockIdx.x;
    T lo[3], hi[3];
    box_of_tiles<T>(boxes, b, tiles, lo, hi, s_box);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) out_lo[(size_t)b * 3 + c] = lo[c], out_hi[(size_t)b * 3 + c] = hi[c];
}

// ---------------------------------------------------------------------------------------------------- FPS, TILED
// min_dist [B][N] lives in the workspace, -1 marks a chosen point; keys [2][B][T] hold every tile's winning key of the last
// round and of this one.  Grid (T, B) for k_fps_tile_init and k_fps_tile_step, (1, B) for the step that only finishes.
__global__ __launch_bounds__(kBlock) void k_fps_tile_init(const float *__restrict__ pts, const int *__restrict__ n, int N, int tiles,
                                                          const float *__restrict__ boxes, float *__restrict__ md,
                                                          model_u64 *__restrict__ keys)
{
    __shared__ float s_box[kModelWaves * 6];
    __shared__ model_u64 s_key[kModelWaves];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int nb = model_len(n, b, N);
    const float *p = pts + (size_t)b * N * 3;
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    if (boxes) box_of_tiles<float>(boxes, b, tiles, lo, hi, s_box);           // uniform: a kernel argument
    model_u64 key = 0;
#pragma unroll
    for (int r = 0; r < kModelPer; ++r) {
        const int i = tile * kModelTile + r * kBlock + tid;
        if (i < nb) {
            float m = FLT_MAX;
            if (boxes) {
                m = fps_centre_dist(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], lo, hi);
                key = u64_max(key, fps_key(m, i));
            }
            md[(size_t)b * N + i] = m;
        }
    }
    key = block_max_u64<kModelWaves>(key, s_key);
    if (tid == 0) keys[(size_t)b * tiles + tile] = key;
}

// Round k: every workgroup finds `cur` from the last round's tile keys (the same few hundred keys in every workgroup), then
// updates its tile and writes its key for the next round.  `last`: only idx[k] is written.
__global__ __launch_bounds__(kBlock) void k_fps_tile_step(const float *__restrict__ pts, const int *__restrict__ n,
                                                          const int *__restrict__ start, int N, int tiles, int sn, int k, int last,
                                                          float *__restrict__ md, const model_u64 *__restrict__ keys_in,
                                                          model_u64 *__restrict__ keys_out, int *__restrict__ idx)
{
    __shared__ model_u64 s_in[kModelWaves], s_out[kModelWaves];
    const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
    const int nb = model_len(n, b, N);
    const float *p = pts + (size_t)b * N * 3;
    int cur;
    if (start && k == 0) {                                                    // uniform: kernel arguments
        cur = min(max(start[b], 0), nb - 1);
    } else {
        model_u64 key = 0;
        for (int q = tid; q < tiles; q += kBlock) key = u64_max(key, keys_in[(size_t)b * tiles + q]);
        cur = fps_pick(block_max_u64<kModelWaves>(key, s_in), nb);
    }
    if (tile == 0 && tid == 0) idx[(size_t)b * sn + k] = cur;
    if (last) return;                                                         // uniform
    const float cx = p[3 * (size_t)cur], cy = p[3 * (size_t)cur + 1], cz = p[3 * (size_t)cur + 2];          // cur < nb
    model_u64 key = 0;
#pragma unroll
    for (int r = 0; r < kModelPer; ++r) {
        const int i = tile * kModelTile + r * kBlock + tid;
        if (i < nb) {
            float m = md[(size_t)b * N + i];
            if (i == cur) {
                md[(size_t)b * N + i] = -1.f;
            } else if (m != -1.f) {
                const float d = fps_d2(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2], cx, cy, cz);
                if (d < m) md[(size_t)b * N + i] = m = d;
                key = u64_max(key, fps_key(m, i));
            }
        }
    }
    key = block_max_u64<kModelWaves>(key, s_out);
    if (tid == 0) keys_out[(size_t)b * tiles + tile] = key;
}

// ---------------------------------------------------------------------------------------------------- diameter
// Grid (T, T, B); the workgroups with ti > tj leave at once, so each pair of tiles is visited once.  Tile tj is staged in LDS as
// binary64 and read as a broadcast, four points of tile ti sit in each lane's registers.  A slot whose point lies beyond n_b
// holds its tile's first point instead (a real point: it changes no maximum), so the loops run to bounds that come from N
// alone and the padding is never read.  best [B]: the bits of the largest d2, which order as the non-negative doubles do.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_diameter_pairs(const T *__restrict__ pts, const int *__restrict__ n, int N,
                                                           model_u64 *__restrict__ best)
{
    __shared__ double s_q[3][kModelTile];
    __shared__ model_u64 s_max[kModelWaves];
    const int tid = threadIdx.x, ti = blockIdx.x, tj = blockIdx.y, b = blockIdx.z;
    if (ti > tj) return;                                                      // uniform, before any barrier
    const int nb = model_len(n, b, N);
    if (tj * kModelTile >= nb) return;                                        // uniform; so ti * kModelTile < nb as well
    const T *p = pts + (size_t)b * N * 3;
    double ax[kModelPer], ay[kModelPer], az[kModelPer];
#pragma unroll
    for (int r = 0; r < kModelPer; ++r) {
        int i = ti * kModelTile + r * kBlock + tid;
        if (i >= nb) i = ti * kModelTile;
        ax[r] = (double)p[3 * (size_t)i], ay[r] = (double)p[3 * (size_t)i + 1], az[r] = (double)p[3 * (size_t)i + 2];
    }
    const int cj = min(kModelTile, N - tj * kModelTile);
    for (int e = tid; e < cj; e += kBlock) {
        int i = tj * kModelTile + e;
        if (i >= nb) i = tj * kModelTile;
        s_q[0][e] = (double)p[3 * (size_t)i], s_q[1][e] = (double)p[3 * (size_t)i + 1], s_q[2][e] = (double)p[3 * (size_t)i + 2];
    }
    __syncthreads();
    double m = 0.0;
    for (int j = 0; j < cj; ++j) {
        const double qx = s_q[0][j], qy = s_q[1][j], qz = s_q[2][j];
#pragma unroll
        for (int r = 0; r < kModelPer; ++r) {
            const double dx = ax[r] - qx, dy = ay[r] - qy, dz = az[r] - qz;
            const double d = (dx * dx + dy * dy) + dz * dz;
            m = d > m ? d : m;
        }
    }
    const model_u64 bits = block_max_u64<kModelWaves>((model_u64)__double_as_longlong(m), s_max);
    if (tid == 0) atomicMax(best + b, bits);
}

__global__ __launch_bounds__(kBlock) void k_diameter_finish(const model_u64 *__restrict__ best, int B, double *__restrict__ out)
{
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b < B) out[b] = sqrt(__longlong_as_double((long long)best[b]));
}

// ---------------------------------------------------------------------------------------------------- host
int model_tiles(int N) { return (N + kModelTile - 1) / kModelTile; }

size_t model_up(size_t v) { return (v + 255) & ~(size_t)255; }

int model_sizes(int B, int N)
{
    if (B <= 0 || N <= 0) return fail(PVV_E_ARG, "model: B and N must be positive");
    if (B > PVV_MODEL_MAX_B) return fail(PVV_E_ARG, "model: B > 65535: split the batch");
    if (N > PVV_MODEL_MAX_N) return fail(PVV_E_ARG, "model: N > 2^20 points: beyond the stated limit");
    if ((long long)B * model_tiles(N) > (1ll << 22)) return fail(PVV_E_ARG, "model: B * ceil(N / 1024) > 2^22: split the batch");
    return PVV_OK;
}

int fps_sizes(int B, int N, int sn, int path)
{
    if (int e = model_sizes(B, N)) return e;
    if (sn <= 0) return fail(PVV_E_ARG, "fps: sn must be positive");
    if (sn > PVV_MODEL_MAX_N || (long long)B * sn >= (1ll << 31)) return fail(PVV_E_ARG, "fps: sn > 2^20 or B * sn >= 2^31");
    if (path != PVV_FPS_AUTO && path != PVV_FPS_ONE_BLOCK && path != PVV_FPS_TILED) return fail(PVV_E_ARG, "fps: unknown path");
    if (path == PVV_FPS_ONE_BLOCK && N > PVV_FPS_ONE_BLOCK_MAX) return fail(PVV_E_ARG, "fps: ONE_BLOCK takes clouds of up to 8192 points");
    return PVV_OK;
}

bool fps_tiled(int N, int path) { return path == PVV_FPS_TILED || (path == PVV_FPS_AUTO && N > PVV_FPS_ONE_BLOCK_MAX); }

struct FpsLayout { size_t md, keys, boxes, total; };

FpsLayout fps_layout(int B, int N)
{
    const size_t T = (size_t)model_tiles(N);
    FpsLayout L;
    L.md = 0;
    L.keys = L.md + model_up(sizeof(float) * (size_t)B * N);
    L.boxes = L.keys + model_up(sizeof(model_u64) * 2 * B * T);
    L.total = L.boxes + model_up(sizeof(float) * 6 * B * T);
    return L;
}

struct ModelLayout { size_t boxes, best, total; };

ModelLayout model_layout(int B, int N)
{
    ModelLayout L;
    L.boxes = 0;
    L.best = L.boxes + model_up(sizeof(double) * 6 * (size_t)B * model_tiles(N));
    L.total = L.best + model_up(sizeof(model_u64) * (size_t)B);
    return L;
}

int model_ws(const void *ws, size_t ws_bytes, size_t need)
{
    if (!ws) return fail(PVV_E_ARG, "model: NULL workspace");
    if ((uintptr_t)ws % 256 != 0) return fail(PVV_E_ARG, "model: workspace must be 256-byte aligned");
    if (ws_bytes < need) return fail(PVV_E_WORKSPACE, "model: workspace too small");
    return PVV_OK;
}

template <typename T>
int model_bounds(const T *pts, const int *d_n, int B, int N, unsigned char *ws, T *lo, T *hi, hipStream_t st)
{
    const int tiles = model_tiles(N);
    T *boxes = (T *)(ws + model_layout(B, N).boxes);
    hipLaunchKernelGGL(k_box_tiles<T>, dim3(tiles, B), dim3(kBlock), 0, st, pts, d_n, N, tiles, boxes);
    if (int e = check_launch("k_box_tiles")) return e;
    hipLaunchKernelGGL(k_box_finish<T>, dim3(B), dim3(kBlock), 0, st, (const T *)boxes, tiles, lo, hi);
    return check_launch("k_box_finish");
}

template <typename T>
int model_diameter(const T *pts, const int *d_n, int B, int N, unsigned char *ws, double *out, hipStream_t st)
{
    const int tiles = model_tiles(N);
    if ((long long)B * tiles * tiles > (1ll << 22)) return fail(PVV_E_ARG, "diameter: B * ceil(N / 1024)^2 > 2^22: split the batch");
    model_u64 *best = (model_u64 *)(ws + model_layout(B, N).best);
    if (hipMemsetAsync(best, 0, sizeof(model_u64) * (size_t)B, st) != hipSuccess) return fail(PVV_E_ARG, "model: hipMemsetAsync failed");
    hipLaunchKernelGGL(k_diameter_pairs<T>, dim3(tiles, tiles, B), dim3(kBlock), 0, st, pts, d_n, N, best);
    if (int e = check_launch("k_diameter_pairs")) return e;
    hipLaunchKernelGGL(k_diameter_finish, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const model_u64 *)best, B, out);
    return check_launch("k_diameter_finish");
}

}  // namespace

PVV_EXPORT size_t pvv_fps_workspace_bytes(int B, int N, int sn, int path)
{
    if (fps_sizes(B, N, sn, path)) return 0;
    return fps_tiled(N, path) ? fps_layout(B, N).total : 256;
}

PVV_EXPORT int pvv_fps(const float *d_points, const int *d_n, const int *d_start, int B, int N, int sn, int path, void *workspace,
                       size_t workspace_bytes, int *d_idx, void *stream)
{
    if (int e = fps_sizes(B, N, sn, path)) return e;
    if (!d_points || !d_idx) return fail(PVV_E_ARG, "fps: NULL device pointer");
    const bool tiled = fps_tiled(N, path);
    if (int e = model_ws(workspace, workspace_bytes, tiled ? fps_layout(B, N).total : 256)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (!tiled) {
        if (N <= kFpsBlock) hipLaunchKernelGGL(k_fps_one_block<1>, dim3(B), dim3(kFpsBlock), 0, st, d_points, d_n, d_start, N, sn, d_idx);
        else hipLaunchKernelGGL(k_fps_one_block<kFpsPer>, dim3(B), dim3(kFpsBlock), 0, st, d_points, d_n, d_start, N, sn, d_idx);
        return check_launch("k_fps_one_block");
    }
    const int tiles = model_tiles(N);
    const FpsLayout L = fps_layout(B, N);
    unsigned char *ws = (unsigned char *)workspace;
    float *md = (float *)(ws + L.md), *boxes = (float *)(ws + L.boxes);
    model_u64 *keys[2] = {(model_u64 *)(ws + L.keys), (model_u64 *)(ws + L.keys) + (size_t)B * tiles};
    if (!d_start) {
        hipLaunchKernelGGL(k_box_tiles<float>, dim3(tiles, B), dim3(kBlock), 0, st, d_points, d_n, N, tiles, boxes);
        if (int e = check_launch("k_box_tiles")) return e;
    }
    hipLaunchKernelGGL(k_fps_tile_init, dim3(tiles, B), dim3(kBlock), 0, st, d_points, d_n, N, tiles, d_start ? (const float *)nullptr : boxes,
                       md, keys[0]);
    if (int e = check_launch("k_fps_tile_init")) return e;
    for (int k = 0; k < sn; ++k) {
        const int last = k == sn - 1;
        hipLaunchKernelGGL(k_fps_tile_step, dim3(last ? 1 : tiles, B), dim3(kBlock), 0, st, d_points, d_n, d_start, N, tiles, sn, k, last, md,
                           (const model_u64 *)keys[k & 1], keys[(k + 1) & 1], d_idx);
        if (int e = check_launch("k_fps_tile_step")) return e;
    }
    return PVV_OK;
}

PVV_EXPORT size_t pvv_model_workspace_bytes(int B, int N)
{
    if (model_sizes(B, N)) return 0;
    return model_layout(B, N).total;
}

PVV_EXPORT int pvv_model_bounds(const void *d_points, int is_f64, const int *d_n, int B, int N, void *workspace, size_t workspace_bytes,
                                void *d_lo, void *d_hi, void *stream)
{
    if (int e = model_sizes(B, N)) return e;
    if (!d_points || !d_lo || !d_hi) return fail(PVV_E_ARG, "model: NULL device pointer");
    if (int e = model_ws(workspace, workspace_bytes, model_layout(B, N).total)) return e;
    unsigned char *ws = (unsigned char *)workspace;
    if (is_f64) return model_bounds<double>((const double *)d_points, d_n, B, N, ws, (double *)d_lo, (double *)d_hi, (hipStream_t)stream);
    return model_bounds<float>((const float *)d_points, d_n, B, N, ws, (float *)d_lo, (float *)d_hi, (hipStream_t)stream);
}

PVV_EXPORT int pvv_model_diameter(const void *d_points, int is_f64, const int *d_n, int B, int N, void *workspace, size_t workspace_bytes,
                                  double *d_out, void *stream)
{
    if (int e = model_sizes(B, N)) return e;
    if (!d_points || !d_out) return fail(PVV_E_ARG, "model: NULL device pointer");
    if (int e = model_ws(workspace, workspace_bytes, model_layout(B, N).total)) return e;
    unsigned char *ws = (unsigned char *)workspace;
    if (is_f64) return model_diameter<double>((const double *)d_points, d_n, B, N, ws, d_out, (hipStream_t)stream);
    return model_diameter<float>((const float *)d_points, d_n, B, N, ws, d_out, (hipStream_t)stream);
}
