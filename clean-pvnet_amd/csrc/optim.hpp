// optim.hpp -- the clipped optimizer step of every parameter tensor in one launch (include/pvnet_vote.h, "Optimizer step").
//
// Reference behaviour restated (paths relative to the reference's root):
//   T = lib/train/trainers/trainer.py:42-45 (zero_grad, clip_grad_value_(..., 40), optimizer.step)
//   O = lib/train/optimizer.py:12-27 (one param group per tensor), R = lib/utils/optimizer/radam.py:29-95, torch.optim.Adam / SGD
//
// One block per chunk of PVV_OPTIM_CHUNK elements of one tensor.  The block finds its tensor by a binary search of the chunk
// prefix (uniform: scalar loads), reads the tensor's row of the table and streams p, g, m, v once: 16-byte loads and stores where
// the chunk's four addresses allow them, one element per lane otherwise and for the last numel % 4 elements.  Nothing outside
// [0, numel) of any tensor is touched.  float32, one rounding per operation of the header's contract, no fused multiply-add
// (-ffp-contract=off and the pragma of pvnet_vote.hip), `/` and sqrtf correctly rounded, subnormals kept: tests/optim_twin.py is
// the same arithmetic in numpy and the device equals it byte for byte.

namespace {

constexpr int kOptimChunk = PVV_OPTIM_CHUNK;
static_assert(kOptimChunk % (4 * kBlock) == 0, "a full chunk is a whole number of 16-byte rounds of the block");
static_assert(sizeof(pvv_optim_row) == 80 && offsetof(pvv_optim_row, numel) == 32 && offsetof(pvv_optim_row, s) == 48,
              "pvv_optim_row is laid out by the Python side as well");

// One element.  `s` and `rf` are the row's scalars and flags (the header says which is which per kind).
template <int KIND>
__device__ __forceinline__ void optim_element(float &p, float g, float &m, float &v, const float (&s)[8], int rf, bool clip, float c)
{
    if (clip) g = g < -c ? -c : (g > c ? c : g);             // comparisons: a NaN stays a NaN, as torch.clamp keeps it
    if (KIND == PVV_OPTIM_ADAM) {
        g = g + s[0] * p;
        m = m + s[1] * (g - m);
        v = v * s[2] + s[3] * (g * g);
        const float den = sqrtf(v) / s[4] + s[5];
        p = p + s[6] * (m / den);
    } else if (KIND == PVV_OPTIM_RADAM) {
        v = v * s[2] + s[3] * (g * g);
        m = m * s[0] + s[1] * g;
        if (!(rf & PVV_OPTIM_ROW_NO_UPDATE)) {
            if (rf & PVV_OPTIM_ROW_DECAY) p = p + s[5] * p;
            if (rf & PVV_OPTIM_ROW_ADAPTIVE) p = p + s[6] * (m / (sqrtf(v) + s[4]));
            else p = p + s[6] * m;
        }
    } else {
        g = g + s[0] * p;
        m = (rf & PVV_OPTIM_ROW_FIRST) ? g : m * s[1] + g;
        p = p + s[2] * m;
    }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void k_optim_step(const pvv_optim_row *__restrict__ rows, const int32_t *__restrict__ chunk_start,
                                                       int n_tensors, float c, int call_flags)
{
    constexpr bool kHasV = KIND != PVV_OPTIM_SGD;
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n_tensors;                               // chunk_start[lo] <= b < chunk_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= b) lo = mid; else hi = mid;
    }
    const pvv_optim_row r = rows[lo];
    const long long base = (long long)(b - chunk_start[lo]) * kOptimChunk;
    const long long left = r.numel - base;
    if (left <= 0) return;                                    // a prefix that disagrees with numel: nothing is touched
    const int cnt = left < kOptimChunk ? (int)left : kOptimChunk;
    float *const p = (float *)r.p + base, *const g = (float *)r.g + base, *const m = (float *)r.m + base;
    float *const v = kHasV ? (float *)r.v + base : nullptr;
    const bool clip = (call_flags & PVV_OPTIM_CLIP) != 0, zero = (call_flags & PVV_OPTIM_ZERO_GRAD) != 0;
    const bool first = KIND == PVV_OPTIM_SGD && (r.flags & PVV_OPTIM_ROW_FIRST);       // m is written, never read

    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    const int nvec = aligned ? cnt >> 2 : 0;
    for (int i = (int)threadIdx.x; i < nvec; i += kBlock) {
        float4 P = ((const float4 *)p)[i];
        const float4 G = ((const float4 *)g)[i];
        float4 M = first ? make_float4(0.f, 0.f, 0.f, 0.f) : ((const float4 *)m)[i];
        float4 V = kHasV ? ((const float4 *)v)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        optim_element<KIND>(P.x, G.x, M.x, V.x, r.s, r.flags, clip, c);
        optim_element<KIND>(P.y, G.y, M.y, V.y, r.s, r.flags, clip, c);
        optim_element<KIND>(P.z, G.z, M.z, V.z, r.s, r.flags, clip, c);
        optim_element<KIND>(P.w, G.w, M.w, V.w, r.s, r.flags, clip, c);
        ((float4 *)p)[i] = P;
        ((float4 *)m)[i] = M;
        if (kHasV) ((float4 *)v)[i] = V;
        if (zero) ((float4 *)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = nvec * 4 + (int)threadIdx.x; i < cnt; i += kBlock) {
        float P = p[i], M = first ? 0.f : m[i], V = kHasV ? v[i] : 0.f;
        optim_element<KIND>(P, g[i], M, V, r.s, r.flags, clip, c);
        p[i] = P;
        m[i] = M;
        if (kHasV) v[i] = V;
        if (zero) g[i] = 0.f;
    }
}

}  // namespace

PVV_EXPORT int pvv_optim_chunk(void) { return kOptimChunk; }

PVV_EXPORT int pvv_optim_step(int kind, const pvv_optim_row *d_rows, const int32_t *d_chunk_start, int n_tensors, long long n_chunks,
                              float clip_value, int flags, void *stream)
{
    if (kind != PVV_OPTIM_ADAM && kind != PVV_OPTIM_RADAM && kind != PVV_OPTIM_SGD) return fail(PVV_E_ARG, "optim: unknown kind");
    if (flags & ~(PVV_OPTIM_CLIP | PVV_OPTIM_ZERO_GRAD)) return fail(PVV_E_ARG, "optim: unknown bits in flags");
    if (n_tensors < 0 || n_chunks < n_tensors || n_chunks >= (1ll << 31))
        return fail(PVV_E_ARG, "optim: n_tensors >= 0 and n_tensors <= n_chunks < 2^31 (every row has a chunk)");
    if ((flags & PVV_OPTIM_CLIP) && !(clip_value >= 0.f)) return fail(PVV_E_ARG, "optim: clip_value must be >= 0");
    if (n_tensors == 0) return PVV_OK;
    if (!d_rows || !d_chunk_start) return fail(PVV_E_ARG, "optim: NULL device pointer");
    if (((uintptr_t)d_rows & 7) != 0 || ((uintptr_t)d_chunk_start & 3) != 0) return fail(PVV_E_ARG, "optim: the table must be 8-byte aligned");
    const dim3 grid((unsigned)n_chunks), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    if (kind == PVV_OPTIM_ADAM)
        hipLaunchKernelGGL(k_optim_step<PVV_OPTIM_ADAM>, grid, block, 0, st, d_rows, d_chunk_start, n_tensors, clip_value, flags);
    else if (kind == PVV_OPTIM_RADAM)
        hipLaunchKernelGGL(k_optim_step<PVV_OPTIM_RADAM>, grid, block, 0, st, d_rows, d_chunk_start, n_tensors, clip_value, flags);
    else
        hipLaunchKernelGGL(k_optim_step<PVV_OPTIM_SGD>, grid, block, 0, st, d_rows, d_chunk_start, n_tensors, clip_value, flags);
    return check_launch("k_optim_step");
}
