// render.hpp -- shaded colour images, instance labels and depth of a batch of scenes on the device (include/pvnet_vote.h,
// "Colour renders").  Included at the end of pvnet_vote.hip after ct_augment.hpp: built with -ffp-contract=off, every double
// operation below rounds once, in the order written, so that the numpy twin (tests/render_twin.py) gives the same bytes.
//
// The coverage rules (snapping, near clip, edge functions, the owns-its-line rule, the sweep by piece size) are those of
// raster.hpp, which the depth rasteriser of pvnet_vsd.hip draws with too; only the sink of a covered sample is this file's own.
//
//   k_rc_vertices  grid (vertex tiles, B*M): eye-space coordinates in binary64 and the snapped image coordinates of every
//                  (instance, vertex), once.
//   k_rc_raster    grid (tiles of 256 faces, B*M).  A lane sets up one face; a piece whose bounding box holds at most
//                  raster::kSmall samples is swept by its own lane, every other piece by the whole wave, 64 blocks of 8x8 samples at a
//                  time.  Every covered sample offers (bits of float32(Z) << 32) | (m << 24) | f to the 8-byte key image with one
//                  unsigned 64-bit atomicMin: nearest surface, then lowest instance, then lowest face.
//   k_rc_shade     one lane per four consecutive pixels of the flattened batch: the owner's colour, label, depth and face, or the
//                  background; 12 bytes of img leave as three dwords, label as one, depth and face as 16 bytes.  The last group
//                  (fewer than four pixels) is stored element by element.  Areas: an LDS histogram per block for the block's first
//                  image, one integer atomic per non-zero bin; a pixel of a later image in the same block adds directly.
//
// No float atomics.  Reference behaviour restated: lib/utils/linemod/opengl_renderer.py:171-179,
// lib/datasets/tless/opengl_renderer.py:150-156 (render(mode='rgb')), lib/utils/linemod/opengl_backend.py:21-67 (the shaders).
//
// Index bounds: instance = blockIdx.y < B*M; its object o is used only when 0 <= o < O and its range row satisfies
// 0 <= first, 0 <= count <= Nmax (Fmax), first + count <= N (F) -- tested on the device before anything is read through it
// (rc_range).  Vertex i < count <= Nmax indexes slot instance*Nmax + i of the workspace; a face row is used only when its three
// indices lie in [0, count).  Every sample a kernel touches satisfies 0 <= x < W and 0 <= y < H because a piece's bounding box is
// clamped to the image rectangle before it is swept; the key image of image b starts at b*H*W.  k_rc_shade: pixel p < B*H*W, the
// key's instance m < M and face f < count are tested again before the vertex slots are read; histogram bin = label <= M <= 255.
#pragma once

#include <climits>

namespace {

#include "raster.hpp"

constexpr int kRcMaxSide = 16384;
constexpr int kRcMaxM = 255;
constexpr int kRcMaxFaces = 1 << 24;
constexpr unsigned long long kRcEmpty = ~0ull;

static_assert(sizeof(raster::Vtx) == 32, "pvnet_vote.h promises 32 bytes per vertex slot");

struct RcRange { int v0, vn, f0, fn; bool ok; };

struct RcScene {                        // what the three kernels share
    const float *pts;
    const uint8_t *colors;
    const int32_t *faces, *ranges, *obj;
    const double *pose, *K;
    int N, F, O, Nmax, Fmax, K_batched, B, M, H, W;
    double near, far;
};

struct __attribute__((aligned(16))) RcVec4f { float v[4]; };
struct __attribute__((aligned(16))) RcVec4i { int v[4]; };
struct __attribute__((aligned(16))) RcVec2k { unsigned long long v[2]; };

__device__ bool rc_pose_finite(const double *P)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && isfinite(P[i]);
    return ok;
}

// The object of instance `inst` and its rows of the mesh, tested against the mesh before use; ok == false: no instance.
__device__ RcRange rc_range(const RcScene &s, int inst)
{
    RcRange r = {0, 0, 0, 0, false};
    const int o = s.obj ? s.obj[inst] : 0;
    if (o < 0 || o >= s.O) return r;
    const int32_t *q = s.ranges + 4 * (size_t)o;
    r.v0 = q[0], r.vn = q[1], r.f0 = q[2], r.fn = q[3];
    r.ok = r.v0 >= 0 && r.vn >= 0 && r.vn <= s.Nmax && r.v0 <= s.N - r.vn && r.f0 >= 0 && r.fn >= 0 && r.fn <= s.Fmax &&
           r.f0 <= s.F - r.fn;
    return r;
}

__global__ __launch_bounds__(kBlock) void k_rc_vertices(RcScene s, raster::Vtx *__restrict__ vtx)
{
    const int inst = blockIdx.y;
    const RcRange r = rc_range(s, inst);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (!r.ok || i >= r.vn) return;
    const raster::Cam c = raster::load_cam(s.K + (s.K_batched ? (size_t)(inst / s.M) * 9 : 0));
    const float *p = s.pts + ((size_t)r.v0 + i) * 3;
    vtx[(size_t)inst * s.Nmax + i] = raster::vertex(s.pose + (size_t)inst * 12, c, (double)p[0], (double)p[1], (double)p[2], s.near);
}

// The key sink: a covered sample offers (bits of float32(Z) << 32) | tag with one unsigned 64-bit atomicMin, tag = (m << 24) | f
// of the lane that owns the piece.
struct RcKeySink {
    unsigned long long *img;
    int W;
    double near, far;
    unsigned tag;

    __device__ void operator()(int x, int y, const raster::Plane &pl, const raster::Cam &c) const
    {
        double dx, dy, Z;
        if (!raster::plane_depth(pl, c, x, y, &dx, &dy, &Z)) return;
        if (Z >= near && Z <= far)
            atomicMin(img + (size_t)y * W + x, ((unsigned long long)__float_as_uint((float)Z) << 32) | tag);
    }

    __device__ RcKeySink of(int lane) const { return {img, W, near, far, (unsigned)raster::rl((int)tag, lane)}; }
};

__global__ __launch_bounds__(kBlock) void k_rc_raster(RcScene s, const raster::Vtx *__restrict__ vtx, unsigned long long *__restrict__ keys)
{
    const int inst = blockIdx.y;
    const RcRange r = rc_range(s, inst);
    if (!r.ok || !rc_pose_finite(s.pose + (size_t)inst * 12)) return;      // block-uniform: the instance draws nothing
    const int b = inst / s.M, m = inst - b * s.M;
    const raster::Cam c = raster::load_cam(s.K + (s.K_batched ? (size_t)b * 9 : 0));
    const int f = blockIdx.x * kBlock + threadIdx.x;
    raster::Face fc = {};                                                   // no piece
    if (f < r.fn) {
        const int32_t *row = s.faces + ((size_t)r.f0 + f) * 3;
        const int i0 = row[0], i1 = row[1], i2 = row[2];
        if (i0 >= 0 && i0 < r.vn && i1 >= 0 && i1 < r.vn && i2 >= 0 && i2 < r.vn) {
            const raster::Vtx *vp = vtx + (size_t)inst * s.Nmax;
            fc = raster::clip_face(c, vp[i0], vp[i1], vp[i2], s.near, s.W, s.H);
        }
    }
    const unsigned tag = ((unsigned)m << 24) | ((unsigned)f & 0xffffffu);   // f < fn <= 2^24 wherever a piece exists
    const RcKeySink sink = {keys + (size_t)b * s.H * s.W, s.W, s.near, s.far, tag};
    raster::sweep(fc.pc0, fc.pl, sink, c);
    if (__any(fc.pc1.w != 0)) raster::sweep(fc.pc1, fc.pl, sink, c);
}

struct RcPixel { uint8_t c[3], label; float z; int face; };

// Output 0 for v < 0 or NaN, 255 for v > 255, else floor(v + 0.5)
__device__ uint8_t rc_to_u8(double v)
{
    if (!(v >= 0.0)) return 0;
    if (v > 255.0) return 255;
    return (uint8_t)(int)floor(v + 0.5);
}

// The shading contract of the header for the owner (m, f) of pixel (x, y) of image b; false when the key names nothing that
// can be read (never for a key the raster wrote).
__device__ bool rc_shade_owner(const RcScene &s, const raster::Vtx *__restrict__ vtx, int b, int x, int y, int m, int f, double ambient,
                               RcPixel *out)
{
    if (m >= s.M) return false;
    const int inst = b * s.M + m;
    const RcRange r = rc_range(s, inst);
    if (!r.ok || f >= r.fn) return false;
    const int32_t *row = s.faces + ((size_t)r.f0 + f) * 3;
    const int i0 = row[0], i1 = row[1], i2 = row[2];
    if (i0 < 0 || i0 >= r.vn || i1 < 0 || i1 >= r.vn || i2 < 0 || i2 >= r.vn) return false;
    const raster::Vtx *vp = vtx + (size_t)inst * s.Nmax;
    const raster::Vtx v0 = vp[i0], v1 = vp[i1], v2 = vp[i2];
    const raster::Cam c = raster::load_cam(s.K + (s.K_batched ? (size_t)b * 9 : 0));
    double a[3], bb[3], dx, dy, Zd = 0.0;
    const raster::Plane pl = raster::plane(v0, v1, v2, a, bb);
    raster::plane_depth(pl, c, x, y, &dx, &dy, &Zd);
    const double n[3] = {pl.n0, pl.n1, pl.n2};
    const double P[3] = {dx * Zd, dy * Zd, Zd};
    const double q[3] = {P[0] - v0.X, P[1] - v0.Y, P[2] - v0.Z};
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double qb[3] = {q[1] * bb[2] - q[2] * bb[1], q[2] * bb[0] - q[0] * bb[2], q[0] * bb[1] - q[1] * bb[0]};
    const double aq[3] = {a[1] * q[2] - a[2] * q[1], a[2] * q[0] - a[0] * q[2], a[0] * q[1] - a[1] * q[0]};
    const double w1 = ((qb[0] * n[0] + qb[1] * n[1]) + qb[2] * n[2]) / nn;
    const double w2 = ((aq[0] * n[0] + aq[1] * n[1]) + aq[2] * n[2]) / nn;
    const double w0 = (1.0 - w1) - w2;
    const double pp = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2];
    const double diffuse = fabs(pl.num) / sqrt(nn * pp);
    const double t = ambient + diffuse;
    const double light = t > 1.0 ? 1.0 : t;
    const uint8_t *C0 = s.colors + ((size_t)r.v0 + i0) * 3, *C1 = s.colors + ((size_t)r.v0 + i1) * 3, *C2 = s.colors + ((size_t)r.v0 + i2) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double col = (w0 * (double)C0[k] + w1 * (double)C1[k]) + w2 * (double)C2[k];
        out->c[k] = rc_to_u8(light * col);
    }
    out->label = (uint8_t)(m + 1);
    out->z = (float)Zd;
    out->face = f;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_rc_shade(RcScene s, const raster::Vtx *__restrict__ vtx, const unsigned long long *__restrict__ keys,
                                                     const uint8_t *__restrict__ bg, int bg_vec, uint32_t bg_color, double ambient,
                                                     uint8_t *__restrict__ img, uint8_t *__restrict__ label, float *__restrict__ depth,
                                                     int32_t *__restrict__ area, int32_t *__restrict__ face)
{
    __shared__ int s_hist[kBlock];
    const int tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    const size_t HW = (size_t)s.H * s.W, total = HW * s.B;
    const size_t first = (size_t)blockIdx.x * kBlock * 4;                 // < total by the grid
    const size_t b0 = first / HW;
    const size_t g = (size_t)blockIdx.x * kBlock + tid, p0 = 4 * g;
    if (p0 < total) {
        const int cnt = total - p0 >= 4 ? 4 : (int)(total - p0);
        unsigned long long key[4] = {kRcEmpty, kRcEmpty, kRcEmpty, kRcEmpty};
        if (cnt == 4) {                                                  // 32 bytes at a multiple of 32
            const RcVec2k k0 = *reinterpret_cast<const RcVec2k *>(keys + p0), k1 = *reinterpret_cast<const RcVec2k *>(keys + p0 + 2);
            key[0] = k0.v[0], key[1] = k0.v[1], key[2] = k1.v[0], key[3] = k1.v[1];
        } else {
            for (int j = 0; j < cnt; ++j) key[j] = keys[p0 + j];
        }
        uint8_t bgb[12];
        const bool any_empty = key[0] == kRcEmpty || key[1] == kRcEmpty || key[2] == kRcEmpty || key[3] == kRcEmpty;
        if (bg && any_empty) {
            if (bg_vec && cnt == 4) {
                const uint32_t *b4 = reinterpret_cast<const uint32_t *>(bg) + 3 * g;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t q = b4[k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) bgb[4 * k + j] = (uint8_t)(q >> (8 * j));
                }
            } else {
                for (int j = 0; j < 3 * cnt; ++j) bgb[j] = bg[p0 * 3 + j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) bgb[j] = (uint8_t)(bg_color >> (8 * (j % 3)));
        }
        size_t b = p0 / HW;
        const size_t rem = p0 - b * HW;
        int y = (int)(rem / (size_t)s.W), x = (int)(rem - (size_t)y * s.W);
        RcPixel px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            RcPixel o;
            o.c[0] = bgb[3 * j], o.c[1] = bgb[3 * j + 1], o.c[2] = bgb[3 * j + 2];
            o.label = 0, o.z = 0.f, o.face = -1;
            if (j < cnt && key[j] != kRcEmpty) {
                const unsigned tag = (unsigned)key[j];
                RcPixel owned;
                if (rc_shade_owner(s, vtx, (int)b, x, y, (int)(tag >> 24), (int)(tag & 0xffffffu), ambient, &owned)) {
                    o = owned;
                    if (b == b0) atomicAdd(&s_hist[o.label], 1);
                    else atomicAdd(area + b * s.M + (o.label - 1), 1);
                }
            }
            px[j] = o;
            if (++x == s.W) {
                x = 0;
                if (++y == s.H) y = 0, ++b;
            }
        }
        if (cnt == 4) {
            uint32_t w[3] = {0, 0, 0};
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j / 4] |= (uint32_t)px[j / 3].c[j % 3] << (8 * (j % 4));
            uint32_t *o4 = reinterpret_cast<uint32_t *>(img) + 3 * g;
            o4[0] = w[0], o4[1] = w[1], o4[2] = w[2];
            reinterpret_cast<uint32_t *>(label)[g] = (uint32_t)px[0].label | ((uint32_t)px[1].label << 8) | ((uint32_t)px[2].label << 16) |
                                                     ((uint32_t)px[3].label << 24);
            RcVec4f z;
#pragma unroll
            for (int j = 0; j < 4; ++j) z.v[j] = px[j].z;
            reinterpret_cast<RcVec4f *>(depth)[g] = z;
            if (face) {
                RcVec4i fv;
#pragma unroll
                for (int j = 0; j < 4; ++j) fv.v[j] = px[j].face;
                reinterpret_cast<RcVec4i *>(face)[g] = fv;
            }
        } else {                                                         // the last one to three pixels of the batch
            for (int j = 0; j < cnt; ++j) {
                const size_t p = p0 + j;
                img[p * 3] = px[j].c[0], img[p * 3 + 1] = px[j].c[1], img[p * 3 + 2] = px[j].c[2];
                label[p] = px[j].label;
                depth[p] = px[j].z;
                if (face) face[p] = px[j].face;
            }
        }
    }
    __syncthreads();
    if (tid >= 1 && tid <= s.M && s_hist[tid] != 0) atomicAdd(area + b0 * s.M + (tid - 1), s_hist[tid]);
}

struct RcLayout { size_t vtx, keys, total; };

RcLayout rc_layout(int B, int M, int Nmax, int H, int W)
{
    RcLayout L;
    L.vtx = 0;
    L.keys = align_up(sizeof(raster::Vtx) * (size_t)B * M * Nmax);
    L.total = L.keys + align_up(sizeof(unsigned long long) * (size_t)B * H * W);
    return L;
}

int rc_check(int B, int M, int Nmax, int H, int W)
{
    if (B < 1 || M < 1 || M > kRcMaxM || (long long)B * M > 65535) return fail(PVV_E_ARG, "render: B >= 1, M in [1, 255] and B*M <= 65535 are required");
    if (H < 1 || W < 1 || H > kRcMaxSide || W > kRcMaxSide) return fail(PVV_E_ARG, "render: the image's sides must lie in [1, 16384]");
    if (Nmax < 1 || Nmax > INT_MAX / 3) return fail(PVV_E_ARG, "render: the largest vertex count must lie in [1, 2^31 / 3)");
    if (((size_t)B * H * W + 1023) / 1024 > (size_t)INT_MAX) return fail(PVV_E_ARG, "render: B*H*W must stay below 2^41");
    return PVV_OK;
}

}  // namespace

PVV_EXPORT size_t pvv_render_workspace_bytes(int B, int M, int Nmax, int H, int W)
{
    if (rc_check(B, M, Nmax, H, W)) return 0;
    return rc_layout(B, M, Nmax, H, W).total;
}

PVV_EXPORT int pvv_render_color(const float *d_pts, const uint8_t *d_colors, const int32_t *d_faces, int N, int F, const int32_t *d_ranges,
                                int O, int Nmax, int Fmax, const double *d_pose, const int32_t *d_obj, const double *d_K, int K_batched,
                                const uint8_t *d_bg, const uint8_t *h_bg_color, int B, int M, int H, int W, double near, double far,
                                double ambient, void *d_workspace, size_t workspace_bytes, uint8_t *d_img, uint8_t *d_label, float *d_depth,
                                int32_t *d_area, int32_t *d_face, void *stream)
{
    if (int e = rc_check(B, M, Nmax, H, W)) return e;
    if (N < 1 || N > INT_MAX / 3 || F < 0 || F > INT_MAX / 3 || Nmax > N) return fail(PVV_E_ARG, "render: N in [1, 2^31 / 3), F in [0, 2^31 / 3) and Nmax <= N are required");
    if (Fmax < 0 || Fmax > kRcMaxFaces || Fmax > F) return fail(PVV_E_ARG, "render: an object may have at most 2^24 faces (and no more than F)");
    if (O < 1) return fail(PVV_E_ARG, "render: at least one object is required");
    if (!(near > 0.0) || !(far >= near) || !(ambient >= 0.0)) return fail(PVV_E_ARG, "render: 0 < near <= far and ambient >= 0 are required");
    if (!d_pts || !d_colors || (F > 0 && !d_faces) || !d_ranges || !d_pose || !d_K || !h_bg_color || !d_workspace || !d_img || !d_label ||
        !d_depth || !d_area)
        return fail(PVV_E_ARG, "render: NULL pointer");
    if ((uintptr_t)d_workspace % 32 != 0 || (uintptr_t)d_img % 4 != 0 || (uintptr_t)d_label % 4 != 0 || (uintptr_t)d_depth % 16 != 0 ||
        (uintptr_t)d_face % 16 != 0 || (uintptr_t)d_area % 4 != 0 || (uintptr_t)d_pose % 8 != 0 || (uintptr_t)d_K % 8 != 0)
        return fail(PVV_E_ARG, "render: workspace must be 32-byte, depth and face 16-byte, pose and K 8-byte, img, label and area 4-byte aligned");
    const RcLayout L = rc_layout(B, M, Nmax, H, W);
    if (workspace_bytes < L.total) return fail(PVV_E_WORKSPACE, "render: workspace smaller than pvv_render_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    raster::Vtx *vtx = (raster::Vtx *)((uint8_t *)d_workspace + L.vtx);
    unsigned long long *keys = (unsigned long long *)((uint8_t *)d_workspace + L.keys);
    const size_t total = (size_t)B * H * W;
    if (hipMemsetAsync(keys, 0xff, total * sizeof(unsigned long long), st) != hipSuccess) return fail(PVV_E_ARG, "render: hipMemsetAsync failed");
    if (hipMemsetAsync(d_area, 0, sizeof(int32_t) * (size_t)B * M, st) != hipSuccess) return fail(PVV_E_ARG, "render: hipMemsetAsync failed");
    RcScene s;
    s.pts = d_pts, s.colors = d_colors, s.faces = d_faces, s.ranges = d_ranges, s.obj = d_obj, s.pose = d_pose, s.K = d_K;
    s.N = N, s.F = F, s.O = O, s.Nmax = Nmax, s.Fmax = Fmax, s.K_batched = K_batched, s.B = B, s.M = M, s.H = H, s.W = W;
    s.near = near, s.far = far;
    if (Fmax > 0) {
        hipLaunchKernelGGL(k_rc_vertices, dim3((Nmax + kBlock - 1) / kBlock, B * M), dim3(kBlock), 0, st, s, vtx);
        if (int e = check_launch("k_rc_vertices")) return e;
        hipLaunchKernelGGL(k_rc_raster, dim3((Fmax + kBlock - 1) / kBlock, B * M), dim3(kBlock), 0, st, s, (const raster::Vtx *)vtx, keys);
        if (int e = check_launch("k_rc_raster")) return e;
    }
    const uint32_t bgc = (uint32_t)h_bg_color[0] | ((uint32_t)h_bg_color[1] << 8) | ((uint32_t)h_bg_color[2] << 16);
    const int bg_vec = d_bg && (uintptr_t)d_bg % 4 == 0;
    hipLaunchKernelGGL(k_rc_shade, dim3((unsigned)((total + 1023) / 1024)), dim3(kBlock), 0, st, s, (const raster::Vtx *)vtx,
                       (const unsigned long long *)keys, d_bg, bg_vec, bgc, ambient, d_img, d_label, d_depth, d_area, d_face);
    return check_launch("k_rc_shade");
}
