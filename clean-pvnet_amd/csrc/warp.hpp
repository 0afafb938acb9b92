// warp.hpp -- the fixed-point rules of the 8-bit affine warps, stated once: crop.hpp, augment.hpp,
// ct_augment.hpp and tless_augment.hpp all sample, take boxes and place cut-outs with this code.  Part of the translation unit
// pvnet_vote.hip, after vote_common.hpp (the wave reductions): built with -ffp-contract=off, every float and double operation
// below rounds once, in the order written, so that the numpy twin (tests/crop_twin.py: sat_rint, invert_affine, warp_u8,
// uncrop_mask) gives the same bits.
//
// A destination pixel (x, y) goes through the inverse map I to a source position with 10 fractional bits: the row part
// (I[1] * y + I[2]) and the column part I[0] * x are rounded separately and added as integers.  The bilinear rule keeps 5 of
// the bits as weights and rounds the weighted sum once; the nearest rule rounds the position.  A tap outside the source is 0
// and is tested before its address is formed.
//
// Reference behaviour restated:
//   U = lib/utils/data_utils.py:123-156 (get_affine_transform)      T = lib/utils/tless/tless_test_utils.py:49-54 (magnify_box)
//   P = lib/utils/tless/tless_utils.py:86-97 (cut_and_paste)
#pragma once

namespace {

// rint (half to even), saturated to int32; a NaN becomes INT32_MIN
__device__ long long sat_rint(double v)
{
    const double r = rint(v);
    if (!(r > -2147483648.0)) return -2147483648ll;
    if (r >= 2147483647.0) return 2147483647ll;
    return (long long)r;
}

// The inverse of a 2 x 3 affine map in the operation order of OpenCV's invertAffineTransform; a singular map gives zeros.
__device__ void invert_affine(const double *M, double *I)
{
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0. ? 1. / D : 0.;
    const double A11 = M[4] * D, A22 = M[0] * D, m1 = M[1] * (-D), m3 = M[3] * (-D);
    const double b1 = -A11 * M[2] - m1 * M[5], b2 = -m3 * M[2] - A22 * M[5];
    I[0] = A11, I[1] = m1, I[2] = b1, I[3] = m3, I[4] = A22, I[5] = b2;
}

// The bilinear rule's source of destination (x, y): the integer pixel and the two 5-bit weights.
__device__ void warp_linear_coords(const double *I, int x, int y, long long *sx, long long *sy, int *a, int *b)
{
    const long long X0 = sat_rint((I[1] * y + I[2]) * 1024.) + 16, Y0 = sat_rint((I[4] * y + I[5]) * 1024.) + 16;
    const long long X = (X0 + sat_rint(I[0] * x * 1024.)) >> 5, Y = (Y0 + sat_rint(I[3] * x * 1024.)) >> 5;
    *sx = X >> 5, *sy = Y >> 5, *a = (int)(X & 31), *b = (int)(Y & 31);
}

// The nearest rule's source pixel of destination (x, y), in two halves: what row y contributes, and the pixel for column x.
__device__ void warp_nearest_row(const double *I, int y, long long *XR, long long *YR)
{
    *XR = sat_rint((I[1] * y + I[2]) * 1024.) + 512, *YR = sat_rint((I[4] * y + I[5]) * 1024.) + 512;
}
__device__ void warp_nearest_col(const double *I, int x, long long XR, long long YR, long long *X, long long *Y)
{
    *X = (XR + sat_rint(I[0] * x * 1024.)) >> 10, *Y = (YR + sat_rint(I[3] * x * 1024.)) >> 10;
}

// The bilinear sample of src [h,w,C] uint8 for destination (x, y): put(c, value) takes channel c as soon as it is formed.
template <int C, typename Put>
__device__ void sample_linear_to(const uint8_t *__restrict__ src, int h, int w, const double *I, int x, int y, Put put)
{
    long long sx, sy;
    int a, b;
    warp_linear_coords(I, x, y, &sx, &sy, &a, &b);
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
    const bool in_x0 = sx >= 0 && sx < w, in_x1 = sx + 1 >= 0 && sx + 1 < w, in_y0 = sy >= 0 && sy < h, in_y1 = sy + 1 >= 0 && sy + 1 < h;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int p00 = in_y0 && in_x0 ? src[((size_t)sy * w + sx) * C + c] : 0;
        const int p01 = in_y0 && in_x1 ? src[((size_t)sy * w + sx + 1) * C + c] : 0;
        const int p10 = in_y1 && in_x0 ? src[((size_t)(sy + 1) * w + sx) * C + c] : 0;
        const int p11 = in_y1 && in_x1 ? src[((size_t)(sy + 1) * w + sx + 1) * C + c] : 0;
        put(c, (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 16384) >> 15);
    }
}

// out[0, C) = that sample
template <int C>
__device__ void sample_linear(const uint8_t *__restrict__ src, int h, int w, const double *I, int x, int y, int *out)
{
    sample_linear_to<C>(src, h, w, I, x, y, [&](int c, int v) { out[c] = v; });
}

// out[0, C) = the nearest sample of src [h,w,C] uint8 for destination (x, y)
template <int C>
__device__ void sample_nearest(const uint8_t *__restrict__ src, int h, int w, const double *I, int x, int y, int *out)
{
    long long XR, YR, X, Y;
    warp_nearest_row(I, y, &XR, &YR);
    warp_nearest_col(I, x, XR, YR, &X, &Y);
    const bool in = X >= 0 && X < w && Y >= 0 && Y < h;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = in ? src[((size_t)Y * w + (size_t)X) * C + c] : 0;
}

// ------------------------------------------------------------------------------------------------- boxes and placements
constexpr int kExtentBig = 1 << 30;

// The box of the pixels that were noted, as maxima so that zeroed memory is the empty box and one integer atomic per
// side merges a row: (kExtentBig - xmin, xmax + 1, kExtentBig - ymin, ymax + 1).
struct Extent {
    int32_t v[4];

    // One pixel, into a lane's own box.
    __device__ void add(int x, int y) { v[0] = max(v[0], kExtentBig - x), v[1] = max(v[1], x + 1), v[2] = max(v[2], kExtentBig - y), v[3] = max(v[3], y + 1); }

    // A wave's row of pixels, lane threadIdx.x at (x, y) (blocks of 64 x n lanes: y is the same for the wave's lanes), into a
    // box in memory.  Every lane of the wave calls it.
    __device__ void note(bool hit, int x, int y)
    {
        const int nx = wave_max(hit ? kExtentBig - x : 0), x1 = wave_max(hit ? x + 1 : 0);
        if (threadIdx.x == 0 && x1) {
            atomicMax(&v[0], nx);
            atomicMax(&v[1], x1);
            atomicMax(&v[2], kExtentBig - y);
            atomicMax(&v[3], y + 1);
        }
    }

    __device__ bool empty() const { return v[1] == 0; }

    // (xmin, ymin, xmax, ymax), inclusive, of a box that is not empty
    __device__ void decode(int *b) const { b[0] = kExtentBig - v[0], b[1] = kExtentBig - v[2], b[2] = v[1] - 1, b[3] = v[3] - 1; }
};
static_assert(sizeof(Extent) == 16, "four int32 in AugState, TlaStat and the workspaces");

// lo + floor(u * (hi - lo)) for hi > lo, lo otherwise (where np.random.randint raises)
__device__ int uniform_randint(int lo, int hi, double u)
{
    if (hi <= lo) return lo;
    const long long k = (long long)floor(u * (double)(hi - lo));
    return lo + (int)min(k, (long long)(hi - lo) - 1);
}

// Where a cut-out goes (P:87-93): the box of its mask and the drawn corner on the H x W canvas, as
// (y_min, x_min, h, w, dst_y, dst_x); (0, 0, -1, -1, 0, 0) without a pixel.
__device__ void place_record(const Extent &e, int H, int W, double uy, double ux, int32_t *out)
{
    if (e.empty()) {
        out[0] = 0, out[1] = 0, out[2] = -1, out[3] = -1, out[4] = 0, out[5] = 0;
        return;
    }
    int b[4];
    e.decode(b);
    const int bh = b[3] - b[1], bw = b[2] - b[0];
    out[0] = b[1], out[1] = b[0], out[2] = bh, out[3] = bw;
    out[4] = uniform_randint(0, H - bh, uy), out[5] = uniform_randint(0, W - bw, ux);
}

// Does the cut-out placed by record p cover canvas pixel (X, Y) (P:94-97 as a gather)?  mask is its h x w plane; the answer is
// the pixel's byte of the plane, NULL for no.
__device__ const uint8_t *place_covers(const int32_t *__restrict__ p, const uint8_t *__restrict__ mask, int h, int w, int X, int Y)
{
    if (p[2] < 0) return nullptr;
    const long long y = (long long)Y - p[4] + p[0], x = (long long)X - p[5] + p[1];
    if (y < p[0] || y > (long long)p[0] + p[2] || x < p[1] || x > (long long)p[1] + p[3]) return nullptr;
    if (y < 0 || y >= h || x < 0 || x >= w) return nullptr;                  // (the box lies inside the plane)
    const uint8_t *m = mask + ((size_t)y * w + (size_t)x);
    return *m != 0 ? m : nullptr;
}

// ------------------------------------------------------------------------------------------------------- the crop's map
// The closed form of get_affine_transform(center, scale, 0, [ow, oh]) (U:123-156) in binary64.
__device__ void crop_transform(double cx, double cy, double scale, int ow, int oh, double *M)
{
    const double a = (double)ow / scale;
    M[0] = a, M[1] = 0., M[2] = ow * 0.5 - a * cx, M[3] = 0., M[4] = a, M[5] = oh * 0.5 - a * cy;
}

// The rectangle of magnify_box (T:49-54) for the box (x0, y0, x1, y1) under the map of crop_transform: (rx0, ry0, rx1, ry1),
// inclusive, clamped to the crop.
__device__ void magnify_rect(const double *M, double x0, double y0, double x1, double y1, double ratio, int ow, int oh, int32_t *r)
{
    const double a = M[0], px0 = x0 * a + M[2], py0 = y0 * a + M[5], px1 = x1 * a + M[2], py1 = y1 * a + M[5];
    const double mx = (px0 + px1) / 2., my = (py0 + py1) / 2.;
    const long long c[4] = {sat_rint((px0 - mx) * ratio + mx), sat_rint((py0 - my) * ratio + my),
                            sat_rint((px1 - mx) * ratio + mx), sat_rint((py1 - my) * ratio + my)};
    r[0] = (int)min(max(c[0], 0ll), (long long)ow - 1), r[1] = (int)min(max(c[1], 0ll), (long long)oh - 1);
    r[2] = (int)min(max(c[2], 0ll), (long long)ow - 1), r[3] = (int)min(max(c[3], 0ll), (long long)oh - 1);
}

}  // namespace
