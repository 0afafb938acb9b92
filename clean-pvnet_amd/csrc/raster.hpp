// raster.hpp -- the coverage rules of the device rasterisers, stated once: the depth renderer (pvnet_vsd.hip) and the colour
// renderer (render.hpp) both draw with this code and differ only in the sink a covered sample goes to.  Included inside the
// anonymous namespace of the translation unit, after its own `#pragma clang fp contract(off)`: every double operation below
// rounds once, in the order written, so that the numpy twin (tests/vsd_twin.py) gives the same bytes.
//
// A vertex is taken to eye space in binary64 and, when it lies inside the near plane, projected and snapped to 8 sub-pixel
// bits.  A face is cut at the near plane into one or two pieces, each oriented to positive area with its bounding box clamped
// to the image.  The sample of pixel (x, y) is its centre, (256x + 128, 256y + 128) in snapped units; it is covered when all
// three edge functions are positive, or zero on an edge that owns its line.  Its depth is that of the face's plane -- of the
// unclipped face, so the pieces of one face agree.
#pragma once

#include <climits>

namespace raster {

constexpr int kSmall = 32;           // a piece with at most this many samples in its bounding box is swept by its own lane
constexpr int kBadCoord = INT_MIN;   // snapped coordinate of a vertex that has none (outside the near plane, or too large)
constexpr double kSnapLimit = 268435456.0;   // 2^28

struct Vtx {                         // 32 bytes, one per (pose, vertex)
    double X, Y, Z;
    int U, V;
};

struct Cam {
    double fx, s, cx, fy, cy;
};

struct Piece {                       // a clipped, oriented (positive area) triangle in snapped coordinates, with its samples
    int ax, ay, bx, by, cx, cy;
    int xmin, ymin, w, h;            // w == 0: no piece
};

struct Plane {
    double n0, n1, n2, num;
};

struct Face {                        // what a face draws: its plane and its pieces (pc1 only when one vertex is outside)
    Plane pl;
    Piece pc0, pc1;
};

__device__ Cam load_cam(const double *K)
{
    Cam c;
    c.fx = K[0];
    c.s = K[1];
    c.cx = K[2];
    c.fy = K[4];
    c.cy = K[5];
    return c;
}

// u = (fx*X + s*Y)/Z + cx, v = (fy*Y)/Z + cy, snapped to 8 sub-pixel bits; kBadCoord when out of range or not a number
__device__ void project_snap(const Cam &c, double X, double Y, double Z, int *U, int *V)
{
    const double u = (c.fx * X + c.s * Y) / Z + c.cx;
    const double v = (c.fy * Y) / Z + c.cy;
    const double Ud = floor(256.0 * u + 0.5), Vd = floor(256.0 * v + 0.5);
    const bool ok = fabs(Ud) <= kSnapLimit && fabs(Vd) <= kSnapLimit;      // false for NaN
    *U = ok ? (int)Ud : kBadCoord;
    *V = ok ? (int)Vd : kBadCoord;
}

// The point (x, y, z) under the row-major 3x4 pose T: X = ((T0*x + T1*y) + T2*z) + T3 and so on, snapped when Z >= near.
__device__ Vtx vertex(const double *T, const Cam &c, double x, double y, double z, double near)
{
    Vtx o;
    o.X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    o.Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    o.Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    o.U = o.V = kBadCoord;
    if (o.Z >= near) project_snap(c, o.X, o.Y, o.Z, &o.U, &o.V);
    return o;
}

// The vertex where the edge from the inside vertex p to the outside vertex q meets Z = near, projected and snapped.
__device__ void clip_snap(const Cam &c, const Vtx &p, const Vtx &q, double near, int *U, int *V)
{
    const double t = (near - p.Z) / (q.Z - p.Z);
    const double X = p.X + t * (q.X - p.X);
    const double Y = p.Y + t * (q.Y - p.Y);
    project_snap(c, X, Y, near, U, V);
}

__device__ Piece make_piece(int U0, int V0, int U1, int V1, int U2, int V2, int W, int H)
{
    Piece t;
    t.w = t.h = 0;
    t.ax = t.ay = t.bx = t.by = t.cx = t.cy = t.xmin = t.ymin = 0;
    if (U0 == kBadCoord || U1 == kBadCoord || U2 == kBadCoord) return t;
    const long long area2 = (long long)(U1 - U0) * (V2 - V0) - (long long)(V1 - V0) * (U2 - U0);
    if (area2 == 0) return t;
    if (area2 < 0) {
        int k = U1; U1 = U2; U2 = k;
        k = V1; V1 = V2; V2 = k;
    }
    // samples (256x + 128, 256y + 128) inside the vertices' box: x >= (Umin - 128)/256, x <= (Umax - 128)/256
    int xmin = (min(U0, min(U1, U2)) - 128 + 255) >> 8, xmax = (max(U0, max(U1, U2)) - 128) >> 8;
    int ymin = (min(V0, min(V1, V2)) - 128 + 255) >> 8, ymax = (max(V0, max(V1, V2)) - 128) >> 8;
    xmin = max(xmin, 0);
    ymin = max(ymin, 0);
    xmax = min(xmax, W - 1);
    ymax = min(ymax, H - 1);
    if (xmin > xmax || ymin > ymax) return t;
    t.ax = U0; t.ay = V0; t.bx = U1; t.by = V1; t.cx = U2; t.cy = V2;
    t.xmin = xmin; t.ymin = ymin; t.w = xmax - xmin + 1; t.h = ymax - ymin + 1;
    return t;
}

// E = dx*(py - ay) - dy*(px - ax) > 0, or = 0 on an edge that owns its line.  |dx|, |dy| <= 2^29 and |py - ay|, |px - ax| <
// 2^29: every product fits 59 bits.
__device__ bool edge_in(int ax, int ay, int bx, int by, int px, int py)
{
    const int dx = bx - ax, dy = by - ay;
    const long long E = (long long)dx * (py - ay) - (long long)dy * (px - ax);
    const bool owns = dy > 0 || (dy == 0 && dx > 0);
    return E > 0 || (E == 0 && owns);
}

__device__ bool covered(const Piece &t, int x, int y)
{
    const int px = 256 * x + 128, py = 256 * y + 128;
    return edge_in(t.ax, t.ay, t.bx, t.by, px, py) && edge_in(t.bx, t.by, t.cx, t.cy, px, py) &&
           edge_in(t.cx, t.cy, t.ax, t.ay, px, py);
}

// The largest value an edge function takes on the samples x0..x1, y0..y1 is negative: no sample of the block is inside.
__device__ bool edge_rejects(int ax, int ay, int bx, int by, int x0, int y0, int x1, int y1)
{
    const int dx = bx - ax, dy = by - ay;
    const int py = 256 * (dx > 0 ? y1 : y0) + 128, px = 256 * (dy > 0 ? x0 : x1) + 128;
    return (long long)dx * (py - ay) - (long long)dy * (px - ax) < 0;
}

__device__ bool block_rejected(const Piece &t, int x0, int y0, int x1, int y1)
{
    return edge_rejects(t.ax, t.ay, t.bx, t.by, x0, y0, x1, y1) || edge_rejects(t.bx, t.by, t.cx, t.cy, x0, y0, x1, y1) ||
           edge_rejects(t.cx, t.cy, t.ax, t.ay, x0, y0, x1, y1);
}

// n = a x b with a = v1 - v0, b = v2 - v0, num = (n0*v0.X + n1*v0.Y) + n2*v0.Z; a and b go to the caller that shades.
__device__ Plane plane(const Vtx &v0, const Vtx &v1, const Vtx &v2, double *a, double *b)
{
    a[0] = v1.X - v0.X, a[1] = v1.Y - v0.Y, a[2] = v1.Z - v0.Z;
    b[0] = v2.X - v0.X, b[1] = v2.Y - v0.Y, b[2] = v2.Z - v0.Z;
    Plane pl;
    pl.n0 = a[1] * b[2] - a[2] * b[1];
    pl.n1 = a[2] * b[0] - a[0] * b[2];
    pl.n2 = a[0] * b[1] - a[1] * b[0];
    pl.num = (pl.n0 * v0.X + pl.n1 * v0.Y) + pl.n2 * v0.Z;
    return pl;
}

// dy = ((y+0.5) - cy)/fy, dx = (((x+0.5) - cx) - s*dy)/fx, den = (n0*dx + n1*dy) + n2, Z = num/den; false when den == 0
__device__ bool plane_depth(const Plane &pl, const Cam &c, int x, int y, double *dx_, double *dy_, double *Z)
{
    const double dy = (((double)y + 0.5) - c.cy) / c.fy;
    const double dx = ((((double)x + 0.5) - c.cx) - c.s * dy) / c.fx;
    const double den = (pl.n0 * dx + pl.n1 * dy) + pl.n2;
    *dx_ = dx, *dy_ = dy;
    if (den == 0.0) return false;
    *Z = pl.num / den;
    return true;
}

__device__ void rotate_left(Vtx &a, Vtx &b, Vtx &c, int r)
{
    if (r == 1) {
        const Vtx k = a; a = b; b = c; c = k;
    } else if (r == 2) {
        const Vtx k = c; c = b; b = a; a = k;
    }
}

// The near clip of one face.  No vertex inside: nothing.  All inside: the face.  One inside, a: (a, ab, ac).  One outside, c:
// (a, b, bc) and (a, bc, ac).  ab is where the edge from a to b meets the near plane.  The plane and the pieces are locals
// gathered at the return: assigned as members of one Face in the branches they end up in scratch memory (88 bytes a lane).
// Forced inline, so that the optimiser meets this code inside the raster kernel as it did when it stood there: left to the
// inliner's own order the depth render of two poses measured 2 % slower (same registers, another schedule).
__device__ __forceinline__ Face clip_face(const Cam &c, const Vtx &f0, const Vtx &f1, const Vtx &f2, double near, int W, int H)
{
    Vtx v0 = f0, v1 = f1, v2 = f2;
    Piece pc0 = make_piece(kBadCoord, 0, 0, 0, 0, 0, W, H), pc1 = pc0;      // no piece
    Plane pl = {0.0, 0.0, 0.0, 0.0};
    const int m = (v0.Z >= near ? 1 : 0) | (v1.Z >= near ? 2 : 0) | (v2.Z >= near ? 4 : 0);
    if (!m) return {pl, pc0, pc1};
    double a[3], b[3];
    pl = plane(v0, v1, v2, a, b);
    if (m == 7) {
        pc0 = make_piece(v0.U, v0.V, v1.U, v1.V, v2.U, v2.V, W, H);
    } else if (m == 1 || m == 2 || m == 4) {
        rotate_left(v0, v1, v2, m == 1 ? 0 : m == 2 ? 1 : 2);
        int Ub, Vb, Uc, Vc;
        clip_snap(c, v0, v1, near, &Ub, &Vb);
        clip_snap(c, v0, v2, near, &Uc, &Vc);
        pc0 = make_piece(v0.U, v0.V, Ub, Vb, Uc, Vc, W, H);
    } else {
        rotate_left(v0, v1, v2, m == 3 ? 0 : m == 6 ? 1 : 2);
        int Ub, Vb, Ua, Va;
        clip_snap(c, v1, v2, near, &Ub, &Vb);
        clip_snap(c, v0, v2, near, &Ua, &Va);
        pc0 = make_piece(v0.U, v0.V, v1.U, v1.V, Ub, Vb, W, H);
        pc1 = make_piece(v0.U, v0.V, Ub, Vb, Ua, Va, W, H);
    }
    return {pl, pc0, pc1};
}

__device__ int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ double rl(double v, int lane)
{
    return __hiloint2double(rl(__double2hiint(v), lane), rl(__double2loint(v), lane));
}

__device__ Piece rl(const Piece &t, int lane)
{
    Piece o;
    o.ax = rl(t.ax, lane); o.ay = rl(t.ay, lane); o.bx = rl(t.bx, lane); o.by = rl(t.by, lane);
    o.cx = rl(t.cx, lane); o.cy = rl(t.cy, lane);
    o.xmin = rl(t.xmin, lane); o.ymin = rl(t.ymin, lane); o.w = rl(t.w, lane); o.h = rl(t.h, lane);
    return o;
}

// One piece per lane (w == 0: none), called by whole waves.  Small pieces by their own lane, the others by the whole wave: 64
// blocks of 8x8 samples are tested against the three edges at a time (one block per lane), the blocks that survive are sampled
// one sample per lane.  sink(x, y, plane, cam) takes a covered sample; sink.of(lane) is the sink of the lane whose piece the
// wave is sweeping.
template <class Sink>
__device__ void sweep(const Piece &mine, const Plane &pl, const Sink &sink, const Cam &c)
{
    const int lane = threadIdx.x & 63;
    const int cnt = mine.w * mine.h;                       // <= 2^28: no side of an image exceeds 2^14
    const bool small = cnt <= kSmall;
    if (small) {
        int x = mine.xmin, y = mine.ymin;
        for (int i = 0; i < cnt; ++i) {
            if (covered(mine, x, y)) sink(x, y, pl, c);
            if (++x == mine.xmin + mine.w) {
                x = mine.xmin;
                ++y;
            }
        }
    }
    unsigned long long big = __ballot(!small);
    while (big) {
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        const Piece t = rl(mine, src);
        Plane q;
        q.n0 = rl(pl.n0, src); q.n1 = rl(pl.n1, src); q.n2 = rl(pl.n2, src); q.num = rl(pl.num, src);
        const Sink to = sink.of(src);
        const int xmax = t.xmin + t.w - 1, ymax = t.ymin + t.h - 1;
        const int bx0 = t.xmin >> 3, by0 = t.ymin >> 3;
        const int nbx = (xmax >> 3) - bx0 + 1, nby = (ymax >> 3) - by0 + 1;
        const int nblocks = nbx * nby;
        for (int base = 0; base < nblocks; base += 64) {
            const int bi = base + lane;
            const int by = bi / nbx, bx = bi - by * nbx;
            bool live = bi < nblocks;
            if (live) {
                const int x0 = max((bx0 + bx) << 3, t.xmin), y0 = max((by0 + by) << 3, t.ymin);
                const int x1 = min(((bx0 + bx) << 3) + 7, xmax), y1 = min(((by0 + by) << 3) + 7, ymax);
                live = !block_rejected(t, x0, y0, x1, y1);
            }
            unsigned long long todo = __ballot(live);
            while (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int x = ((bx0 + rl(bx, j)) << 3) + (lane & 7), y = ((by0 + rl(by, j)) << 3) + (lane >> 3);
                if (x >= t.xmin && x <= xmax && y >= t.ymin && y <= ymax && covered(t, x, y)) to(x, y, q, c);
            }
        }
    }
}

}  // namespace raster
