// pvnet_pose.hip -- pose of a whole batch on the device, start included (include/pvnet_pose.h), native HIP for gfx950.
// One wavefront per image (4 images per block), binary64.  Lane i owns keypoint i (loops for pn > 64); sums are reduced
// across the wave by a butterfly (every lane ends with the same bits), the 12 x 12 eigenproblem of the DLT lives in the
// wave's LDS rows, and everything else -- the P3P quartic, the 3 x 3 decompositions, the angle-axis -- is computed by every
// lane on the same uniform values.  The refinement is pnp_lm.hpp, the code pvnet_pnp.hip runs.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "pnp_lm.hpp"
#include "pvnet_pose.h"

#define PVP_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

using namespace pnp_lm;

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0; }

// (key, index) order of the selections: a larger key first; on equal keys the higher index (tie_high, numpy's ascending
// argsort read from the end) or the lower one (a stable descending argsort).
__device__ __forceinline__ bool before(double k, int i, double bk, int bi, bool tie_high)
{
    return k > bk || (k == bk && (tie_high ? i > bi : i < bi));
}

// The best keypoint not among sel[0..ns) by key(i), over the whole wave.  Keys are never NaN.
template <class Key>
__device__ int wave_pick(const Key &key, int pn, const int sel[6], int ns, bool tie_high, int lane)
{
    double bk = -INFINITY;
    int bi = tie_high ? -1 : INT_MAX;
    for (int i = lane; i < pn; i += 64) {
        bool taken = false;
        for (int s = 0; s < 6; ++s) taken |= s < ns && sel[s] == i;
        const double k = key(i);
        if (!taken && before(k, i, bk, bi, tie_high)) { bk = k; bi = i; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double ok = __shfl_xor(bk, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (before(ok, oi, bk, bi, tie_high)) { bk = ok; bi = oi; }
    }
    return bi;
}

// Symmetric 3 x 3 eigen-decomposition by cyclic Jacobi (Numerical Recipes' rotation): the eigenvalues end on A's
// diagonal, the eigenvectors in V's columns.
__device__ void eig3(double A[3][3], double V[3][3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                const double theta = 0.5 * (A[q][q] - A[p][p]) / apq;
                double t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if (r != p && r != q) {
                        const double gp = A[r][p], hq = A[r][q];
                        A[r][p] = A[p][r] = gp - s * (hq + gp * tau);
                        A[r][q] = A[q][r] = hq + s * (gp - hq * tau);
                    }
                    const double vp = V[r][p], vq = V[r][q];
                    V[r][p] = vp - s * (vq + vp * tau);
                    V[r][q] = vq + s * (vp - vq * tau);
                }
            }
    }
}

__device__ __forceinline__ void cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double det3(const double M[3][3])
{
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// un_pnp_utils.rotation_to_angle_axis, branch for branch
__device__ void angle_axis(const double R[3][3], double w[3])
{
    const double c = (R[0][0] + R[1][1] + R[2][2] - 1.0) / 2.0;
    const double v[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / 2.0;
    const double th = atan2(s, c);                            // well conditioned at 0 and at pi, where acos(c) is not
    if (th < 1e-9) {
        for (int k = 0; k < 3; ++k) w[k] = v[k] / 2.0;
    } else if (c > -0.5) {                                    // the axis from the antisymmetric part, |v| = 2 sin th
        const double f = th / (2.0 * s);
        for (int k = 0; k < 3; ++k) w[k] = v[k] * f;
    } else {                                                  // towards pi v vanishes: (R + R^T) / 2 - c I = (1 - c) a a^T
        double S[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) S[r][k] = (R[r][k] + R[k][r]) / 2.0 - (r == k ? c : 0.0);
        const int m = S[1][1] > S[0][0] ? (S[2][2] > S[1][1] ? 2 : 1) : (S[2][2] > S[0][0] ? 2 : 0);   // np.argmax: the first maximum
        double a[3] = {S[m][0], S[m][1], S[m][2]};
        if (v[0] * a[0] + v[1] * a[1] + v[2] * a[2] < 0.0)
            for (int k = 0; k < 3; ++k) a[k] = -a[k];
        const double f = th / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 3; ++k) w[k] = a[k] * f;
    }
}

// un_pnp_utils.rodrigues
__device__ void rodrigues(const double w[3], double R[3][3])
{
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double Kx[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    const double a = th < 1e-12 ? 1.0 : sin(th) / th, b = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double k2 = 0.0;
            for (int k = 0; k < 3; ++k) k2 += Kx[r][k] * Kx[k][c];
            R[r][c] = (r == c ? 1.0 : 0.0) + a * Kx[r][c] + b * k2;
        }
}

struct Cplx { double re, im; };
__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cplx csub(Cplx a, Cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ Cplx cdiv(Cplx a, Cplx b)
{
    const double s = fabs(b.re) + fabs(b.im), br = b.re / s, bi = b.im / s, ar = a.re / s, ai = a.im / s;
    const double d = br * br + bi * bi;
    return {(ar * br + ai * bi) / d, (ai * br - ar * bi) / d};
}

// All roots of coef[0] z^4 + ... + coef[4] (np.roots: leading zero coefficients dropped, trailing ones give the root 0,
// which the caller rejects anyway) by Durand-Kerner.  Returns the number of roots written to z.
__device__ int quartic_roots(const double coef[5], Cplx z[4])
{
    int lead = 0, n = 4;
    while (lead < 4 && coef[lead] == 0.0) ++lead;
    while (n > lead && coef[n] == 0.0) --n;                   // a trailing zero: the root 0
    const int deg = n - lead;
    if (deg <= 0) return 0;
    double a[5];                                              // monic, a[0] = 1
    for (int k = 0; k <= 4; ++k) a[k] = k <= deg ? coef[lead + k] / coef[lead] : 0.0;
    double bound = 0.0;
    for (int k = 1; k <= deg; ++k) bound = fmax(bound, fabs(a[k]));
    bound += 1.0;                                             // Cauchy: every root lies within it
    Cplx w = {0.4, 0.9}, pw = {bound, 0.0};
    for (int k = 0; k < 4; ++k) { z[k] = pw; pw = cmul(pw, w); }
    double prev = INFINITY;
    for (int iter = 0; iter < 500; ++iter) {
        double moved = 0.0, size = 0.0;
        for (int k = 0; k < 4; ++k) {
            if (k >= deg) break;
            Cplx p = {1.0, 0.0}, den = {1.0, 0.0};
            for (int j = 1; j <= 4; ++j)
                if (j <= deg) p = {p.re * z[k].re - p.im * z[k].im + a[j], p.re * z[k].im + p.im * z[k].re};
            for (int j = 0; j < 4; ++j)
                if (j < deg && j != k) den = cmul(den, csub(z[k], z[j]));
            if (den.re == 0.0 && den.im == 0.0) continue;
            const Cplx d = cdiv(p, den);
            z[k] = csub(z[k], d);
            moved = fmax(moved, fabs(d.re) + fabs(d.im));
            size = fmax(size, fabs(z[k].re) + fabs(z[k].im));
        }
        if (moved <= 1e-14 * fmax(size, 1.0)) break;          // quadratic convergence: this step reached rounding
        if (iter >= 30 && moved >= prev) break;               // no longer shrinking: at the rounding floor of a close pair
        prev = moved;
    }
    return deg;
}

// un_pnp_utils.p3p_depths (Grunert; Haralick et al. 1994, eqs. 9-11): unit bearings f, object points P -> up to four depth
// triples.  A collinear object triple (the rotation about its line is undetermined) has none.
__device__ int p3p_depths(const double f[3][3], const double P[3][3], double sols[4][3])
{
    double d12[3], d02[3], d01[3];
    for (int k = 0; k < 3; ++k) { d12[k] = P[1][k] - P[2][k]; d02[k] = P[0][k] - P[2][k]; d01[k] = P[0][k] - P[1][k]; }
    const double a2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double b2 = d02[0] * d02[0] + d02[1] * d02[1] + d02[2] * d02[2];
    const double c2 = d01[0] * d01[0] + d01[1] * d01[1] + d01[2] * d01[2];
    if (fmin(a2, fmin(b2, c2)) <= 0.0) return 0;
    double cr[3];
    cross(d01, d02, cr);
    if (cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2] <= 1e-12 * c2 * b2) return 0;
    const double ca = f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2];
    const double cb = f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2];
    const double cg = f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2];
    const double q = (a2 - c2) / b2, r = (a2 + c2) / b2;
    const double coef[5] = {
        (q - 1) * (q - 1) - 4 * c2 / b2 * ca * ca,
        4 * (q * (1 - q) * cb - (1 - r) * ca * cg + 2 * c2 / b2 * ca * ca * cb),
        2 * (q * q - 1 + 2 * q * q * cb * cb + 2 * ((b2 - c2) / b2) * ca * ca - 4 * r * ca * cb * cg + 2 * ((b2 - a2) / b2) * cg * cg),
        4 * (-q * (1 + q) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - r) * ca * cg),
        (1 + q) * (1 + q) - 4 * a2 / b2 * cg * cg};
    for (int k = 0; k < 5; ++k)
        if (!isfinite(coef[k])) return 0;
    Cplx z[4];
    const int nr = quartic_roots(coef, z);
    int ns = 0;
    for (int k = 0; k < 4; ++k) {
        if (k >= nr) break;
        const double mod = sqrt(z[k].re * z[k].re + z[k].im * z[k].im);
        if (fabs(z[k].im) > 1e-6 * fmax(1.0, mod) || z[k].re <= 0.0) continue;
        const double v = z[k].re, den = 2 * (cg - v * ca);
        if (fabs(den) < 1e-14) continue;
        const double u = ((q - 1) * v * v - 2 * q * cb * v + 1 + q) / den;
        const double d = 1 + u * u - 2 * u * cg;
        if (u <= 0.0 || d <= 0.0) continue;
        const double s1 = sqrt(c2 / d);
        sols[ns][0] = s1; sols[ns][1] = u * s1; sols[ns][2] = v * s1;
        ++ns;
    }
    return ns;
}

struct Args {
    const double *pts2d, *pts3d, *wgt2d, *K;
    int method, B, pn, pts3d_batched, K_batched, max_iter;
    double ftol;
    double *rt, *Rt, *init_rt, *info;
    int *status;
};

__device__ __forceinline__ double p3p_key(const double *wg, int i)   // un_pnp_utils.py:26, non-finite -> -inf
{
    const double k = wg[i * 3] + wg[i * 3 + 1];
    return isfinite(k) ? k : -INFINITY;
}

// initial_pose_p3p: true and rt when a solution exists
__device__ bool start_p3p(const double *p2, const double *p3, const double *wg, const double Kc[3][3], const double Ki[3][3],
                          int pn, int lane, double rt[6])
{
    int sel[6] = {0, 0, 0, 0, 0, 0};                         // sel[0] the best key ... sel[3] the fourth best
    auto key = [&](int i) { return p3p_key(wg, i); };
    for (int s = 0; s < 4; ++s) sel[s] = wave_pick(key, pn, sel, s, true, lane);
    const int idx[4] = {sel[3], sel[2], sel[1], sel[0]};      // argsort(key)[-4:]
    double P4[4][3], p4[4][2], f[3][3];
    for (int j = 0; j < 4; ++j) {
        for (int k = 0; k < 3; ++k) P4[j][k] = p3[idx[j] * 3 + k];
        p4[j][0] = p2[idx[j] * 2]; p4[j][1] = p2[idx[j] * 2 + 1];
        if (j < 3) {
            double n[3], nn = 0.0;
            for (int r = 0; r < 3; ++r) { n[r] = Ki[r][0] * p4[j][0] + Ki[r][1] * p4[j][1] + Ki[r][2]; nn += n[r] * n[r]; }
            nn = sqrt(nn);
            for (int r = 0; r < 3; ++r) f[j][r] = n[r] / nn;
        }
    }
    double sols[4][3];
    const double P3[3][3] = {{P4[0][0], P4[0][1], P4[0][2]}, {P4[1][0], P4[1][1], P4[1][2]}, {P4[2][0], P4[2][1], P4[2][2]}};
    const int ns = p3p_depths(f, P3, sols);
    double best = INFINITY, bR[3][3], bt[3];
    bool found = false;
    for (int si = 0; si < 4; ++si) {
        if (si >= ns) break;
        double X[3][3], cP[3] = {0, 0, 0}, cX[3] = {0, 0, 0};
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) { X[j][k] = f[j][k] * sols[si][j]; cP[k] += P3[j][k] / 3.0; cX[k] += X[j][k] / 3.0; }
        // absolute orientation: H = sum (P - cP)(X - cX)^T = sum sigma_k u_k v_k^T, R = sum v_k u_k^T with the determinant
        // correction -- H has rank 2, so the third pair is v1 x v2, u1 x u2 (not an eigenvector of the null space)
        double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int j = 0; j < 3; ++j)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) H[r][c] += (P3[j][r] - cP[r]) * (X[j][c] - cX[c]);
        double G[3][3], V[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) G[r][c] = H[0][r] * H[0][c] + H[1][r] * H[1][c] + H[2][r] * H[2][c];
        eig3(G, V);
        int o0 = 0, o1 = 1, o2 = 2;                           // eigenvalues descending
        if (G[o1][o1] > G[o0][o0]) { int t = o0; o0 = o1; o1 = t; }
        if (G[o2][o2] > G[o0][o0]) { int t = o0; o0 = o2; o2 = t; }
        if (G[o2][o2] > G[o1][o1]) { int t = o1; o1 = o2; o2 = t; }
        double v[3][3], u[3][3];
        for (int k = 0; k < 3; ++k) { v[0][k] = V[k][o0]; v[1][k] = V[k][o1]; }
        bool ok = true;
        for (int m = 0; m < 2; ++m) {
            const double sg = sqrt(fmax(G[m == 0 ? o0 : o1][m == 0 ? o0 : o1], 0.0));
            if (!(sg > 0.0)) ok = false;
            for (int r = 0; r < 3; ++r) u[m][r] = (H[r][0] * v[m][0] + H[r][1] * v[m][1] + H[r][2] * v[m][2]) / sg;
        }
        if (!ok) continue;
        cross(v[0], v[1], v[2]);
        cross(u[0], u[1], u[2]);
        double R[3][3], t[3], x4[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r][c] = v[0][r] * u[0][c] + v[1][r] * u[1][c] + v[2][r] * u[2][c];
        for (int r = 0; r < 3; ++r) t[r] = cX[r] - (R[r][0] * cP[0] + R[r][1] * cP[1] + R[r][2] * cP[2]);
        for (int r = 0; r < 3; ++r) x4[r] = R[r][0] * P4[3][0] + R[r][1] * P4[3][1] + R[r][2] * P4[3][2] + t[r];
        if (!(x4[2] > 0.0)) continue;
        const double h[3] = {x4[0] / x4[2], x4[1] / x4[2], 1.0};
        const double ex = Kc[0][0] * h[0] + Kc[0][1] * h[1] + Kc[0][2] * h[2] - p4[3][0];
        const double ey = Kc[1][0] * h[0] + Kc[1][1] * h[1] + Kc[1][2] * h[2] - p4[3][1];
        const double err = ex * ex + ey * ey;
        if (!found || err < best) {
            found = true; best = err;
            for (int r = 0; r < 3; ++r) { bt[r] = t[r]; for (int c = 0; c < 3; ++c) bR[r][c] = R[r][c]; }
        }
    }
    if (!found) return false;
    angle_axis(bR, rt);
    for (int k = 0; k < 3; ++k) rt[3 + k] = bt[k];
    return true;
}

// OpenCV's planarity test on all keypoints (cvFindExtrinsicCameraParams2): eigenvalues of the centred scatter matrix
__device__ bool planar(const double *p3, int pn, int lane)
{
    double s[3] = {0, 0, 0};
    for (int i = lane; i < pn; i += 64)
        for (int k = 0; k < 3; ++k) s[k] += p3[i * 3 + k];
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = wave_sum(s[k]) / pn;
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (int i = lane; i < pn; i += 64) {
        const double d[3] = {p3[i * 3] - c[0], p3[i * 3 + 1] - c[1], p3[i * 3 + 2] - c[2]};
        m[0] += d[0] * d[0]; m[1] += d[0] * d[1]; m[2] += d[0] * d[2]; m[3] += d[1] * d[1]; m[4] += d[1] * d[2]; m[5] += d[2] * d[2];
    }
    for (int k = 0; k < 6; ++k) m[k] = wave_sum(m[k]);
    double A[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}}, V[3][3];
    eig3(A, V);
    double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2], t;
    if (l1 > l0) { t = l0; l0 = l1; l1 = t; }
    if (l2 > l0) { t = l0; l0 = l2; l2 = t; }
    if (l2 > l1) { t = l1; l1 = l2; l2 = t; }
    return !(l2 / l1 >= 1e-3);
}

// initial_pose_dlt(P, p, K, order_key): with_key selects the weighted form (order_key = the P3P key).  ws: 288 doubles of
// this wave's LDS.  pn >= 6.
__device__ void start_dlt(const double *p2, const double *p3, const double *wg, bool with_key, const double Ki[3][3], int pn,
                          int lane, double *ws, double rt[6])
{
    // the rows kept and their weights: keypoints with a positive key; fewer than six: the six best (stable, descending),
    // every key + 1e-12; row weight max(sqrt(key / max key), 1e-3)
    auto dkey = [&](int i) { const double k = wg[i * 3] + wg[i * 3 + 1]; return isfinite(k) ? fmax(k, 0.0) : 0.0; };
    int sel[6] = {0, 0, 0, 0, 0, 0};
    bool six = false;
    if (with_key) {
        int npos = 0;
        for (int i = lane; i < pn; i += 64) npos += dkey(i) > 0.0;
        npos = (int)wave_sum((double)npos);
        six = npos < 6;
        if (six)
            for (int s = 0; s < 6; ++s) sel[s] = wave_pick(dkey, pn, sel, s, false, lane);
    }
    auto kept = [&](int i) {
        if (!with_key) return true;
        if (!six) return dkey(i) > 0.0;
        bool k = false;
        for (int s = 0; s < 6; ++s) k |= sel[s] == i;
        return k;
    };
    auto wkey = [&](int i) { return six ? dkey(i) + 1e-12 : dkey(i); };
    double kmax = 0.0, cnt = 0.0, sP[3] = {0, 0, 0};
    for (int i = lane; i < pn; i += 64)
        if (kept(i)) {
            cnt += 1.0;
            for (int k = 0; k < 3; ++k) sP[k] += p3[i * 3 + k];
            if (with_key) kmax = fmax(kmax, wkey(i));
        }
    cnt = wave_sum(cnt);
    kmax = wave_max(kmax);
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = wave_sum(sP[k]) / cnt;
    double ss = 0.0;
    for (int i = lane; i < pn; i += 64)
        if (kept(i))
            for (int k = 0; k < 3; ++k) ss += (p3[i * 3 + k] - c[k]) * (p3[i * 3 + k] - c[k]);
    const double s = sqrt(wave_sum(ss) / cnt) + 1e-30;
    double *A = ws, *V = ws + 144;                             // A[12][12], V[12][12] row-major
    double M[3][4];
    if (six) {
        // Six rows of weight down to 1e-3: the normal matrix would square a condition number of ~1e5 and leave the null
        // vector to 1e-6 only.  Six keypoints make A itself 12 x 12, so its right singular vectors come from a one-sided
        // (Hestenes) Jacobi on A's columns, as accurate as the twin's svd(A).  Lane r owns row r of A and of V; a column
        // pair is rotated from its three dot products, reduced across the wave (the same bits in every lane).
        if (lane < 12) {
            const int i = min(max(sel[lane >> 1], 0), pn - 1);   // six distinct keypoints (pn >= 6); clamped all the same
            const double rw = fmax(sqrt(wkey(i) / kmax), 1e-3);
            const double u = p2[i * 2], v = p2[i * 2 + 1];
            const double n = (lane & 1) ? Ki[1][0] * u + Ki[1][1] * v + Ki[1][2] : Ki[0][0] * u + Ki[0][1] * v + Ki[0][2];
            const double Qh[4] = {(p3[i * 3] - c[0]) / s, (p3[i * 3 + 1] - c[1]) / s, (p3[i * 3 + 2] - c[2]) / s, 1.0};
            const int off = (lane & 1) ? 4 : 0;
            for (int q = 0; q < 12; ++q) { A[lane * 12 + q] = 0.0; V[lane * 12 + q] = lane == q ? 1.0 : 0.0; }
            for (int q = 0; q < 4; ++q) { A[lane * 12 + off + q] = rw * Qh[q]; A[lane * 12 + 8 + q] = -(rw * n) * Qh[q]; }
        }
        wave_sync();
        for (int sweep = 0; sweep < 30; ++sweep) {
            bool rotated = false;
            for (int p = 0; p < 11; ++p)
                for (int q = p + 1; q < 12; ++q) {
                    const double ap = lane < 12 ? A[lane * 12 + p] : 0.0, aq = lane < 12 ? A[lane * 12 + q] : 0.0;
                    const double alpha = wave_sum(ap * ap), beta = wave_sum(aq * aq), gamma = wave_sum(ap * aq);
                    if (fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;   // orthogonal to rounding (uniform)
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    if (zeta < 0.0) t = -t;
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    if (lane < 12) {                           // its own row only: no other lane reads it before the end
                        A[lane * 12 + p] = cs * ap - sn * aq;
                        A[lane * 12 + q] = sn * ap + cs * aq;
                        const double vp = V[lane * 12 + p], vq = V[lane * 12 + q];
                        V[lane * 12 + p] = cs * vp - sn * vq;
                        V[lane * 12 + q] = sn * vp + cs * vq;
                    }
                }
            if (!rotated) break;
        }
        int jmin = 0;
        double smin = INFINITY;
        for (int j = 0; j < 12; ++j) {                         // the smallest singular value: the shortest column of A
            const double a = lane < 12 ? A[lane * 12 + j] : 0.0;
            const double n2 = wave_sum(a * a);
            if (n2 < smin) { smin = n2; jmin = j; }
        }
        wave_sync();
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 4; ++q) M[r][q] = V[(4 * r + q) * 12 + jmin];
    } else {
        // A^T A of the 2pn x 12 system: rows w [Qh, 0, -nx Qh] and w [0, Qh, -ny Qh] -> four symmetric 4 x 4 sums
        double S[4][10];
        for (int b = 0; b < 4; ++b)
            for (int k = 0; k < 10; ++k) S[b][k] = 0.0;
        for (int i = lane; i < pn; i += 64) {
            if (!kept(i)) continue;
            double w2 = 1.0;
            if (with_key) { const double rw = fmax(sqrt(wkey(i) / kmax), 1e-3); w2 = rw * rw; }
            const double u = p2[i * 2], v = p2[i * 2 + 1];
            const double nx = Ki[0][0] * u + Ki[0][1] * v + Ki[0][2], ny = Ki[1][0] * u + Ki[1][1] * v + Ki[1][2];
            const double Qh[4] = {(p3[i * 3] - c[0]) / s, (p3[i * 3 + 1] - c[1]) / s, (p3[i * 3 + 2] - c[2]) / s, 1.0};
            const double wb[4] = {w2, w2 * nx, w2 * ny, w2 * (nx * nx + ny * ny)};
            int k = 0;
            for (int r = 0; r < 4; ++r)
                for (int q = r; q < 4; ++q, ++k) {
                    const double e = Qh[r] * Qh[q];
                    for (int b = 0; b < 4; ++b) S[b][k] += wb[b] * e;
                }
        }
        for (int b = 0; b < 4; ++b)
            for (int k = 0; k < 10; ++k) S[b][k] = wave_sum(S[b][k]);
        if (lane < 12) {
            for (int q = 0; q < 12; ++q) { A[lane * 12 + q] = 0.0; V[lane * 12 + q] = lane == q ? 1.0 : 0.0; }
        }
        wave_sync();
        if (lane == 0) {
            // blocks (row offset, column offset, sum, sign): [0:4,0:4] = [4:8,4:8] = S0, [0:4,8:12] = -S1, [4:8,8:12] = -S2,
            // [8:12,8:12] = S3, each symmetric, mirrored below the diagonal
            const int blk[5][4] = {{0, 0, 0, 1}, {4, 4, 0, 1}, {0, 8, 1, -1}, {4, 8, 2, -1}, {8, 8, 3, 1}};
            for (int e = 0; e < 5; ++e) {
                const int ro = blk[e][0], co = blk[e][1];
                int k = 0;
                for (int r = 0; r < 4; ++r)
                    for (int q = r; q < 4; ++q, ++k) {
                        const double val = blk[e][3] * S[blk[e][2]][k];
                        A[(ro + r) * 12 + co + q] = val; A[(co + q) * 12 + ro + r] = val;
                        A[(ro + q) * 12 + co + r] = val; A[(co + r) * 12 + ro + q] = val;
                    }
            }
        }
        wave_sync();
        // cyclic Jacobi on the 12 x 12 normal matrix, lane r owns row r (and, A being symmetric, column r) of A and of V
        for (int sweep = 0; sweep < 50; ++sweep) {
            double off = 0.0;
            if (lane < 12)
                for (int q = lane + 1; q < 12; ++q) off += fabs(A[lane * 12 + q]);
            if (wave_sum(off) == 0.0) break;
            for (int p = 0; p < 11; ++p)
                for (int q = p + 1; q < 12; ++q) {
                    const double apq = A[p * 12 + q], app = A[p * 12 + p], aqq = A[q * 12 + q];
                    if (apq == 0.0) continue;
                    const double g = 100.0 * fabs(apq);
                    const bool tiny = fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq);
                    double t = 0.0, sn = 0.0, tau = 0.0;
                    if (!tiny) {
                        const double theta = 0.5 * (aqq - app) / apq;
                        t = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                        const double cs = 1.0 / sqrt(1.0 + t * t);
                        sn = t * cs; tau = sn / (1.0 + cs);
                    }
                    if (lane < 12 && !tiny) {
                        if (lane != p && lane != q) {
                            const double gp = A[lane * 12 + p], hq = A[lane * 12 + q];
                            const double np_ = gp - sn * (hq + gp * tau), nq = hq + sn * (gp - hq * tau);
                            A[lane * 12 + p] = np_; A[p * 12 + lane] = np_;
                            A[lane * 12 + q] = nq; A[q * 12 + lane] = nq;
                        }
                        const double vp = V[lane * 12 + p], vq = V[lane * 12 + q];
                        V[lane * 12 + p] = vp - sn * (vq + vp * tau);
                        V[lane * 12 + q] = vq + sn * (vp - vq * tau);
                    }
                    if (lane == 0) {
                        if (!tiny) { A[p * 12 + p] = app - t * apq; A[q * 12 + q] = aqq + t * apq; }
                        A[p * 12 + q] = 0.0; A[q * 12 + p] = 0.0;
                    }
                    wave_sync();
                }
        }
        int jmin = 0;
        for (int j = 1; j < 12; ++j)
            if (A[j * 12 + j] < A[jmin * 12 + jmin]) jmin = j;
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 4; ++q) M[r][q] = V[(4 * r + q) * 12 + jmin];
    }
    wave_sync();                                              // the LDS rows are the refinement's next
    double M3[3][3] = {{M[0][0], M[0][1], M[0][2]}, {M[1][0], M[1][1], M[1][2]}, {M[2][0], M[2][1], M[2][2]}};
    if (det3(M3) < 0.0)
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 4; ++q) M[r][q] = -M[r][q];
            for (int q = 0; q < 3; ++q) M3[r][q] = -M3[r][q];
        }
    // polar decomposition M3 = R (V S V^T): R = M3 V S^-1 V^T, scale = mean singular value
    double G[3][3], W[3][3];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) G[r][q] = M3[0][r] * M3[0][q] + M3[1][r] * M3[1][q] + M3[2][r] * M3[2][q];
    eig3(G, W);
    double sg[3];
    for (int k = 0; k < 3; ++k) sg[k] = sqrt(fmax(G[k][k], 0.0));
    const double scale = (sg[0] + sg[1] + sg[2]) / 3.0;
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double mv = M3[r][0] * W[0][k] + M3[r][1] * W[1][k] + M3[r][2] * W[2][k];
                acc += mv / sg[k] * W[q][k];
            }
            R[r][q] = acc;
        }
    angle_axis(R, rt);
    // undo the conditioning: X = R ((P - c) / s) + t  =>  s X = R P + (s t - R c)
    for (int r = 0; r < 3; ++r) rt[3 + r] = s * (M[r][3] / scale) - (R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2]);
}

template <bool kRefine>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_pose(Args a)
{
    __shared__ double s_part[kWavesPerBlock][64][kSums + 1];
    __shared__ double s_sum[kWavesPerBlock][kSums];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWavesPerBlock + wave;
    if (b >= a.B) return;                                      // whole wave: no block-level barrier below
    const int pn = a.pn;
    const double *p2 = a.pts2d + (size_t)b * pn * 2;
    const double *p3 = a.pts3d + (a.pts3d_batched ? (size_t)b * pn * 3 : 0);
    const double *wg = a.wgt2d ? a.wgt2d + (size_t)b * pn * 3 : nullptr;
    const double *Kb = a.K + (a.K_batched ? (size_t)b * 9 : 0);
    double Kc[3][3], Ki[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Kc[r][c] = Kb[r * 3 + c];
    const double dK = det3(Kc);
    for (int r = 0; r < 3; ++r)                               // the adjugate over the determinant
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            Ki[r][c] = (Kc[r1][c1] * Kc[r2][c2] - Kc[r1][c2] * Kc[r2][c1]) / dK;
        }
    bool bad = false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) bad |= !isfinite(Kc[r][c]) || !isfinite(Ki[r][c]);
    for (int i = lane; i < pn; i += 64) {
        bad |= !isfinite(p2[i * 2]) || !isfinite(p2[i * 2 + 1]);
        bad |= !isfinite(p3[i * 3]) || !isfinite(p3[i * 3 + 1]) || !isfinite(p3[i * 3 + 2]);
        if (kRefine && wg) bad |= !isfinite(wg[i * 3]) || !isfinite(wg[i * 3 + 1]) || !isfinite(wg[i * 3 + 2]);
    }
    double x[6];
    int status;
    if (wave_any(bad)) {
        status = PVP_STATUS_NONFINITE;
    } else if (a.method == PVP_START_P3P && start_p3p(p2, p3, wg, Kc, Ki, pn, lane, x)) {
        status = PVP_STATUS_P3P;
    } else if (pn < 6) {
        status = PVP_STATUS_NO_START;
    } else if (planar(p3, pn, lane)) {
        status = PVP_STATUS_PLANAR;
    } else {
        const bool fallback = a.method == PVP_START_P3P;
        start_dlt(p2, p3, wg, fallback, Ki, pn, lane, &s_part[wave][0][0], x);
        status = fallback ? PVP_STATUS_DLT_FALLBACK : PVP_STATUS_DLT;
    }
    if (status < 0)
        for (int k = 0; k < 6; ++k) x[k] = NAN;
    if (lane == 0) a.status[b] = status;
    if (!kRefine) {
        if (lane < 6) a.rt[(size_t)b * 6 + lane] = x[lane];
        return;
    }
    if (a.init_rt && lane < 6) a.init_rt[(size_t)b * 6 + lane] = x[lane];
    LmInfo r = {NAN, NAN, 0, 0};
    bool refined = false;
    if (status >= 0 && !(status == PVP_STATUS_P3P && pn == 4)) {   // four keypoints: the P3P pose (un_pnp_utils.py:34-38)
        const Cam cam = {Kb[0], Kb[4], Kb[2], Kb[5]};
        r = wg ? lm_refine<false>(x, p2, p3, wg, cam, pn, a.max_iter, a.ftol, s_part[wave], s_sum[wave], lane)
               : lm_refine<true>(x, p2, p3, nullptr, cam, pn, a.max_iter, a.ftol, s_part[wave], s_sum[wave], lane);
        refined = true;
    }
    if (lane < 6) a.rt[(size_t)b * 6 + lane] = x[lane];
    if (a.info && lane == 0) {
        a.info[(size_t)b * 4] = r.initial_cost; a.info[(size_t)b * 4 + 1] = r.cost;
        a.info[(size_t)b * 4 + 2] = refined ? (double)r.iterations : NAN;
        a.info[(size_t)b * 4 + 3] = refined ? (double)r.termination : NAN;
    }
    if (a.Rt && lane < 12) {
        double R[3][3];
        rodrigues(x, R);
        const int row = lane >> 2, col = lane & 3;
        a.Rt[(size_t)b * 12 + lane] = col < 3 ? R[row][col] : x[3 + row];
    }
}

int launch(Args a, bool refine, hipStream_t st)
{
    if (a.B < 0 || a.pn < 4 || a.pn > 4096 || (a.method != PVP_START_P3P && a.method != PVP_START_DLT)) return -1;
    if (!a.pts2d || !a.pts3d || !a.K || !a.rt || !a.status || (a.method == PVP_START_P3P && !a.wgt2d)) return -1;
    if (a.B == 0) return 0;
    const dim3 grid((a.B + kWavesPerBlock - 1) / kWavesPerBlock), block(64 * kWavesPerBlock);
    if (refine) hipLaunchKernelGGL(k_pose<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_pose<false>, grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace

PVP_EXPORT int pvp_initial_pose_batched(const double *d_pts2d, const double *d_pts3d, const double *d_wgt2d,
                                        const double *d_K, int method, double *d_rt, int *d_status, int B, int pn,
                                        int pts3d_batched, int K_batched, void *stream)
{
    const Args a = {d_pts2d, d_pts3d, d_wgt2d, d_K, method, B, pn, pts3d_batched, K_batched, 0, 0.0,
                    d_rt, nullptr, nullptr, nullptr, d_status};
    return launch(a, false, (hipStream_t)stream);
}

PVP_EXPORT int pvp_pose_batched(const double *d_pts2d, const double *d_pts3d, const double *d_wgt2d, const double *d_K,
                                int method, double *d_result_rt, double *d_Rt, double *d_init_rt, int *d_status,
                                double *d_info, int B, int pn, int pts3d_batched, int K_batched, int max_iterations,
                                double function_tolerance, void *stream)
{
    const Args a = {d_pts2d, d_pts3d, d_wgt2d, d_K, method, B, pn, pts3d_batched, K_batched, max_iterations,
                    function_tolerance > 0.0 ? function_tolerance : 1e-6, d_result_rt, d_Rt, d_init_rt, d_info, d_status};
    return launch(a, true, (hipStream_t)stream);
}
