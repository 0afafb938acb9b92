"""numpy twin of the arithmetic contract of include/pvnet_metrics.h, written from the contract with the operation order
explicit (no np.dot, so no BLAS contraction or reordering), plus the bounds the device results are held to.  The CPU tests
pin this twin to the fixtures made by the reference's own evaluator (tests/golden/make_metrics_golden.py); the GPU tests
use it where the fixtures have no case.

Bounds (u = 2**-53, all derived, none tuned):
  mean distances  |got - want| <= 4*N*u*want + 32*u*cmax, cmax the largest absolute coordinate entering the difference.
                  Two fixed-order sums of N non-negative binary64 terms differ by at most 2(N-1)u relative, doubled for the
                  per-term roundings; the second term is the few roundings of each coordinate, all that is left when the
                  poses are identical and the distance is rounding noise.
  translation     8*u*|t|*100 (|t| the larger of the two translation norms).
  angle           rad2deg(2*sqrt(2*delta)), delta = 24*u: delta bounds the rounding of the nine products and eight additions
                  of the trace, arccos turns an error delta of its argument into at most sqrt(2*delta) (reached at 0 and 180
                  degrees), once for each of the two implementations.
  integers        equal.
"""
import numpy as np

U = 2.0 ** -53
ANG_BOUND_DEG = float(np.rad2deg(2.0 * np.sqrt(2.0 * 24 * U)))

LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def cloud(n, seed):
    """A seeded synthetic model of LINEMOD scale (metres): anisotropic Gaussian, float32, with a few exact duplicate points
    so that the tie rule of the search (first minimum wins) is exercised."""
    rng = np.random.RandomState(seed)
    m = (rng.randn(n, 3) * np.array([0.04, 0.03, 0.02])).astype(np.float32)
    if n > 10:
        m[7] = m[3]
        m[n - 1] = m[n // 2]
        m[n // 3] = m[3]
    return m


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose(w, t):
    return np.concatenate([rodrigues(w), np.asarray(t, np.float64).reshape(3, 1)], 1)


def transform(model, P):
    """x[:, i] = ((m0*R[i,0] + m1*R[i,1]) + m2*R[i,2]) + t[i], binary64, one rounding per operation."""
    m = np.asarray(model, np.float32).astype(np.float64)
    P = np.asarray(P, np.float64)
    return np.stack([((m[:, 0] * P[i, 0] + m[:, 1] * P[i, 1]) + m[:, 2] * P[i, 2]) + P[i, 3] for i in range(3)], 1)


def nearest(ref32, que32, chunk=512):
    """For every query the index of the nearest reference point: (dx*dx + dy*dy) + dz*dz in binary32, first minimum."""
    ref32, que32 = np.asarray(ref32, np.float32), np.asarray(que32, np.float32)
    out = np.zeros(que32.shape[0], np.int32)
    for q0 in range(0, que32.shape[0], chunk):
        q = que32[q0:q0 + chunk]
        dx = ref32[None, :, 0] - q[:, None, 0]
        dy = ref32[None, :, 1] - q[:, None, 1]
        dz = ref32[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        out[q0:q0 + chunk] = np.argmin(d, 1)                       # argmin returns the first minimum
    return out


def _norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def project(x, K):
    K = np.asarray(K, np.float64)
    u = [(x[:, 0] * K[i, 0] + x[:, 1] * K[i, 1]) + x[:, 2] * K[i, 2] for i in range(3)]
    return np.stack([u[0] / u[2], u[1] / u[2]], 1)


def cm_degree(Pp, Pg):
    d = Pp[:, 3] - Pg[:, 3]
    trans = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * 100
    tr = None
    for i in range(3):
        di = (Pp[i, 0] * Pg[i, 0] + Pp[i, 1] * Pg[i, 1]) + Pp[i, 2] * Pg[i, 2]
        tr = di if tr is None else tr + di
    tr = tr if tr <= 3 else 3
    tr = tr if tr >= -1 else -1
    return trans, np.rad2deg(np.arccos((tr - 1.0) / 2.0))


def pose_metrics(Pp, Pg, model, K, symmetric=True, search=nearest):
    """The five values of one pose pair, the neighbour indices and the magnitudes the bounds need."""
    Pp, Pg = np.asarray(Pp, np.float64), np.asarray(Pg, np.float64)
    n = model.shape[0]
    nan = float("nan")
    if not (np.isfinite(Pp).all() and np.isfinite(Pg).all()):
        return {"add": nan, "adds": nan, "proj2d": nan, "trans_cm": nan, "ang_deg": nan, "adds_idx": np.zeros(n, np.int32),
                "cmax3d": 0.0, "cmax2d": 0.0, "tnorm": 0.0}
    xp, xg = transform(model, Pp), transform(model, Pg)
    out = {"add": float(np.sum(_norm3(xp - xg)) / n)}
    if symmetric:
        idx = search(xp.astype(np.float32), xg.astype(np.float32))
        out["adds_idx"] = idx.astype(np.int32)
        out["adds"] = float(np.sum(_norm3(xp[idx] - xg)) / n)
    else:
        out["adds_idx"] = np.zeros(n, np.int32)
        out["adds"] = nan
    up, ug = project(xp, K), project(xg, K)
    d = up - ug
    out["proj2d"] = float(np.sum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])) / n)
    t, a = cm_degree(Pp, Pg)
    out["trans_cm"], out["ang_deg"] = float(t), float(a)
    out["cmax3d"] = float(max(np.abs(xp).max(), np.abs(xg).max()))
    out["cmax2d"] = float(max(np.abs(up).max(), np.abs(ug).max()))
    out["tnorm"] = float(max(np.linalg.norm(Pp[:, 3]), np.linalg.norm(Pg[:, 3])))
    return out


def bounds(want, n):
    """The largest |got - want| allowed per value for a twin result ``want`` (see the module docstring)."""
    mean = lambda v, cmax: 4.0 * n * U * abs(v) + 32.0 * U * cmax                # noqa: E731
    return {"add": mean(want["add"], want["cmax3d"]),
            "adds": mean(want["adds"], want["cmax3d"]) if np.isfinite(want["adds"]) else 0.0,
            "proj2d": mean(want["proj2d"], want["cmax2d"]),
            "trans_cm": 8.0 * U * want["tnorm"] * 100.0,
            "ang_deg": ANG_BOUND_DEG}


def assert_close(got, want, n, what=""):
    """``got``: the five values as floats; ``want``: a ``pose_metrics`` result.  Prints each figure before it asserts."""
    bd = bounds(want, n)
    for k in ("add", "adds", "proj2d", "trans_cm", "ang_deg"):
        g, w = float(got[k]), float(want[k])
        if np.isnan(w):
            print("%s %-8s got %r want nan" % (what, k, g))
            assert np.isnan(g), (what, k, g)
            continue
        print("%s %-8s got %.17g want %.17g |diff| %.3g bound %.3g" % (what, k, g, w, abs(g - w), bd[k]))
        assert abs(g - w) <= bd[k], (what, k, g, w, abs(g - w), bd[k])


def hits(vals, diameter, symmetric, percentage=0.1, proj_threshold=5.0):
    """The reference's three comparisons on one image's values (a comparison with NaN is a miss)."""
    dist = vals["adds"] if symmetric else vals["add"]
    return {"add": bool(dist < diameter * percentage), "proj2d": bool(vals["proj2d"] < proj_threshold),
            "cmd5": bool(vals["trans_cm"] < 5 and vals["ang_deg"] < 5)}
