"""Inputs that put the pose solver on the branches random poses never reach: rotations at and around a half turn and the
identity, every exit of the Levenberg-Marquardt refinement, non-finite input, the DLT's six-best selection, Grunert's quartic
with a vanishing end coefficient, skewed and singular cameras.  Test infrastructure: plain numpy, shared by the CPU
preconditions (tests/test_pose.py, which keep each input on its branch) and the GPU tests (tests/test_gpu_pose_edges.py)."""
from unittest import mock

import numpy as np

from oracle import pnp_oracle as po
from tests.test_pnp import KMAT

AXES = [np.array(a, np.float64) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 1), np.ones(3) / np.sqrt(3.0), (0.6, -0.8, 0.0),
                                          (-0.36, 0.48, 0.8))]
ROUND_TRIP_ANGLES = [0.0, 1e-12, 1e-10, 1e-9, 2e-9, 1e-6, 1.0] + [np.pi - d for d in (0.5, 1e-2, 1e-3, 1e-4, 1e-5, 2e-6, 1.1e-6,
                                                                                  9e-7, 3e-7, 1e-9, 0.0)]
START_ANGLES = [0.0, 1e-10, 2e-9, np.pi] + [np.pi - d for d in (3e-7, 1.1e-6, 2e-6, 1e-5, 1e-4, 1e-3)]
THETA2_SWITCH = 2.220446049250313e-16          # rotate_point's first-order branch: theta2 <= this (pnp_lm.hpp, rotation.h)


def round_trip_axes():
    """The six fixed axes (coordinate axes, the diagonal that ties the three diagonal entries, two in general position with
    exact and inexact squares) and 20 seeded random ones."""
    rng = np.random.RandomState(20261020)
    rnd = rng.randn(20, 3)
    return AXES + [a / np.linalg.norm(a) for a in rnd]


def project(rt, P, K=KMAT):
    """Pixel coordinates of the object points P under pose rt through the full camera matrix K (skew included)."""
    X = np.array([po.angle_axis_rotate_point(rt[:3], p) for p in P]) + rt[3:]
    h = (K @ (X / X[:, 2:]).T).T
    return h[:, :2]


def posed(seed, w, pn=9, noise=0.0, K=KMAT):
    """tests.test_pnp.problem's instance (same draws, same order) with the rotation set to w: -> p2, P, W, rt."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(-0.06, 0.06, (pn, 3))
    rt = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.1, 0.1, 2), rng.uniform(0.6, 1.1, 1)])
    rt[:3] = w
    p2 = project(rt, P, K) + rng.randn(pn, 2) * noise
    W = np.stack([rng.uniform(0.2, 2.0, pn), rng.uniform(-0.3, 0.3, pn), rng.uniform(0.2, 2.0, pn)], 1)
    return p2, P, W, rt


def half_turn_starts(angle):
    """Noise-free 9-keypoint instances rotated by `angle` about each of the six fixed axes.  The seeds are ones whose P3P
    triple stays clear of a double root of Grunert's quartic at every angle of START_ANGLES (one seed in six does not: the
    start is then determined to ~1e-6 only, whatever the conversion to angle-axis does; test_gpu_pose.py covers those)."""
    return [posed(seed, a * angle) for seed, a in zip((300, 311, 321, 330, 343, 351), AXES)]


# ------------------------------------------------------------------------------------------------ the refinement
def _case(name, p2, P, W, init, expect=None, **kw):
    return dict(name=name, p2=p2, P=P, W=W, init=np.asarray(init, np.float64), expect=expect, kw=kw)


def lm_cases():
    """Refinement inputs compared with po.solve_lm iterate for iterate.  `expect` is the termination the twin must give on
    the CPU (None: whatever it gives), `kw` the options of the call."""
    out = []
    # starts on either side of rotate_point's first-order branch; the truth is the identity
    p2, P, W, rt = posed(41, np.zeros(3), noise=1.0)
    t0 = rt[3:] + np.array([0.004, -0.003, 0.02])
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    for name, w in (("w_zero", np.zeros(3)), ("w_1e-9", np.array([1e-9, -2e-9, 5e-10])), ("w_below_switch", 1.4e-8 * u),
                    ("w_above_switch", 1.6e-8 * u)):
        out.append(_case(name, p2, P, W, np.concatenate([w, t0]), expect=3))
    # a start beyond the half turn, the truth short of it, about the same axis
    a = AXES[5]
    p2, P, W, rt = posed(42, a * (np.pi - 0.02), noise=1.0)
    out.append(_case("across_half_turn", p2, P, W, np.concatenate([a * (np.pi + 0.03), rt[3:] + [0.003, -0.002, 0.01]]), expect=3))
    # termination 1: at the minimum of a noise-free instance; no weight at all
    p2, P, W, rt = posed(43, np.array([0.3, -0.2, 0.5]))
    out.append(_case("at_the_truth", p2, P, 0.1 * W, rt, expect=1))   # weights 0.1: the rounding-sized gradient is ~1e-12
    p2, P, W, rt = posed(44, np.array([-0.4, 0.1, 0.7]), noise=1.0)
    init = rt + np.array([0.05, -0.04, 0.03, 0.004, -0.006, 0.02])
    out.append(_case("no_weight", p2, P, 0.0 * W, init, expect=1))
    # termination 0: the iteration limit
    for n in (1, 2):
        out.append(_case("limit_%d" % n, p2, P, W, init, expect=0, max_iterations=n))
    # 1, 2, 3 weighted keypoints of 9: a rank-deficient normal matrix
    for n in (1, 2, 3):
        Wn = W.copy()
        Wn[n:] = 0.0
        out.append(_case("weighted_%d_of_9" % n, p2, P, Wn, init, expect=2))
    # keypoint counts around the 64-lane loop
    for pn in (63, 64, 65, 128, 129):
        q2, qP, qW, qrt = posed(50 + pn, np.array([0.2, 0.9, -0.4]), pn=pn, noise=1.0)
        out.append(_case("pn_%d" % pn, q2, qP, qW, qrt + np.array([0.05, -0.04, 0.03, 0.004, -0.006, 0.02])))
    return out


def batch_of_five():
    """Five different 9-keypoint problems: one batched call must equal the five single calls bit for bit (a block holds
    four images, so the second block runs one live wave)."""
    out = []
    for s in range(5):
        p2, P, W, rt = posed(60 + s, np.array([0.5 - 0.2 * s, 0.1 * s, -0.3]), noise=1.0)
        out.append(_case("batch_%d" % s, p2, P, W, rt + np.array([0.05, -0.04, 0.03, 0.004, -0.006, 0.02])))
    return out


def inside_the_object():
    """A start that puts the camera inside the object (tz = 0.03, initial cost ~1e9): compared at the minimum only."""
    p2, P, W, rt = posed(45, np.array([0.3, 0.2, -0.4]), noise=1.0)
    init = rt + np.array([0.05, -0.04, 0.03, 0.004, -0.006, 0.0])
    init[5] = 0.03
    return _case("inside_the_object", p2, P, W, init, max_iterations=200, function_tolerance=1e-15)


def nonfinite_cases():
    """One NaN in a keypoint, a weight, a model point, the start; and a finite start that puts a keypoint at z = 0.  The
    refinement from a given start does not screen its input: it must fail as its twin does (termination 4, x = start)."""
    p2, P, W, rt = posed(46, np.array([0.1, -0.6, 0.3]), noise=1.0)
    init = rt + np.array([0.05, -0.04, 0.03, 0.004, -0.006, 0.02])
    out = []
    for name, k in (("nan_p2", 0), ("nan_W", 2), ("nan_P", 1), ("nan_init", 3)):
        arrs = [p2.copy(), P.copy(), W.copy(), init.copy()]
        arrs[k].reshape(-1)[4] = np.nan
        out.append(_case(name, arrs[0], arrs[1], arrs[2], arrs[3], expect=4))
    z0 = init.copy()
    z0[:3] = 0.0                                                    # X = P + t exactly: keypoint 2 lands on z = 0
    z0[5] = -P[2, 2]
    out.append(_case("z_zero", p2, P, W, z0, expect=4))
    return out


# ------------------------------------------------------------------------------------------------ the start
def skew_cameras(n):
    """One camera per image, every one with skew K[0,1] = 1.7."""
    Ks = []
    for i in range(n):
        K = KMAT.copy()
        K[0, 1] = 1.7
        K[0, 0] *= 1.0 + 0.01 * i
        K[1, 2] += 3.0 * i
        Ks.append(K)
    return Ks


def skew_problems():
    """(problems, cameras): one noisy 9-keypoint instance per skewed camera.  The seeds are ones whose P3P triple is clear of
    a double root (two in ten are not), so that both starts are determined to 1e-9 and compared at the floor of 1e-7."""
    Ks = skew_cameras(6)
    return [posed(801 + 10 * i, np.array([0.3, -0.5, 0.2 * i]), K=K, noise=0.5) for i, K in enumerate(Ks)], Ks


def lane_loop_problems(pn, method):
    """Noisy instances with pn keypoints; for P3P from seeds clear of a double root, as above; one instance at 4096."""
    seeds = {("p3p", 64): (964, 974), ("p3p", 65): (965, 975)}.get((method, pn), (850 + pn, 851 + pn)[:1 if pn == 4096 else 2])
    return [posed(s, np.array([0.3, -0.5, 0.2 * i]), pn=pn, noise=1.0) for i, s in enumerate(seeds)]


SIX_PATH_SEEDS = {9: (0, 1, 4), 17: (0, 7, 9)}


def six_path_cases(seeds=None):
    """P3P has no solution (its three keypoints are collinear) and only four keypoints carry a positive key: the DLT fallback
    must take the six best keys -- four positive, then the zeros (0, negative, NaN, +inf all count as 0) in index order.
    Two of the six rows weigh 1e-3 and three of the six points lie on a line, so the start is barely determined: detection
    noise of 1e-3 px already moves it by 1e-3 to 0.3, and at 0.5 px the 12 x 12 system's null vector is no pose at all (its
    3 x 3 block has a condition number of 1e4 to 1e6, which orthogonalising it multiplies rounding by in any implementation).
    Hence 1e-3 px: enough for a wrong choice among the tied keys to move the start by a hundred bounds and more, little enough
    for the start to be a pose.  SIX_PATH_SEEDS are those of the first twelve seeds per keypoint count whose second route
    (eigh of A^T A) stays within 1e-7 of the first, so that no bound exceeds 1e-5.  -> (p2, P, W, rt) per case, rt the true pose."""
    out = []
    for pn in (9, 17):
        for s in (SIX_PATH_SEEDS if seeds is None else seeds)[pn]:
            p2, P, W, rt = posed(500 + 10 * s + pn, np.array([0.4 - 0.3 * (s % 3), -0.2, 0.3 + 0.2 * (s % 3)]), pn=pn)
            rng = np.random.RandomState(900 + 10 * s + pn)
            pos = np.sort(rng.choice(pn, 4, replace=False))
            W = W.copy()
            W[:, 1] = 0.0                                         # key = wxx
            fill = [0.0, -0.7, np.nan, np.inf, 0.0]                  # five at least are left over: every kind each time
            rest = [i for i in range(pn) if i not in pos]
            for n, i in enumerate(rest):
                W[i, 0] = fill[(n + s) % len(fill)]
            W[pos, 0] = [0.5, 1.1, 0.8, 1.7]
            order = pos[np.argsort(W[pos, 0])]                    # ascending: P3P runs on order[:3], order[3] chooses
            P, p2 = P.copy(), p2.copy()
            P[order[2]] = 0.3 * P[order[0]] + 0.7 * P[order[1]]
            p2[order[2]] = project(rt, P[order[2]][None])[0]
            p2 = p2 + rng.randn(pn, 2) * 1e-3
            out.append((p2, P, W, rt))
    return out


def _kabsch(P, X):
    cP, cX = P.mean(0), X.mean(0)
    U, _S, Vt = np.linalg.svd((P - cP).T @ (X - cX))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cX - R @ cP


WIDE_K = np.array([[128.0, 0, 256.0], [0, 128.0, 128.0], [0, 0, 1.0]])     # its inverse is exact in binary64
_N60 = np.array([[1.0, 0.0, 1.0], [0.375, 1.625, 1.0]])                    # two normalised image points exactly 60 degrees apart


def zero_coefficient_case(which):
    """Grunert's quartic with coef[0] == 0 (which = 0) or coef[4] == 0 (which = 4), exactly.  The P3P triple is equilateral
    with exactly equal computed sides (q == 0, r == 2, c2 / b2 == a2 / b2 == 1), which leaves coef[0] = 1 - 4 ca^2 and
    coef[4] = 1 - 4 cg^2: zero when the bearings of P1, P2 (of P0, P1) are 60 degrees apart and their computed dot product
    is exactly 0.5.  The pixels of those two keypoints are WIDE_K (1, 0, 1) and WIDE_K (0.375, 1.625, 1): dyadic, so the
    normalised points are exact wherever they are computed, and the dot product of the unit bearings rounds to 0.5 in every
    order of evaluation, fused or not (tests/test_pose.py asserts every one).  A right-angled triple with
    perpendicular bearings would zero the same coefficients, but no pair of unit bearings has a dot product that is exactly 0
    under a fused multiply-add: the last product would have to be exact.
    -> p2, P, W, R, t (9 keypoints; the keys select the triple in order; R, t the true pose)."""
    rng = np.random.RandomState(700 + which)
    P = np.concatenate([0.5 * np.eye(3), rng.uniform(-0.3, 0.3, (6, 3)) + [0.2, 0.2, 0.1]])
    ends = {0: (1, 2), 4: (0, 1)}[which]
    third = {0: 0, 4: 2}[which]
    L = np.sqrt(0.5)
    f = _N60 / np.linalg.norm(_N60, axis=1, keepdims=True)
    X = np.zeros((3, 3))
    X[ends[0]], X[ends[1]] = L * f[0], L * f[1]                    # both at distance L, 60 degrees apart: L from each other
    d = X[ends[0]] - X[ends[1]]
    e = np.array([0.0, 0.0, 1.0]) - d * d[2] / (d @ d)             # away from the camera, square to that side
    X[third] = (X[ends[0]] + X[ends[1]]) / 2 + L * np.sqrt(0.75) * e / np.linalg.norm(e)
    R, t = _kabsch(P[:3], X)
    Xc = P @ R.T + t
    p2 = (WIDE_K @ (Xc / Xc[:, 2:]).T).T[:, :2]
    p2[ends[0]] = (WIDE_K @ _N60[0])[:2]                           # exactly, not to rounding
    p2[ends[1]] = (WIDE_K @ _N60[1])[:2]
    W = np.stack([rng.uniform(0.2, 0.4, 9), np.zeros(9), rng.uniform(0.2, 2.0, 9)], 1)
    W[:3, 0] = [1.0, 1.1, 1.2]                                     # ascending keys: the triple in order, then ...
    W[3 + int(np.argmax(Xc[3:, 2])), 0] = 1.5                      # ... the keypoint that chooses among the solutions
    return p2, P, W, R, t


def p3p_coefficients(P3, f):
    """The five coefficients un_pnp_utils.p3p_depths hands to np.roots, captured from the twin itself."""
    from clean_pvnet_amd.un_pnp_utils import p3p_depths
    seen = []
    roots = np.roots

    def spy(c):
        seen.append(np.array(c, np.float64))
        return roots(c)
    with mock.patch.object(np, "roots", spy):
        p3p_depths(f, P3)
    return seen[0]


# ------------------------------------------------------------------------------------------------ the host twins' starts
def _stable_rank(key):
    """A key with the device's tie rule made explicit: initial_pose_p3p's argsort(key)[-4:] then selects as a stable sort."""
    k = np.where(np.isfinite(key), key, -np.inf)
    return np.argsort(np.argsort(k, kind="stable"), kind="stable").astype(np.float64)


def twin_start(P, p2, W, K, method):
    """(rt, status) of the host twins, as the device defines them: test_gpu_pose._twin_start for any camera and method."""
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt, initial_pose_p3p
    if method == "dlt":
        return (initial_pose_dlt(P, p2, K), 1) if P.shape[0] >= 6 else (None, -1)
    key = W[:, 0] + W[:, 1]
    rt = initial_pose_p3p(P, p2, K, _stable_rank(key))
    if rt is not None:
        return rt, 0
    if P.shape[0] < 6:
        return None, -1
    return initial_pose_dlt(P, p2, K, order_key=key), 2


def pose_distance(a, b, raw=False):
    """max |difference| of two poses: of the raw six numbers, or of (R, t)."""
    from clean_pvnet_amd.un_pnp_utils import rodrigues
    if raw:
        return float(np.abs(a - b).max())
    return max(float(np.abs(rodrigues(a[:3]) - rodrigues(b[:3])).max()), float(np.abs(a[3:] - b[3:]).max()))


def twin_uncertainty(P, p2, W, K, method, want, raw=False):
    """The twin's own rounding uncertainty: its start by a second route -- the quartic's roots from the reversed polynomial
    (test_gpu_pose._start_tolerance), the 12-column system's null vector from the eigenvectors of A^T A (np.linalg.eigh)
    instead of svd(A) -- against the first."""
    roots, svd = np.roots, np.linalg.svd

    def reversed_roots(c):
        r = roots(np.asarray(c)[::-1])
        return 1.0 / r[r != 0]

    def svd_by_eigh(A, *a, **k):
        if getattr(A, "ndim", 0) != 2 or A.shape[1] != 12:
            return svd(A, *a, **k)
        lam, V = np.linalg.eigh(A.T @ A)
        return None, np.sqrt(np.clip(lam[::-1], 0, None)), V[:, ::-1].T          # rows by descending singular value
    with mock.patch.object(np, "roots", reversed_roots), mock.patch.object(np.linalg, "svd", svd_by_eigh):
        other, _ = twin_start(P, p2, W, K, method)
    if other is None or want is None:
        return 0.0
    return pose_distance(other, want, raw)
