"""The pose solver on the branches random poses never reach (inputs: tests/pose_edges.py; their CPU preconditions:
tests/test_pose.py), on the MI355X against its host twins:
  the start kernel (csrc/pvnet_pose.hip) at half turns and the identity, on the DLT's six-best path, with a skewed and a
  singular camera, with Grunert's quartic short of its leading or trailing coefficient, around the 64-lane loop;
  the refinement (csrc/pnp_lm.hpp) at every termination, on both sides of the first-order rotation branch, across the half
  turn, with a rank-deficient normal matrix, and on non-finite input, iterate for iterate against po.solve_lm.
Starts are compared as (R, t), not as raw angle-axis vectors, wherever the rotation is near a half turn: there w and -w are
the same rotation.  The tolerance of a start is test_gpu_pose.py's: max(1e-7, 100 x the twin's own uncertainty), the
uncertainty being the twin's start computed a second way (np.roots on the reversed quartic; the DLT's null vector from
eigh(A^T A) instead of svd(A))."""
import numpy as np
import pytest

from oracle import pnp_oracle as po
from tests import pose_edges as E
from tests.pose_edges import pose_distance, twin_start, twin_uncertainty
from tests.test_pnp import KMAT

pytestmark = pytest.mark.gpu


def _t(gpu, arrays):
    import torch
    return torch.tensor(np.stack(arrays), dtype=torch.float64, device=gpu)


def _device_start(gpu, probs, Ks, method):
    """probs: (p2, P, W, ...) per image; Ks: one camera or one per image."""
    import torch
    from clean_pvnet_amd.pose import initial_pose_batched
    Kt = _t(gpu, Ks) if isinstance(Ks, list) else torch.tensor(Ks, dtype=torch.float64, device=gpu)
    rt, st = initial_pose_batched(_t(gpu, [q[0] for q in probs]), _t(gpu, [q[1] for q in probs]), Kt,
                                  _t(gpu, [q[2] for q in probs]), method=method)
    return rt.cpu().numpy(), st.cpu().numpy()


def _check_starts(gpu, probs, Ks, method, raw=True, cap=1e-7, what=""):
    """Device start == twin start for every image, status included, within max(1e-7, 100 x the twin's own uncertainty).
    `cap` is the largest bound an image may need: 1e-7 says that no image of the call is ill-conditioned, so that the floor
    decides for every one.  -> (statuses, the bounds used, the device starts)."""
    rt, st = _device_start(gpu, probs, Ks, method)
    bounds = []
    with np.errstate(all="ignore"):
        for i, q in enumerate(probs):
            p2, P, W = q[:3]
            K = Ks[i] if isinstance(Ks, list) else Ks
            want, status = twin_start(P, p2, W, K, method)
            assert st[i] == status, (what, method, i, st[i], status)
            if want is None:
                assert np.isnan(rt[i]).all()
                continue
            assert np.isfinite(rt[i]).all(), (what, method, i, rt[i])
            unc = twin_uncertainty(P, p2, W, K, method, want, raw)
            tol = max(1e-7, 1e2 * unc)
            bounds.append(tol)
            assert tol <= cap, (what, method, i, "the twin itself is ill-conditioned here", unc)
            d = pose_distance(rt[i], want, raw)
            print("[pose-edges] %s %s image %d: |device - twin| = %.3g, bound %.3g" % (what, method, i, d, tol))
            assert d <= tol, (what, method, i, d, tol)
    return st, bounds, rt


# ------------------------------------------------------------------------------------------------ 1. half turns
@pytest.mark.parametrize("method", ["dlt", "p3p"])
def test_starts_at_half_turns_and_the_identity_equal_the_twin_and_the_truth(pkg, gpu, method):
    """Six axes x ten angles from 0 to pi, noise-free, nine keypoints.  The bound never exceeds 1e-6: the twin's two routes
    agree to 1e-8 at every angle (before the angle-axis conversion was replaced they disagreed by 4.4e-4 at pi - 2e-6)."""
    worst = 0.0
    for th in E.START_ANGLES:
        probs = E.half_turn_starts(th)
        st, bounds, rt = _check_starts(gpu, probs, KMAT, method, raw=False, cap=1e-6, what="angle pi - %.3g" % (np.pi - th))
        assert (st == (1 if method == "dlt" else 0)).all(), (th, st)
        for i, q in enumerate(probs):                            # noise-free: the start is the pose
            d = pose_distance(rt[i], q[3])
            worst = max(worst, d)
            assert d <= bounds[i], (method, th, i, d, bounds[i])
            assert np.linalg.norm(rt[i, :3]) <= np.pi * (1 + 2 * np.finfo(np.float64).eps)
    print("\n[pose-edges] %s start at half turns / identity: max distance to the true pose %.3g" % (method, worst))


# ------------------------------------------------------------------------------------------------ 2. the refinement
def _refine(gpu, cases, **kw):
    from clean_pvnet_amd.un_pnp_utils import uncertainty_pnp_batched
    import torch
    rt, info = uncertainty_pnp_batched(_t(gpu, [c["p2"] for c in cases]), _t(gpu, [c["W"] for c in cases]),
                                       _t(gpu, [c["P"] for c in cases]), torch.tensor(KMAT, device=gpu),
                                       _t(gpu, [c["init"] for c in cases]), return_info=True, **kw)
    return rt.cpu().numpy(), info.cpu().numpy()


def _equals_the_twin(c, rt, info):
    """test_pnp.py's rule: pose within 1e-9, costs within 1e-9 relative, iteration count and termination equal."""
    kw = {k: v for k, v in c["kw"].items() if k == "max_iterations"}
    with np.errstate(all="ignore"):
        x, inf = po.solve_lm(c["init"], c["p2"], c["P"], c["W"], KMAT, **kw)
    assert int(info[2]) == inf["iterations"] and int(info[3]) == inf["termination"], (c["name"], info, inf)
    np.testing.assert_allclose(rt, x, rtol=0, atol=1e-9, err_msg=c["name"])
    np.testing.assert_allclose(info[:2], [inf["initial_cost"], inf["final_cost"]], rtol=1e-9, atol=1e-15, err_msg=c["name"])
    return inf


@pytest.mark.parametrize("name", [c["name"] for c in E.lm_cases()])
def test_refinement_branch_equals_the_lm_twin(pkg, gpu, name):
    c = [c for c in E.lm_cases() if c["name"] == name][0]
    rt, info = _refine(gpu, [c], **c["kw"])
    inf = _equals_the_twin(c, rt[0], info[0])
    if c["expect"] is not None:
        assert inf["termination"] == c["expect"]
    assert np.isfinite(rt).all() and np.isfinite(info).all()


def test_refinement_batch_of_five_equals_its_single_calls_bit_for_bit(pkg, gpu):
    cases = E.batch_of_five()
    rt, info = _refine(gpu, cases)
    for i, c in enumerate(cases):
        one_rt, one_info = _refine(gpu, [c])
        assert np.array_equal(rt[i], one_rt[0]) and np.array_equal(info[i], one_info[0]), c["name"]
        _equals_the_twin(c, rt[i], info[i])


def test_refinement_from_inside_the_object_reaches_the_minimum(pkg, gpu):
    from tests.test_gpu_pose import _same_minimum
    c = E.inside_the_object()
    rt, info = _refine(gpu, [c], **c["kw"])
    xs, _ = po.solve_scipy(c["init"], c["p2"], c["P"], c["W"], KMAT)
    assert info[0, 0] > 1e8 and np.isfinite(rt).all()
    _same_minimum(rt[0], xs, c["p2"], c["P"], c["W"], c["name"])


# ------------------------------------------------------------------------------------------------ 3. non-finite input
@pytest.mark.parametrize("name", [c["name"] for c in E.nonfinite_cases()])
def test_refinement_fails_on_nonfinite_input_as_the_twin_does(pkg, gpu, name):
    """The start comes back bit for bit, termination 4 (never 1: a NaN gradient is not a converged one) after the twin's 14
    iterations, NaN costs; the images on either side of it in the batch keep the bits they have alone."""
    c = [c for c in E.nonfinite_cases() if c["name"] == name][0]
    good = E.batch_of_five()[:2]
    rt, info = _refine(gpu, [good[0], c, good[1]])
    with np.errstate(all="ignore"):
        x, inf = po.solve_lm(c["init"], c["p2"], c["P"], c["W"], KMAT)
    assert inf["termination"] == 4 and np.array_equal(x, c["init"], equal_nan=True)
    same_bits = np.ascontiguousarray(rt[1]).view(np.uint64) == c["init"].view(np.uint64)
    assert (same_bits | (np.isnan(rt[1]) & np.isnan(c["init"]))).all(), (rt[1], c["init"])   # NaN compares as NaN
    assert int(info[1, 3]) == 4 and int(info[1, 2]) == inf["iterations"] == 14, info[1]
    assert np.isnan(info[1, :2]).all() and np.isnan([inf["initial_cost"], inf["final_cost"]]).all()
    for k, g in ((0, good[0]), (2, good[1])):
        one_rt, one_info = _refine(gpu, [g])
        assert np.array_equal(rt[k], one_rt[0]) and np.array_equal(info[k], one_info[0]), (name, k)


# ------------------------------------------------------------------------------------------------ 4. the start kernel
def test_six_best_path_of_the_dlt_fallback_equals_the_twin(pkg, gpu):
    """The existing rule, unchanged: max(1e-7, 100 x the twin's second route).  The second route takes the null vector from
    eigh(A^T A), which squares a condition number of ~1e5 on this path (two of the six rows weigh 1e-3), so the bounds run
    are up to 1e-5 here; the device takes a one-sided Jacobi SVD of the 12 x 12 system itself and stays far inside them."""
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt
    probs = E.six_path_cases()
    for pn in (9, 17):
        grp = [q for q in probs if q[1].shape[0] == pn]
        st, _b, rt = _check_starts(gpu, grp, KMAT, "p3p", cap=1e-5, what="six of %d" % pn)
        assert (st == 2).all(), st
        for i, (p2, P, W, true_rt) in enumerate(grp):            # the twin's start IS the keyed DLT
            with np.errstate(all="ignore"):
                want = initial_pose_dlt(P, p2, KMAT, order_key=W[:, 0] + W[:, 1])
            assert np.array_equal(want, twin_start(P, p2, W, KMAT, "p3p")[0])
            assert pose_distance(rt[i], true_rt) <= 0.02, (pn, i)    # 1e-3 px of noise: still a pose


@pytest.mark.parametrize("method", ["dlt", "p3p"])
def test_start_with_a_skewed_camera_per_image_equals_the_twin(pkg, gpu, method):
    probs, Ks = E.skew_problems()
    st, _b, _rt = _check_starts(gpu, probs, Ks, method, what="skew")
    assert (st == (1 if method == "dlt" else 0)).all(), st


@pytest.mark.parametrize("method", ["dlt", "p3p"])
def test_a_singular_camera_fails_alone(pkg, gpu, method):
    """A zero focal length: status -3 and NaN for that image; its neighbours keep the bits they have without it."""
    Ks = E.skew_cameras(5)
    probs = [E.posed(820 + i, np.array([0.3, -0.5, 0.2 * i]), K=K, noise=0.5) for i, K in enumerate(Ks)]
    good_rt, good_st = _device_start(gpu, probs, Ks, method)
    bad = [K.copy() for K in Ks]
    bad[1][0, 0] = 0.0
    bad[4][1, 1] = 0.0                                           # the single live wave of the second block
    rt, st = _device_start(gpu, probs, bad, method)
    assert st.tolist() == [good_st[0], -3, good_st[2], good_st[3], -3] and (good_st >= 0).all()
    assert np.isnan(rt[[1, 4]]).all()
    assert np.array_equal(rt[[0, 2, 3]], good_rt[[0, 2, 3]])


@pytest.mark.parametrize("which", [0, 4])
def test_p3p_with_a_zero_end_coefficient_of_the_quartic_equals_the_twin(pkg, gpu, which):
    """coef[0] == 0 (a cubic: np.roots drops the leading zero) and coef[4] == 0 (the root 0, rejected): the device's
    Durand-Kerner must take the same reduced polynomial.  tests/test_pose.py asserts that the twin's coefficient is exactly 0."""
    p2, P, W, R, t = E.zero_coefficient_case(which)
    st, _b, rt = _check_starts(gpu, [(p2, P, W)], E.WIDE_K, "p3p", what="coef[%d] == 0" % which)
    assert st.tolist() == [0]
    assert np.abs(po.rodrigues(rt[0, :3]) - R).max() < 1e-7 and np.abs(rt[0, 3:] - t).max() < 1e-7


@pytest.mark.parametrize("method,pn", [("dlt", 64), ("dlt", 65), ("dlt", 128), ("dlt", 4096), ("p3p", 64), ("p3p", 65)])
def test_start_around_the_lane_loop_equals_the_twin(pkg, gpu, method, pn):
    probs = E.lane_loop_problems(pn, method)
    if method == "dlt":                                          # as test_gpu_pose.py: 1e-7, no allowance
        rt, st = _device_start(gpu, probs, KMAT, "dlt")
        assert (st == 1).all()
        for i, (p2, P, W, _rt) in enumerate(probs):
            np.testing.assert_allclose(rt[i], twin_start(P, p2, W, KMAT, "dlt")[0], rtol=0, atol=1e-7, err_msg=str((pn, i)))
    else:
        st, _b, _rt = _check_starts(gpu, probs, KMAT, "p3p", what="pn %d" % pn)
        assert (st == 0).all(), st
