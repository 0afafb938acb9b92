"""The device pose with its start (include/pvnet_pose.h, clean_pvnet_amd.pose) -- what can be checked without a GPU: the C ABI
library exports what its header declares, refuses bad arguments before any launch, and the Python surface has the
reference's shapes.  The numbers are checked on the GPU in test_gpu_pose.py.  Below those: the host twins at the solver's
edges (the angle-axis conversion at half turns, every exit of the refinement, the start's rare branches), which keep the
inputs of test_gpu_pose_edges.py on the branches they were built for."""
import ctypes
import inspect
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import capi
from tests.test_pnp import need_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pvnet_pose.h")
_P = ctypes.c_void_p


def test_header_names_equal_the_library_exports():
    names = capi.declared("pose")
    assert names == {"pvp_initial_pose_batched", "pvp_pose_batched"}
    L = capi.load("pose")
    for n in names:
        assert hasattr(L, n)
    assert {e for e in capi.exported("pose") if e.startswith("pvp_")} == names      # every exported pvp_ symbol is declared


def test_status_and_method_codes_match_the_header(pkg):
    from clean_pvnet_amd import pose
    defs = dict(re.findall(r"#define\s+(PVP_\w+)\s+(-?\d+)", open(HDR).read()))
    assert {k: int(v) for k, v in defs.items() if k.startswith("PVP_START_")} == {"PVP_START_P3P": pose.METHODS["p3p"],
                                                                                   "PVP_START_DLT": pose.METHODS["dlt"]}
    assert sorted(int(v) for k, v in defs.items() if k.startswith("PVP_STATUS_")) == sorted(pose.STATUS)


def test_bad_arguments_are_refused_before_any_launch():
    L = capi.load("pose")
    buf = (ctypes.c_double * 64)()
    ibuf = (ctypes.c_int * 4)()
    d, i = ctypes.cast(buf, _P), ctypes.cast(ibuf, _P)
    # NULL pointers (host pointers elsewhere: a launch would fault, so -1 proves none happened)
    assert L.pvp_initial_pose_batched(None, None, None, None, 0, None, None, 1, 9, 0, 0, None) == -1
    assert L.pvp_initial_pose_batched(d, d, None, d, 0, d, i, 1, 9, 0, 0, None) == -1        # P3P needs the weights
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, None, 1, 9, 0, 0, None) == -1        # no status
    assert L.pvp_pose_batched(None, None, None, None, 1, None, None, None, None, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_pose_batched(d, d, None, d, 0, d, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_pose_batched(d, d, d, d, 1, None, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    # out of range: method, pn, B
    assert L.pvp_initial_pose_batched(d, d, d, d, 2, d, i, 1, 9, 0, 0, None) == -1
    assert L.pvp_pose_batched(d, d, d, d, -1, d, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    for pn in (3, 4097):
        assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, 1, pn, 0, 0, None) == -1
        assert L.pvp_pose_batched(d, d, d, d, 1, d, None, None, i, None, 1, pn, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, -1, 9, 0, 0, None) == -1
    # an empty batch is valid and launches nothing
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, 0, 9, 0, 0, None) == 0
    assert L.pvp_pose_batched(d, d, None, d, 1, d, None, None, i, None, 0, 9, 0, 0, 0, 0.0, None) == 0


def test_python_signatures(pkg):
    from clean_pvnet_amd import pose
    from clean_pvnet_amd.un_pnp_utils import uncertainty_pnp_batched
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    E = inspect.Parameter.empty
    assert sig(pose.initial_pose_batched) == [("points_2d", E), ("points_3d", E), ("camera_matrix", E), ("weights_2d", None),
                                              ("method", "p3p")]
    assert sig(pose.pnp_batched) == [("points_3d", E), ("points_2d", E), ("camera_matrix", E)]
    assert sig(pose.pnp) == [("points_3d", E), ("points_2d", E), ("camera_matrix", E), ("method", 0)]
    assert sig(pose.solve_pose) == [("output", E), ("kpt_3d", E), ("K", E), ("un_pnp", False)]
    assert dict(sig(uncertainty_pnp_batched))["init_rt"] is None
    from lib.csrc.uncertainty_pnp import un_pnp_utils as drop_in
    for n in ("initial_pose_batched", "pnp_batched", "pnp", "solve_pose"):
        assert getattr(drop_in, n) is getattr(pose, n)


def test_pnp_supports_only_the_iterative_method(pkg):
    from clean_pvnet_amd.pose import pnp
    P = np.random.RandomState(0).uniform(-0.05, 0.05, (9, 3))
    for method in (1, 2, 6):                                   # SOLVEPNP_EPNP, _P3P, _UPNP
        with pytest.raises(NotImplementedError):
            pnp(P, np.zeros((9, 2)), np.eye(3), method=method)


def test_p3p_twin_has_no_solution_for_a_collinear_triple(pkg):
    """The rotation about the line of a collinear object triple is undetermined; the twin (and the device) reject it
    rather than return an arbitrary one."""
    from clean_pvnet_amd.un_pnp_utils import p3p_depths
    P = np.array([[0.0, 0.0, 0.0], [0.04, 0.01, -0.02], [0.028, 0.007, -0.014]])
    f = np.array([[0.1, 0.05, 1.0], [0.12, 0.02, 1.0], [0.11, 0.04, 1.0]])
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    assert p3p_depths(f, P) == []


# ---------------------------------------------------------------------------------------- the solver's edges, on the CPU
def test_angle_axis_round_trip_at_half_turns_and_the_identity(pkg):
    """rodrigues -> rotation_to_angle_axis -> rodrigues returns the matrix it was given at every angle, the half turn and
    its neighbourhood included: to 1e-13 for an exactly rounded R, and to 1e-10 = 100 x the perturbation for R + E, E uniform
    in +-1e-12 (what any solver's R carries; the conversion's condition number is O(1)).  The acos / sin form this replaced
    missed both bounds from pi - 1e-4 on: 3e-8 at pi exactly rounded, 2.0 -- the identity -- at pi with the noise."""
    from clean_pvnet_amd.un_pnp_utils import rodrigues, rotation_to_angle_axis
    from tests import pose_edges as E
    rng = np.random.RandomState(7)
    worst = {False: 0.0, True: 0.0}
    for th in E.ROUND_TRIP_ANGLES:
        for a in E.round_trip_axes():
            R = rodrigues(a * th)
            for noisy in (False, True):
                Rn = R + rng.uniform(-1e-12, 1e-12, (3, 3)) if noisy else R
                w = rotation_to_angle_axis(Rn)
                assert np.isfinite(w).all(), (th, a, noisy)
                # |w| <= pi, the norm being itself a rounded sum (one ulp of pi is 2 eps pi)
                assert np.linalg.norm(w) <= np.pi * (1 + 2 * np.finfo(np.float64).eps), (th, a, noisy, w)
                err = float(np.abs(rodrigues(w) - Rn).max())
                worst[noisy] = max(worst[noisy], err)
                assert err <= (1e-10 if noisy else 1e-13), (th, a, noisy, err)
    print("\n[pose-edges] angle-axis round trip: %.3g exactly rounded, %.3g with 1e-12 noise" % (worst[False], worst[True]))


def test_angle_axis_of_a_half_turn_about_the_diagonal(pkg):
    """A half turn about (1,1,1)/sqrt 3, exactly symmetric, with its three diagonal entries equal: the axis times pi, up to
    the sign a half turn leaves open.  (Which of the equal rows is taken cannot be seen: they are the same row.)"""
    from clean_pvnet_amd.un_pnp_utils import rotation_to_angle_axis
    R = 2.0 / 3.0 * np.ones((3, 3)) - np.eye(3)               # 2 a a^T - I
    w = rotation_to_angle_axis(R)
    np.testing.assert_allclose(np.abs(w), np.pi / np.sqrt(3.0) * np.ones(3), rtol=0, atol=1e-15)
    assert (np.sign(w) == np.sign(w[0])).all()


def test_refinement_inputs_stay_on_their_branches():
    """The inputs of tests/test_gpu_pose_edges.py on the numpy twin: every termination code is reached, each case ends the way
    it was built to, the small-angle starts lie on the intended side of rotate_point's switch, and non-finite input leaves the
    start untouched after the radius has underflowed (14 halvings)."""
    from oracle import pnp_oracle as po
    from tests import pose_edges as E
    from tests.test_pnp import KMAT
    seen = set()
    for c in E.lm_cases() + E.batch_of_five() + E.nonfinite_cases():
        kw = {k: v for k, v in c["kw"].items() if k == "max_iterations"}
        with np.errstate(all="ignore"):
            x, info = po.solve_lm(c["init"], c["p2"], c["P"], c["W"], KMAT, **kw)
        seen.add(info["termination"])
        if c["expect"] is not None:
            assert info["termination"] == c["expect"], (c["name"], info)
        if c["expect"] == 4:
            assert info["iterations"] == 14 and np.array_equal(x, c["init"], equal_nan=True), (c["name"], info)
            assert np.isnan(info["initial_cost"]) and np.isnan(info["final_cost"]), (c["name"], info)
        elif c["name"] != "nan_init":
            assert np.isfinite(x).all(), c["name"]
        if c["name"] == "at_the_truth":                          # a decade inside the gradient tolerance: rounding cannot cross it
            r, J = po.residuals(c["init"], c["p2"], c["P"], c["W"], KMAT, True)
            assert np.abs(J.reshape(-1, 6).T @ r.reshape(-1)).max() <= 1e-11 and info["iterations"] == 0
        if c["name"].startswith("weighted_"):                    # rank-deficient: fewer than three weighted keypoints fix 6 parameters
            _r, J = po.residuals(c["init"], c["p2"], c["P"], c["W"], KMAT, True)
            assert np.linalg.matrix_rank(J.reshape(-1, 6)) == min(6, 2 * int(c["name"].split("_")[1]))
    assert seen == {0, 1, 2, 3, 4}, seen
    side = {c["name"]: float(c["init"][:3] @ c["init"][:3]) for c in E.lm_cases() if c["name"].startswith("w_")}
    assert side["w_zero"] == 0.0 and 0.0 < side["w_1e-9"] <= E.THETA2_SWITCH
    assert 0.8 * E.THETA2_SWITCH < side["w_below_switch"] <= E.THETA2_SWITCH < side["w_above_switch"] < 1.2 * E.THETA2_SWITCH
    c = E.inside_the_object()
    assert c["init"][5] == 0.03 and po.cost(c["init"], c["p2"], c["P"], c["W"], KMAT) > 1e8
    half = [c for c in E.lm_cases() if c["name"] == "across_half_turn"][0]
    assert abs(np.linalg.norm(half["init"][:3]) - (np.pi + 0.03)) < 1e-12


@need_ref
def test_reference_entry_point_fails_on_nonfinite_input_as_the_twin_does():
    """The reference's uncertainty_pnp() under the shim's Levenberg-Marquardt (oracle/ref_build_pnp.cpp) on the non-finite
    inputs: the start comes back, termination 4 after 14 iterations.  The shim's schedule is this project's restatement, so
    this pins the shim to the twin, not the twin to Ceres.  A library built before the shim stopped taking the gradient
    maximum with fmax answers termination 1 after 0 iterations here: rebuild it (make -C oracle -B _ref)."""
    from oracle import pnp_oracle as po
    from tests import pose_edges as E
    from tests.test_pnp import KMAT
    for c in E.nonfinite_cases():
        xr, ir = po.ref_solve(c["init"], c["p2"], c["P"], c["W"], KMAT)
        assert np.array_equal(xr, c["init"], equal_nan=True), c["name"]
        assert (ir["termination"], ir["iterations"]) == (4, 14) and np.isnan(ir["final_cost"]), (c["name"], ir)


def test_start_inputs_stay_on_their_branches(pkg):
    """The start kernel's edge inputs on the host twins: the six-best path is taken (fewer than six positive keys, P3P without a
    solution), and Grunert's quartic really has the exactly zero leading / trailing coefficient."""
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt, initial_pose_p3p
    from tests import pose_edges as E
    from tests.pose_edges import pose_distance, twin_uncertainty
    from tests.test_pnp import KMAT
    for p2, P, W, rt in E.six_path_cases():
        key = W[:, 0] + W[:, 1]
        dkey = np.clip(np.where(np.isfinite(key), key, 0.0), 0.0, None)      # initial_pose_dlt's key
        assert (dkey > 0).sum() == 4 < 6
        zeros = dkey == 0
        assert zeros.sum() >= 5 and np.isnan(key).any() and np.isposinf(key).any() and (key < 0).any() and (key == 0).sum() >= 2
        rank = np.argsort(np.argsort(np.where(np.isfinite(key), key, -np.inf), kind="stable"), kind="stable").astype(np.float64)
        assert initial_pose_p3p(P, p2, KMAT, rank) is None
        # the comparison keeps its teeth: the zeros taken from the other end move the start by more than its bound
        with np.errstate(all="ignore"):
            want = initial_pose_dlt(P, p2, KMAT, order_key=key)
            other = initial_pose_dlt(P[::-1], p2[::-1], KMAT, order_key=key[::-1])
        bound = max(1e-7, 1e2 * twin_uncertainty(P, p2, W, KMAT, "p3p", want, raw=True))
        assert bound <= 1e-5 and np.abs(other - want).max() > 1e2 * bound, (bound, np.abs(other - want).max())
        assert pose_distance(want, rt) <= 0.02                   # 1e-3 px of noise: the six-best start is still a pose
    for which in (0, 4):
        p2, P, W, R, t = E.zero_coefficient_case(which)
        order = np.argsort(W[:, 0] + W[:, 1])[-4:]
        assert list(order[:3]) == [0, 1, 2]
        n = (np.linalg.inv(E.WIDE_K) @ np.concatenate([p2[:3], np.ones((3, 1))], 1).T).T
        f = n / np.linalg.norm(n, axis=1, keepdims=True)
        coef = E.p3p_coefficients(P[:3], f)
        ends = {0: (1, 2), 4: (0, 1)}[which]                     # their dot product is 0.5 however it is evaluated:
        C, D = [Fraction(x) for x in f[ends[0]]], [Fraction(x) for x in f[ends[1]]]
        for i, j, k in itertools.permutations(range(3)):
            unfused = float(Fraction(float(Fraction(float(C[i] * D[i])) + Fraction(float(C[j] * D[j])))) + Fraction(float(C[k] * D[k])))
            fused = float(C[k] * D[k] + Fraction(float(C[j] * D[j] + Fraction(float(C[i] * D[i])))))   # one product rounded, two fused
            assert unfused == 0.5 and fused == 0.5, (which, i, j, k, unfused, fused)
        assert coef[which] == 0.0 and (coef[[k for k in range(5) if k != which]] != 0.0).all(), coef
        rt = initial_pose_p3p(P, p2, E.WIDE_K, W[:, 0] + W[:, 1])
        assert rt is not None                                    # and the twin recovers the pose the pixels came from
        from clean_pvnet_amd.un_pnp_utils import rodrigues
        assert np.abs(rodrigues(rt[:3]) - R).max() < 1e-9 and np.abs(rt[3:] - t).max() < 1e-9


def test_twin_starts_are_well_determined_at_half_turns_and_the_identity(pkg):
    """The noise-free instances of the GPU half-turn test on the host twins alone: both starts, each computed two ways (np.roots
    on the reversed quartic; the DLT's null vector from eigh(A^T A)), agree with each other and with the true pose to 1e-8 as
    (R, t) at every angle from 0 to pi -- so the GPU test's bound, 100 x the disagreement, stays below 1e-6.  With the acos / sin
    conversion the two routes disagreed by 4.4e-4 at pi - 2e-6."""
    from tests import pose_edges as E
    from tests.pose_edges import pose_distance, twin_start, twin_uncertainty
    from tests.test_pnp import KMAT
    worst = {"dlt": 0.0, "p3p": 0.0}
    for th in E.START_ANGLES:
        for p2, P, W, rt in E.half_turn_starts(th):
            for method in ("dlt", "p3p"):
                want, status = twin_start(P, p2, W, KMAT, method)
                assert status == (1 if method == "dlt" else 0) and np.isfinite(want).all()
                d = max(twin_uncertainty(P, p2, W, KMAT, method, want), pose_distance(want, rt))
                worst[method] = max(worst[method], d)
                assert d <= 1e-8, (th, method, d)
    print("\n[pose-edges] twin starts at half turns, two routes and the truth: dlt %.3g, p3p %.3g" % (worst["dlt"], worst["p3p"]))
