"""The device pose with its start (include/pvnet_pose.h, clean_pvnet_amd.pose) against its host twins on the MI355X:
the P3P and DLT starts equal un_pnp_utils.initial_pose_p3p / initial_pose_dlt, the refinement from the device start reaches
the minimum an independent minimiser (scipy / MINPACK) finds, and network output -> pose runs with no start supplied and no
host synchronisation."""
import numpy as np
import pytest

from oracle import pnp_oracle as po
from tests.test_pnp import KMAT, problem, wide_problems

pytestmark = pytest.mark.gpu

CASES = [(s, pn, noise) for s, (pn, noise) in enumerate((pn, n) for pn in (4, 5, 9, 17, 70) for n in (0.0, 0.3, 1.0, 3.0))]


def _key(W):
    return W[:, 0] + W[:, 1]


def _stable_rank(key):
    """A key with the device's tie rule made explicit: initial_pose_p3p's argsort(key)[-4:] then selects as a stable sort."""
    k = np.where(np.isfinite(key), key, -np.inf)
    return np.argsort(np.argsort(k, kind="stable"), kind="stable").astype(np.float64)


def _twin_start(P, p2, W):
    """(rt, status) of the host twins, as the device defines them."""
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt, initial_pose_p3p
    key = _key(W)
    rt = initial_pose_p3p(P, p2, KMAT, _stable_rank(key))
    if rt is not None:
        return rt, 0
    if P.shape[0] < 6:
        return None, -1
    return initial_pose_dlt(P, p2, KMAT, order_key=key), 2


def _batch(gpu, arrays):
    import torch
    return torch.tensor(np.stack(arrays), dtype=torch.float64, device=gpu)


def _device_start(gpu, probs, method):
    import torch
    from clean_pvnet_amd.pose import initial_pose_batched
    rt, st = initial_pose_batched(_batch(gpu, [q[0] for q in probs]), _batch(gpu, [q[1] for q in probs]),
                                  torch.tensor(KMAT, device=gpu), _batch(gpu, [q[2] for q in probs]), method=method)
    return rt.cpu().numpy(), st.cpu().numpy()


def _start_tolerance(P, p2, W, want):
    """1e-7, or 100 x the twin's own rounding uncertainty.  Near a double root of Grunert's quartic the root is determined
    to ~1e-9 in binary64 whatever the solver, and the start, through it, to ~1e-5: two correct implementations differ there
    by more than 1e-7.  The uncertainty is measured by solving the same quartic a second way (np.roots of the reversed
    polynomial, roots inverted) and comparing the twin's two starts."""
    from unittest import mock
    roots = np.roots

    def reversed_roots(c):
        r = roots(np.asarray(c)[::-1])
        return 1.0 / r[r != 0]
    with mock.patch.object(np, "roots", reversed_roots):
        other, _ = _twin_start(P, p2, W)
    if other is None or want is None:
        return 1e-7
    return max(1e-7, 1e2 * float(np.abs(other - want).max()))


def _check_starts(gpu, probs):
    rt, st = _device_start(gpu, probs, "p3p")
    loose = []
    for i, (p2, P, W) in enumerate(probs):
        want, status = _twin_start(P, p2, W)
        assert st[i] == status, (i, st[i], status)
        if want is None:
            assert np.isnan(rt[i]).all()
        else:
            tol = _start_tolerance(P, p2, W, want)
            if tol > 1e-7:
                loose.append((i, tol))
            np.testing.assert_allclose(rt[i], want, rtol=0, atol=tol, err_msg=str(i))
    assert len(loose) <= max(2, 0.25 * len(probs)), loose     # ill-conditioned starts stay the exception
    if loose:
        print("\n[pose] ill-conditioned P3P starts (index, bound):", loose)
    return st


def test_p3p_start_equals_the_host_twin(pkg, gpu):
    for pn in (4, 5, 9, 17, 70):
        probs = [problem(s, pn=pn, noise=n)[:3] for s, p, n in CASES if p == pn]
        st = _check_starts(gpu, probs)
        assert (st == 0).all(), (pn, st)                        # a real start on every ordinary instance


def _edge_cases():
    """Key ties, a NaN key, collinear triples, a fourth keypoint behind the camera -- at 4, 5, 9 and 17 keypoints."""
    out = []
    for s in range(4):
        for pn in (4, 5, 9, 17):
            p2, P, W, rt, _ = problem(100 + 10 * s + pn, pn=pn, noise=0.5)
            key = _key(W)
            order = np.argsort(key, kind="stable")
            t = W.copy()                                         # ties: the five best keys equal
            t[order[-min(5, pn):], 0] = 1.0
            t[order[-min(5, pn):], 1] = 0.25
            out.append((p2, P, t))
            n = W.copy()                                         # the best key NaN
            n[order[-1], 1] = np.nan
            out.append((p2, P, n))
            c, c2 = P.copy(), p2.copy()                          # the first three selected keypoints collinear
            j = order[-4:]
            c[j[2]] = 0.3 * c[j[0]] + 0.7 * c[j[1]]
            X = po.angle_axis_rotate_point(rt[:3], c[j[2]]) + rt[3:]
            c2[j[2]] = [KMAT[0, 0] * X[0] / X[2] + KMAT[0, 2], KMAT[1, 1] * X[1] / X[2] + KMAT[1, 2]]
            out.append((c2, c, W))
            b = P.copy()                                         # the fourth (best-keyed) keypoint behind the camera
            R = po.rodrigues(rt[:3])
            b[order[-1]] = R.T @ (np.array([0.05, 0.02, -0.3]) - rt[3:])
            out.append((p2, b, W))
    return out


def test_p3p_start_edge_cases_follow_the_twin(pkg, gpu):
    probs = _edge_cases()
    for pn in (4, 5, 9, 17):
        grp = [q for q in probs if q[1].shape[0] == pn]
        st = _check_starts(gpu, grp)
        kinds = st.reshape(-1, 4)                                # per seed: ties, NaN, collinear, behind
        assert (kinds[:, 2] == (2 if pn >= 6 else -1)).all(), kinds   # collinear: never a P3P start
        # behind: the true pose is skipped; another P3P solution may keep the point in front (status as the twin's, above)


def test_dlt_start_equals_the_host_twin(pkg, gpu):
    import torch
    from clean_pvnet_amd.pose import initial_pose_batched
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt
    for pn in (9, 17, 70, 300):
        probs = [problem(s, pn=pn, noise=n)[:3] for s, n in enumerate((0.0, 0.3, 1.0, 3.0, 1.0, 2.0))]
        rt, st = _device_start(gpu, probs, "dlt")
        assert (st == 1).all()
        for i, (p2, P, W) in enumerate(probs):
            np.testing.assert_allclose(rt[i], initial_pose_dlt(P, p2, KMAT), rtol=0, atol=1e-7, err_msg=str((pn, i)))
    for pn in (4, 5):                                            # too few keypoints: no start
        p2, P, W, _, _ = problem(pn, pn=pn)
        rt, st = initial_pose_batched(_batch(gpu, [p2]), torch.tensor(P, device=gpu), torch.tensor(KMAT, device=gpu), method="dlt")
        assert st.cpu().tolist() == [-1] and torch.isnan(rt).all()
    p2, P, W, _, _ = problem(7, pn=9)                            # a planar model
    P[:, 2] = 0.0
    rt, st = initial_pose_batched(_batch(gpu, [p2]), torch.tensor(P, device=gpu), torch.tensor(KMAT, device=gpu), method="dlt")
    assert st.cpu().tolist() == [-2] and torch.isnan(rt).all()


def _same_minimum(x, xs, p2, P, W, what):
    """test_pnp.py's rule: cost within 1e-9 relative, pose within 1e-6 (1e-4 in an ill-conditioned valley, cond > 1e8).
    Costs below 1e-12 (noise-free instances, where a valley's floor is rounding) do not decide: the pose does."""
    c, cs = po.cost(x, p2, P, W, KMAT), po.cost(xs, p2, P, W, KMAT)
    assert abs(c - cs) <= 1e-9 * cs + 1e-12, (what, c, cs)
    _r, J = po.residuals(xs, p2, P, W, KMAT, True)
    cond = float(np.linalg.cond(J.reshape(-1, 6).T @ J.reshape(-1, 6)))
    d = max(float(np.abs(po.rodrigues(x[:3]) - po.rodrigues(xs[:3])).max()), float(np.abs(x[3:] - xs[3:]).max()))
    assert d <= (1e-6 if cond <= 1e8 else 1e-4), (what, d, cond)


def test_uncertainty_pnp_batched_without_a_start_reaches_the_minimum(pkg, gpu):
    import torch
    from clean_pvnet_amd.un_pnp_utils import initial_pose_p3p, uncertainty_pnp_batched
    probs = wide_problems()
    other, checked, no_start = 0, 0, 0
    for pn in (4, 5, 9, 17):
        grp = [q for q in probs if q["pn"] == pn]
        t = lambda k: _batch(gpu, [g[k] for g in grp])          # noqa: E731
        Kt = torch.tensor(KMAT, device=gpu)
        rt = uncertainty_pnp_batched(t("p2"), t("W"), t("P"), Kt, None, max_iterations=200, function_tolerance=1e-15).cpu().numpy()
        starts = [_twin_start(g["P"], g["p2"], g["W"])[0] for g in grp]
        have = [i for i, s in enumerate(starts) if s is not None]
        rt_host = np.full_like(rt, np.nan)
        if have:
            rt_host[have] = uncertainty_pnp_batched(_batch(gpu, [grp[i]["p2"] for i in have]), _batch(gpu, [grp[i]["W"] for i in have]),
                                                    _batch(gpu, [grp[i]["P"] for i in have]), Kt, _batch(gpu, [starts[i] for i in have]),
                                                    max_iterations=200, function_tolerance=1e-15).cpu().numpy()
        for i, g in enumerate(grp):
            if starts[i] is None:                                # the host twin has no start either
                assert np.isnan(rt[i]).all(), (pn, i)
                no_start += 1
                continue
            if pn == 4:                                          # the P3P pose, unrefined (un_pnp_utils.py:34-38)
                want = initial_pose_p3p(g["P"], g["p2"], KMAT, _stable_rank(_key(g["W"])))
                np.testing.assert_allclose(rt[i], want, rtol=0, atol=_start_tolerance(g["P"], g["p2"], g["W"], want))
                continue
            _same_minimum(rt[i], rt_host[i], g["p2"], g["P"], g["W"], ("host start", pn, i))
            xs, _ = po.solve_scipy(starts[i], g["p2"], g["P"], g["W"], KMAT)
            if max(float(np.abs(po.rodrigues(rt[i, :3]) - po.rodrigues(xs[:3])).max()), float(np.abs(rt[i, 3:] - xs[3:]).max())) > 1e-3:
                other += 1                                       # scipy ended in another local minimum from the same start
                continue
            _same_minimum(rt[i], xs, g["p2"], g["P"], g["W"], ("scipy", pn, i))
            checked += 1
    print("\n[pose] wide set: %d at the scipy minimum, %d in another basin, %d without a start" % (checked, other, no_start))
    assert other <= 0.03 * len(probs) and checked >= 0.5 * len(probs)


def test_pnp_batched_reaches_the_unweighted_minimum(pkg, gpu):
    import torch
    from clean_pvnet_amd.pose import pnp, pnp_batched, pose_batched
    from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt
    for pn in (9, 17, 70):
        probs = [problem(s, pn=pn, noise=n) for s, n in enumerate((0.0, 0.3, 1.0, 3.0))]
        p2, P = _batch(gpu, [q[0] for q in probs]), _batch(gpu, [q[1] for q in probs])
        Kt = torch.tensor(KMAT, device=gpu)
        Rt = pnp_batched(P, p2, Kt).cpu().numpy()
        out = pose_batched(p2, P, Kt, max_iterations=200, function_tolerance=1e-15)
        rt, st = out["rt"].cpu().numpy(), out["status"].cpu().numpy()
        assert (st == 1).all()
        for i, (q2, qP, _W, rt_true, _) in enumerate(probs):
            one = np.tile([1.0, 0.0, 1.0], (pn, 1))
            xs, _ = po.solve_scipy(initial_pose_dlt(qP, q2, KMAT), q2, qP, one, KMAT)
            _same_minimum(rt[i], xs, q2, qP, one, ("pnp", pn, i))
            np.testing.assert_allclose(Rt[i, :, :3], po.rodrigues(xs[:3]), atol=1e-5)
            np.testing.assert_allclose(Rt[i, :, 3], xs[3:], atol=1e-5)
            if i == 0:                                           # noise-free: the true pose
                np.testing.assert_allclose(Rt[i, :, :3], po.rodrigues(rt_true[:3]), rtol=0, atol=1e-9)
                np.testing.assert_allclose(Rt[i, :, 3], rt_true[3:], rtol=0, atol=1e-9)
                host = pnp(qP, q2, KMAT)                         # the drop-in: numpy in, [3,4] out
                assert host.shape == (3, 4)
                np.testing.assert_allclose(host, Rt[i], rtol=0, atol=1e-12)


def _rendered_fields(gpu):
    """Synthetic network output as in test_pnp.test_gpu_pose_from_voted_keypoints_end_to_end."""
    import torch
    B, H, W, K = 4, 240, 320, 9
    rng = np.random.RandomState(5)
    P = rng.uniform(-0.05, 0.05, (K, 3))
    Kc = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1.0]])
    rts = np.stack([np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.03, 0.03, 2), rng.uniform(0.5, 0.7, 1)]) for _ in range(B)])
    kpts = []
    for rt in rts:
        X = np.array([po.angle_axis_rotate_point(rt[:3], p) for p in P]) + rt[3:]
        kpts.append(np.stack([Kc[0, 0] * X[:, 0] / X[:, 2] + Kc[0, 2], Kc[1, 1] * X[:, 1] / X[:, 2] + Kc[1, 2]], 1))
    kpts = torch.tensor(np.stack(kpts), dtype=torch.float32)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    x = torch.zeros(B, 2 + 2 * K, H, W)
    for b in range(B):
        c = kpts[b].mean(0)
        m = ((xs - c[0]) ** 2 + (ys - c[1]) ** 2) <= 30.0 ** 2
        x[b, 0] = 1.0
        x[b, 1] = torch.where(m, torch.tensor(4.0), torch.tensor(-4.0))
        g = torch.Generator().manual_seed(b)
        for k in range(K):
            dx, dy = kpts[b, k, 0] - xs, kpts[b, k, 1] - ys
            n = torch.sqrt(dx * dx + dy * dy).clamp(min=1e-3)
            x[b, 2 + 2 * k] = dx / n + 0.03 * torch.randn(H, W, generator=g)
            x[b, 3 + 2 * k] = dy / n + 0.03 * torch.randn(H, W, generator=g)
    return x.to(gpu), P, Kc, rts


def test_network_output_to_pose_with_no_start_and_no_host_sync(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.pose import solve_pose
    x, P, Kc, rts = _rendered_fields(gpu)
    Pt, Kt = torch.tensor(P, device=gpu), torch.tensor(Kc, device=gpu)
    torch.cuda.synchronize()
    poses = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        for un_pnp in (True, False):
            o = {"seg": x[:, :2], "vertex": x[:, 2:]}
            decode_keypoint(o, un_pnp=un_pnp, weights=un_pnp, seed=3)
            solve_pose(o, Pt, Kt, un_pnp=un_pnp)
            poses[un_pnp] = (o["pose"], o["pose_status"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for un_pnp, (pose, status) in poses.items():
        pose, status = pose.cpu().numpy(), status.cpu().numpy()
        assert pose.shape == (len(rts), 3, 4) and pose.dtype == np.float64
        assert (status == (0 if un_pnp else 1)).all(), (un_pnp, status)
        for b, rt in enumerate(rts):
            R_err = np.abs(pose[b, :, :3] - po.rodrigues(rt[:3])).max()
            assert R_err < 0.05 and np.abs(pose[b, :, 3] - rt[3:]).max() < 0.03, (un_pnp, b, R_err, pose[b], rt)


def test_batch_layouts_failures_and_determinism(pkg, gpu):
    import torch
    from clean_pvnet_amd.pose import initial_pose_batched, pose_batched
    probs = [problem(s, pn=9, noise=1.0) for s in range(6)]
    p2 = _batch(gpu, [q[0] for q in probs])
    W = _batch(gpu, [q[2] for q in probs])
    P_each = _batch(gpu, [q[1] for q in probs])
    K_each = _batch(gpu, [KMAT * np.array([[1.0 + 0.01 * i] * 3, [1.0 + 0.01 * i] * 3, [1.0] * 3]) for i in range(6)])
    for method, w in (("p3p", W), ("dlt", None)):
        a = pose_batched(p2, P_each, K_each, weights_2d=w, method=method)
        for i in range(6):                                       # batched pts3d / K == one image at a time
            one = pose_batched(p2[i:i + 1], P_each[i], K_each[i], weights_2d=None if w is None else w[i:i + 1], method=method)
            for k in ("rt", "Rt", "status"):
                assert torch.equal(a[k][i:i + 1], one[k]), (method, i, k)
        b = pose_batched(p2, P_each, K_each, weights_2d=w, method=method)
        for k in a:                                              # two identical calls: the same bits
            assert torch.equal(torch.nan_to_num(a[k], nan=7.0), torch.nan_to_num(b[k], nan=7.0)), (method, k)
    # one shared model and camera for the batch
    Ps = torch.tensor(probs[0][1], device=gpu)
    shared = pose_batched(p2[:1].expand(3, -1, -1).contiguous(), Ps, torch.tensor(KMAT, device=gpu))
    assert torch.equal(shared["Rt"][0], shared["Rt"][2]) and (shared["status"] == 1).all()
    # mixed failing and good images: a non-finite keypoint, a planar model
    bad_p2, bad_P = p2.clone(), P_each.clone()
    bad_p2[1, 3, 0] = float("nan")
    bad_P[3, :, 2] = 0.0
    good = pose_batched(p2, P_each, K_each)
    mixed = pose_batched(bad_p2, bad_P, K_each)
    assert mixed["status"].cpu().tolist() == [1, -3, 1, -2, 1, 1]
    for i in (0, 2, 4, 5):
        assert torch.equal(mixed["Rt"][i], good["Rt"][i])
    for i in (1, 3):
        assert torch.isnan(mixed["Rt"][i]).all() and torch.isnan(mixed["rt"][i]).all()
    # an empty batch
    rt, st = initial_pose_batched(p2[:0], P_each[:0], K_each[:0], W[:0])
    assert rt.shape == (0, 6) and st.shape == (0,)
    assert pose_batched(p2[:0], Ps, torch.tensor(KMAT, device=gpu))["Rt"].shape == (0, 3, 4)
