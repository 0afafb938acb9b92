"""The batched depth rasteriser and VSD on the MI355X (include/pvnet_vsd.h, clean_pvnet_amd.vsd): the renders equal the numpy
twin as float32 bit patterns (tests/vsd_twin.py, itself held to an independent ray caster in tests/test_vsd.py), the errors
equal the fixtures made by the reference's own functions, determinism, the evaluator's bookkeeping with bad input, and
network output -> pose -> VSD with no host synchronisation.  The one bound ('tlinear') is derived in tests/vsd_twin.py."""
import os

import numpy as np
import pytest

from oracle import pnp_oracle as po
from tests import vsd_twin as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("vsd_720", "vsd_360", "vsd_near")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _t(gpu, a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=gpu)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(gpu, name):
    import torch
    c = load(name)
    r = twin.regenerate(name, c)
    t = {"pts": _t(gpu, r["pts"]), "faces": _t(gpu, r["faces"]), "K": _t(gpu, c["K"]), "pose_est": _t(gpu, c["pose_est"]),
         "pose_gt": _t(gpu, c["pose_gt"]), "raw": torch.from_numpy(r["raw"]).to(gpu)}
    kw = dict(delta=float(c["delta"]), tau=float(c["tau"]), depth_scale=float(c["depth_scale"]), t_scale=float(c["t_scale"]),
              near=float(c["near"]), far=float(c["far"]))
    return c, r, t, kw


# ----------------------------------------------------------------------------------------------------- 1. the renders, bit exact
@pytest.mark.parametrize("name", FIXTURES)
def test_render_depth_equals_the_twin_bit_for_bit(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.vsd import render_depth
    c, r, t, kw = _inputs(gpu, name)
    ts, near, far = kw["t_scale"], kw["near"], kw["far"]
    poses = np.concatenate([twin.scaled(c["pose_est"], ts).reshape(-1, 3, 4), twin.scaled(c["pose_gt"], ts).reshape(-1, 3, 4)])
    want = np.concatenate([r["est"].reshape((-1,) + r["est"].shape[2:]), r["gt"].reshape((-1,) + r["gt"].shape[2:])])
    batch = render_depth(t["pts"], t["faces"], _t(gpu, poses), t["K"], r["size"], near, far)
    assert batch.dtype == torch.float32 and tuple(batch.shape) == want.shape
    got = batch.cpu().numpy()
    for i in range(len(poses)):
        diff = int((_bits(got[i]) != _bits(want[i])).sum())
        print("%s pose %d: covered %d, samples with other bits %d" % (name, i, int((want[i] > 0).sum()), diff))
        assert diff == 0
        one = render_depth(t["pts"], t["faces"], _t(gpu, poses[i:i + 1]), t["K"], r["size"], near, far)      # P = 1
        assert torch.equal(one[0], batch[i])                                                             # independent of P
    # a camera per pose (skew included): each image equals the twin's with that camera
    Ks = np.stack([twin.camera(c["K"][0, 0] / twin.TLESS_K[0, 0] * (1 + 0.02 * i), skew=0.3 * i) for i in range(len(poses))])
    Ks[:, 0, 2], Ks[:, 1, 2] = c["K"][0, 2] + np.arange(len(poses)), c["K"][1, 2] - np.arange(len(poses))
    got = render_depth(t["pts"], t["faces"], _t(gpu, poses), _t(gpu, Ks), r["size"], near, far).cpu().numpy()
    for i in (0, len(poses) - 1):
        w = twin.render_depth(r["pts"], r["faces"], poses[i], Ks[i], r["size"], near, far)
        assert (w > 0).any() or not (want[i] > 0).any()
        assert int((_bits(got[i]) != _bits(w)).sum()) == 0, (name, i)
    assert tuple(render_depth(t["pts"], t["faces"], _t(gpu, poses[:0]), t["K"], r["size"]).shape) == (0, r["size"][1], r["size"][0])


# --------------------------------------------------------------------------------------- 2. and 3. the errors, twice the same bits
@pytest.mark.parametrize("name", FIXTURES)
def test_vsd_equals_the_reference_fixture_and_is_deterministic(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.vsd import vsd
    c, r, t, kw = _inputs(gpu, name)
    args = (t["pose_est"], t["pose_gt"], t["raw"], t["K"], t["pts"], t["faces"])
    e, im = vsd(*args, cost="step", return_images=True, **kw)
    assert e.dtype == torch.float64 and tuple(e.shape) == c["e_step"].shape
    counts = np.stack([im[k].cpu().numpy() for k in ("union", "inter", "cost")], -1)
    print(name, "counts", counts.tolist(), "e", e.cpu().numpy().tolist())
    np.testing.assert_array_equal(_bits(im["depth_est"].cpu().numpy()), _bits(r["est"]))
    np.testing.assert_array_equal(_bits(im["depth_gt"].cpu().numpy()), _bits(r["gt"]))
    np.testing.assert_array_equal(counts, c["counts"])
    np.testing.assert_array_equal(e.cpu().numpy().view(np.uint64), c["e_step"].view(np.uint64))          # bit for bit
    tl, im_tl = vsd(*args, cost="tlinear", return_images=True, **kw)
    np.testing.assert_array_equal(np.stack([im_tl[k].cpu().numpy() for k in ("union", "inter", "cost")], -1), c["counts"])
    got = tl.cpu().numpy()
    for idx in np.ndindex(*got.shape):
        want = float(c["e_tlinear"][idx])
        bound = twin.tlinear_bound(want, int(c["counts"][idx][1]), float(c["cost_sum"][idx]), int(c["counts"][idx][0]))
        print("%s%s tlinear got %.17g want %.17g |diff| %.3g bound %.3g" % (name, list(idx), got[idx], want,
                                                                          abs(got[idx] - want), bound))
        assert abs(got[idx] - want) <= bound
        i, a, b = idx                                                    # and the device equals the twin's fixed order exactly
        tw = twin.vsd_pair(r["est"][i, a], r["gt"][i, b], twin.sensor_depth(r["raw"][i], kw["depth_scale"]), c["K"],
                           kw["delta"], kw["tau"], "tlinear")
        assert got[idx] == tw["e"], (name, idx)
    # twice: identical bits (integer atomics and a minimum: nothing may depend on the order of execution)
    e2, im2 = vsd(*args, cost="step", return_images=True, **kw)
    tl2 = vsd(*args, cost="tlinear", **kw)
    assert torch.equal(e, e2) and torch.equal(tl, tl2)
    assert torch.equal(im["depth_est"].view(torch.int32), im2["depth_est"].view(torch.int32))
    assert torch.equal(im["depth_gt"].view(torch.int32), im2["depth_gt"].view(torch.int32))
    assert all(torch.equal(im[k], im2[k]) for k in ("union", "inter", "cost"))
    # the sensor image already in model units, binary64, and a camera per image: the same bits
    n = e.shape[0]
    mm = _t(gpu, twin.sensor_depth(r["raw"], kw["depth_scale"]))
    e3 = vsd(t["pose_est"], t["pose_gt"], mm, t["K"][None].repeat(n, 1, 1), t["pts"], t["faces"], cost="step",
             **dict(kw, depth_scale=1.0))
    assert torch.equal(e, e3)
    # padded ground-truth slots
    valid = torch.ones(e.shape[0], e.shape[2], dtype=torch.bool, device=gpu)
    valid[0, -1] = False
    em = vsd(*args, cost="step", gt_valid=valid, **kw)
    assert bool(torch.isnan(em[0, :, -1]).all()) and torch.equal(em[0, :, :-1], e[0, :, :-1]) and torch.equal(em[1:], e[1:])


# ------------------------------------------------------------------------------------------------- 4. the evaluator, bad input
def test_evaluator_over_batches_any_pair_rule_and_bad_input(pkg, gpu):
    import torch
    from clean_pvnet_amd.vsd import VsdEvaluator, render_depth
    c, r, t, kw = _inputs(gpu, "vsd_360")
    thresh = float(c["error_thresh"])
    want = [twin.any_pair_hit(c["e_step"][i], thresh) for i in range(2)]
    assert want == [True, True]
    ev = VsdEvaluator(r["pts"], r["faces"], r["size"], error_thresh=thresh, device=gpu)
    for i in range(2):                                                   # one image per call
        h = ev.evaluate(t["pose_est"][i:i + 1], t["pose_gt"][i:i + 1], t["raw"][i:i + 1], t["K"])
        assert h.cpu().tolist() == [want[i]]
        np.testing.assert_array_equal(ev.last["e"].cpu().numpy().view(np.uint64), c["e_step"][i:i + 1].view(np.uint64))
    # the second predictions alone against the first ground truths alone: no pair below the threshold
    none = [twin.any_pair_hit(c["e_step"][i, 1:, :1], thresh) for i in range(2)]
    h = ev.evaluate(t["pose_est"][:, 1:], t["pose_gt"][:, :1], t["raw"], t["K"])
    assert h.cpu().tolist() == none == [False, False]
    # masked slots: image 0 keeps only its second ground truth, image 1 only its first
    valid = _t(gpu, [[False, True], [True, False]])
    masked = [twin.any_pair_hit(c["e_step"][i], thresh, gt_valid=valid[i].cpu().numpy()) for i in range(2)]
    h = ev.evaluate(t["pose_est"], t["pose_gt"], t["raw"], t["K"], gt_valid=valid)
    assert h.cpu().tolist() == masked
    # a NaN pose is a miss and does not disturb the other pairs
    bad = t["pose_est"].clone()
    bad[0, 1, 2, 1] = float("nan")                                       # image 0 loses its good pair (1, 1): e[0,0,0] stays
    h = ev.evaluate(bad, t["pose_gt"], t["raw"], t["K"])
    eb = ev.last["e"].cpu().numpy()
    assert (eb[0, 1] == 1.0).all() and np.array_equal(eb[0, 0], c["e_step"][0, 0]) and np.array_equal(eb[1], c["e_step"][1])
    nan_hits = [twin.any_pair_hit(eb[i], thresh) for i in range(2)]
    assert h.cpu().tolist() == nan_hits
    img = render_depth(t["pts"], t["faces"], twin_scaled_t(bad[0], kw["t_scale"]), t["K"], r["size"])
    assert not bool(img[1].any()) and bool(img[0].any())                 # an all-zero image, its neighbour untouched
    total = sum(want) + sum(none) + sum(masked) + sum(nan_hits)
    s = ev.summarize()
    assert s == {"vsd": total / 8.0}                                  # 1 + 1 + 2 + 2 + 2 images
    assert np.isnan(ev.summarize()["vsd"])                               # summarize() starts the counters again
    ev.evaluate(t["pose_est"][:1], t["pose_gt"][:1], t["raw"][:1], t["K"])
    assert ev.summarize(n_images=4) == {"vsd": 0.25}                     # the T-LESS denominator: len(gt_img_ids)
    # a face row with an index out of range is skipped: the same renders, no fault
    faces = torch.cat([t["faces"], _t(gpu, [[0, 1, len(r["pts"])], [-1, 2, 3], [2 ** 30, 0, 1]], dtype=torch.int32)])
    ev2 = VsdEvaluator(r["pts"], faces, r["size"], error_thresh=thresh, device=gpu)
    h = ev2.evaluate(t["pose_est"], t["pose_gt"], t["raw"], t["K"])
    np.testing.assert_array_equal(ev2.last["e"].cpu().numpy().view(np.uint64), c["e_step"].view(np.uint64))
    assert h.cpu().tolist() == want


def twin_scaled_t(pose, t_scale):
    import torch
    return torch.cat([pose[:, :, :3], pose[:, :, 3:] * t_scale], 2)


# ---------------------------------------------------------------------------------------------------- 5. end to end, no sync
def _rendered_fields(gpu):
    """Synthetic network output as in test_gpu_pose._rendered_fields."""
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


def test_network_output_to_vsd_with_no_host_sync(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.pose import solve_pose
    from clean_pvnet_amd.vsd import VsdEvaluator
    x, P, Kc, rts = _rendered_fields(gpu)
    pts, faces = twin.mesh(9)                                            # millimetres; the poses are in metres
    size = (320, 240)
    gt = np.stack([np.concatenate([po.rodrigues(rt[:3]), rt[3:].reshape(3, 1)], 1) for rt in rts])
    gt_renders = twin.render_batch(pts, faces, twin.scaled(gt, 1000.0), Kc, size)
    raw = np.stack([twin.scene_depth(90 + i, gt_renders[i:i + 1]) for i in range(len(gt))])
    Pt, Kt, Gt, Rt = _t(gpu, P), _t(gpu, Kc), _t(gpu, gt), torch.from_numpy(raw).to(gpu)
    ev = VsdEvaluator(pts, faces, size, device=gpu)
    seen = {}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for un_pnp in (True, False):
            o = {"seg": x[:, :2], "vertex": x[:, 2:]}
            decode_keypoint(o, un_pnp=un_pnp, weights=un_pnp, seed=3)
            solve_pose(o, Pt, Kt, un_pnp=un_pnp)
            ev.evaluate(o["pose"][:, None], Gt[:, None], Rt, Kt)
            seen[un_pnp] = (o["pose"], ev.last)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = ev.summarize()                                                   # the one read-back: 8 images
    print("summarize:", s)
    hits = 0
    for un_pnp, (pose, last) in seen.items():
        pose = pose.cpu().numpy()
        e = last["e"].cpu().numpy()
        for b in range(len(rts)):
            est = twin.render_depth(pts, faces, twin.scaled(pose[b], 1000.0), Kc, size)
            want = twin.vsd_pair(est, gt_renders[b], twin.sensor_depth(raw[b]), Kc)["e"]
            print("un_pnp=%s image %d: e %.6f twin %.6f" % (un_pnp, b, e[b, 0, 0], want))
            assert e[b, 0, 0] == want
            assert bool(last["hits"][b]) == (want < 0.3)
            hits += want < 0.3
    assert s == {"vsd": hits / 8.0} and hits >= 1, s
