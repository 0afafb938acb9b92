"""The batched ICP refinement on the MI355X (include/pvnet_icp.h, clean_pvnet_amd.icp): with injected samples the poses equal
the numpy twin as binary64 bit patterns (tests/icp_twin.py, itself held to the reference's own ICPRefiner.refine on the
fixtures in tests/test_icp.py), the counts and rounds are equal, the result does not depend on the batch or on the dtypes; with
device-drawn samples it is repeatable and improves the pose; and network output -> pose -> ICP -> scores runs with no host
synchronisation."""
import os

import numpy as np
import pytest

from oracle import pnp_oracle as po
from tests import icp_twin as twin
from tests import tolerances as tol
from tests import vsd_twin as vt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("icp_720", "icp_360", "icp_edge")
INFO = ("status", "n_syn", "n_real", "n", "rounds")
STAGE = (dict(depth_only=True, max_mean_dist_factor=5.0), dict(no_depth=True, max_mean_dist_factor=2.0))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _t(gpu, a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=gpu)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _info(d):
    return np.stack([d[k].cpu().numpy() for k in INFO], 1)


def _inputs(gpu, name):
    import torch
    c = load(name)
    r = twin.regenerate(name, c)
    t = {"pts": _t(gpu, r["pts"]), "faces": _t(gpu, r["faces"]), "K": _t(gpu, c["K"]), "raw": torch.from_numpy(r["raw"]).to(gpu),
         "mask": torch.from_numpy(r["mask"]).to(gpu), "est": _t(gpu, c["pose_est"]), "gt": _t(gpu, c["pose_gt"]),
         "idx": _t(gpu, c["idx"])}
    kw = dict(depth_scale=float(c["depth_scale"]), n_max=int(c["n_max"]), tolerance=float(c["tolerance"]),
              angle_limit_deg=float(c["angle_limit_deg"]))
    return c, r, t, kw


def _stage_starts(gpu, c):
    """The pose each stage starts from, in millimetres: the estimate, then the twin's stage-1 result."""
    return _t(gpu, vt.scaled(c["pose_est"], float(c["t_scale"]))), _t(gpu, c["twin_stage"][0])


# --------------------------------------------------------------------------------------- 1. the stages, bit for bit, repeatable
@pytest.mark.parametrize("name", FIXTURES)
def test_stages_equal_the_twin_bit_for_bit(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.icp import icp_refine, refine
    c, r, t, kw = _inputs(gpu, name)
    P = len(c["pose_est"])
    for s, start in enumerate(_stage_starts(gpu, c)):
        samples = (t["idx"][s, 0], t["idx"][s, 1])
        out, info = refine(t["raw"], start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, return_info=True,
                           **STAGE[s], **kw)
        assert out.dtype == torch.float64 and tuple(out.shape) == (P, 3, 4)
        got, gi = out.cpu().numpy(), _info(info)
        print("%s stage %d: info %s" % (name, s + 1, gi.tolist()))
        np.testing.assert_array_equal(gi, c["info"][s])                              # status, n_syn, n_real, n, rounds
        np.testing.assert_array_equal(gi[:, 4], c["ref_rounds"][s])
        np.testing.assert_array_equal(_bits(got), _bits(c["twin_stage"][s]))
        tol.assert_means_close(got[:, :, 3], c["ref_t"][s], what="stage t (mm) against the reference")
        tol.assert_means_close(got[:, :, :3], c["ref_R"][s], what="stage R against the reference")
        out2, info2 = refine(t["raw"], start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, return_info=True,
                             **STAGE[s], **kw)
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and np.array_equal(_info(info2), gi)
        per = r["per_image"]
        for p in range(P):                                                           # a pose alone equals its row of the batch
            i = p // per
            one, io = refine(t["raw"][i:i + 1], start[p:p + 1], t["K"], t["pts"], t["faces"], mask=t["mask"][p:p + 1],
                             samples=(samples[0][p:p + 1], samples[1][p:p + 1]), return_info=True, **STAGE[s], **kw)
            assert torch.equal(one[0].view(torch.int64), out[p].view(torch.int64)) and np.array_equal(_info(io)[0], gi[p])
    samples = ((t["idx"][0, 0], t["idx"][0, 1]), (t["idx"][1, 0], t["idx"][1, 1]))
    kw2 = {k: v for k, v in kw.items() if k != "depth_scale"}
    both, infos = icp_refine(t["est"], t["raw"], t["mask"], t["K"], t["pts"], t["faces"], t_scale=float(c["t_scale"]),
                             depth_scale=kw["depth_scale"], samples=samples, return_info=True, **kw2)
    np.testing.assert_array_equal(_bits(both.cpu().numpy()), _bits(c["twin_pose"]))
    np.testing.assert_array_equal(np.stack([_info(i) for i in infos]), c["info"])
    tol.assert_means_close(both.cpu().numpy()[:, :, 3] * 1000.0, c["ref_pose"][:, :, 3] * 1000.0)
    tol.assert_means_close(both.cpu().numpy()[:, :, :3], c["ref_pose"][:, :, :3])


# ------------------------------------------------------------------------- 2. a short loop, the rotation limit, per-pose cameras
def test_three_rounds_and_the_rotation_limit_equal_the_twin(pkg, gpu):
    import torch
    from clean_pvnet_amd.icp import refine
    c, r, t, kw = _inputs(gpu, "icp_360")
    starts = _stage_starts(gpu, c)
    p = 0
    z_img = vt.sensor_depth(r["raw"][0], kw["depth_scale"])
    for s, extra, status in ((0, dict(max_iterations=3), twin.REFINED), (1, dict(max_iterations=3), twin.REFINED),
                             (1, dict(max_iterations=10, angle_limit_deg=0.5), twin.ROTATION_LIMIT)):
        k = {**kw, **extra}
        start = starts[s][p:p + 1]
        want, wi = twin.refine(z_img, start[0].cpu().numpy(), c["K"], r["pts"], r["faces"], r["size"], mask=r["mask"][p],
                               samples=(c["idx"][s, 0, p], c["idx"][s, 1, p]), **STAGE[s],
                               **{a: b for a, b in k.items() if a != "depth_scale"})
        assert wi["status"] == status and wi["rounds"] == extra["max_iterations"], wi
        Kp = t["K"][None].clone()                                                    # a camera per pose: the same bits
        got, gi = refine(t["raw"][:1], start, Kp, t["pts"], t["faces"], mask=t["mask"][p:p + 1],
                         samples=(t["idx"][s, 0, p:p + 1], t["idx"][s, 1, p:p + 1]), return_info=True, **STAGE[s], **k)
        print("stage %d %s: info %s" % (s + 1, extra, _info(gi).tolist()))
        assert _info(gi)[0].tolist() == [wi[a] for a in INFO]
        np.testing.assert_array_equal(_bits(got.cpu().numpy()[0]), _bits(want))
        if status == twin.ROTATION_LIMIT:                                            # the step is the identity
            assert torch.equal(got.view(torch.int64), start.view(torch.int64))


# ------------------------------------------------------------------------------------------- 3. the poses that stay unchanged
def test_each_unchanged_status_is_raised_by_its_input(pkg, gpu):
    import torch
    from clean_pvnet_amd.icp import icp_refine, refine
    c, r, t, kw = _inputs(gpu, "icp_360")
    start = _stage_starts(gpu, c)[0].clone()
    k = dict(kw, max_iterations=4)
    samples = (t["idx"][0, 0].clone(), t["idx"][0, 1].clone())
    base, bi = refine(t["raw"], start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, return_info=True,
                      **STAGE[0], **k)
    assert _info(bi)[:, 0].tolist() == [twin.REFINED] * 4
    bad = start.clone()
    bad[0, 1, 1] = float("nan")                                                      # pose 0: not finite
    bad[1, 2, 3] = -bad[1, 2, 3]                                                     # pose 1: t_z <= 0
    mask = t["mask"].clone()
    mask[2] = 0
    mask[2, :3, :6] = 1                                                              # pose 2: 18 pixels < 20
    samples[1][3, 5] = 10 ** 8                                                       # pose 3: an index outside the real cloud
    got, gi = refine(t["raw"], bad, t["K"], t["pts"], t["faces"], mask=mask, samples=samples, min_mask_pixels=20,
                     return_info=True, **STAGE[0], **k)
    gi = _info(gi)
    print("info:", gi.tolist())
    assert gi[:, 0].tolist() == [twin.BAD_POSE, twin.BAD_POSE, twin.SMALL_MASK, twin.BAD_INDEX]
    assert gi[:, 4].tolist() == [0, 0, 0, 0]
    assert torch.equal(got.view(torch.int64), bad.view(torch.int64))                 # bit for bit, the NaN included
    samples[0][3, 7] = -1                                                            # a negative index in the synthetic draw
    samples[1][3, 5] = 0
    got, gi = refine(t["raw"], start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, return_info=True,
                     **STAGE[0], **k)
    assert _info(gi)[:, 0].tolist() == [twin.REFINED] * 3 + [twin.BAD_INDEX]
    assert torch.equal(got[3].view(torch.int64), start[3].view(torch.int64))
    assert torch.equal(got[:3].view(torch.int64), base[:3].view(torch.int64))        # the neighbours are not disturbed
    # the two-stage recipe hands back, in metres and bit for bit, a pose stage 1 refuses
    est = t["est"].clone()
    est[1, 2, 3] = 0.0
    both, (i1, i2) = icp_refine(est, t["raw"], t["mask"], t["K"], t["pts"], t["faces"], depth_scale=kw["depth_scale"],
                                samples=((t["idx"][0, 0], t["idx"][0, 1]), (t["idx"][1, 0], t["idx"][1, 1])), max_iterations=4,
                                return_info=True)
    assert _info(i1)[1, 0] == twin.BAD_POSE and _info(i2)[1, 0] == twin.BAD_POSE
    assert torch.equal(both[1].view(torch.int64), est[1].view(torch.int64)) and not torch.equal(both[0], est[0])


# ------------------------------------------------------------------------------------------------------ 4. every input dtype
def test_sensor_and_mask_dtypes_give_the_same_bits(pkg, gpu):
    import torch
    from clean_pvnet_amd.icp import refine
    c, r, t, kw = _inputs(gpu, "icp_360")
    start = _stage_starts(gpu, c)[0]
    # a scale of 1/8 makes raw * scale exact in float32: the three sensor types then hold the same numbers
    raw_np = (r["raw"].astype(np.int64) * 4 // 5).astype(np.uint16)                  # 0.1 / 0.125 of the stored units
    raw = torch.from_numpy(raw_np).to(gpu)
    k = dict(kw, max_iterations=5, depth_scale=0.125)
    samples = (t["idx"][0, 0], t["idx"][0, 1])
    want, wi = refine(raw, start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, return_info=True, **STAGE[0], **k)
    assert _info(wi)[:, 0].tolist() == [twin.REFINED] * 4 and _info(wi)[:, 4].tolist() == [5] * 4
    z_img = raw_np.astype(np.float64) * 0.125
    p = 1
    tw, _ = twin.refine(z_img[p // r["per_image"]], start[p].cpu().numpy(), c["K"], r["pts"], r["faces"], r["size"], mask=r["mask"][p],
                        samples=(c["idx"][0, 0, p], c["idx"][0, 1, p]), n_max=k["n_max"], max_iterations=5, **STAGE[0])
    np.testing.assert_array_equal(_bits(want[p].cpu().numpy()), _bits(tw))
    for depth in (_t(gpu, z_img, torch.float32), _t(gpu, z_img, torch.float64)):
        assert torch.equal(depth.to(torch.float64), _t(gpu, z_img))
        got = refine(depth, start, t["K"], t["pts"], t["faces"], mask=t["mask"], samples=samples, **STAGE[0], **dict(k, depth_scale=1.0))
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), depth.dtype
    for mask in (t["mask"] != 0, t["mask"].to(torch.int64)):
        got = refine(raw, start, t["K"], t["pts"], t["faces"], mask=mask, samples=samples, **STAGE[0], **k)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), mask.dtype
    with pytest.raises(TypeError):
        refine(raw, start, t["K"], t["pts"], t["faces"], mask=t["mask"].to(torch.float32), samples=samples, **STAGE[0], **k)


# ------------------------------------------------------------------------------------------------- 5. device-drawn samples
@pytest.mark.parametrize("name", ("icp_360",))
def test_device_drawn_samples_repeat_and_improve_the_pose(pkg, gpu, name):
    """The fixture without an occluder: the ADD of the refined pose against the ground truth is below the ADD of the start."""
    import torch
    from clean_pvnet_amd.icp import IcpRefiner
    from clean_pvnet_amd.metrics import pose_metrics
    c, r, t, kw = _inputs(gpu, name)
    assert not bool(c["occluder"])
    ref = IcpRefiner(r["pts"], r["faces"], r["size"], device=gpu, depth_scale=kw["depth_scale"])
    outs = []
    for _ in range(2):
        g = torch.Generator(device=gpu)
        g.manual_seed(11)
        outs.append(ref.icp_refine(t["est"], t["raw"], t["mask"], t["K"], generator=g, return_info=True))
    (a, (a1, a2)), (b, (b1, b2)) = outs
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert np.array_equal(_info(a1), _info(b1)) and np.array_equal(_info(a2), _info(b2))
    assert (_info(a1)[:, 0] == twin.REFINED).all()
    model = t["pts"] / 1000.0                                                        # the poses are in metres
    before = pose_metrics(t["est"], t["gt"], model, t["K"])["add"].cpu().numpy()
    after = pose_metrics(a, t["gt"], model, t["K"])["add"].cpu().numpy()
    print("ADD before (mm)", (1e3 * before).round(3).tolist(), "after", (1e3 * after).round(3).tolist(),
          "status", _info(a1)[:, 0].tolist(), _info(a2)[:, 0].tolist(), "rounds", _info(a1)[:, 4].tolist(), _info(a2)[:, 4].tolist())
    assert (after < before).all()


# ---------------------------------------------------------------------------------------------------- 6. end to end, no sync
def test_network_output_to_scores_through_icp_with_no_host_sync(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.icp import IcpRefiner
    from clean_pvnet_amd.metrics import pose_metrics
    from clean_pvnet_amd.pose import solve_pose
    from clean_pvnet_amd.vsd import VsdEvaluator
    from tests.test_gpu_vsd import _rendered_fields
    x, P, Kc, rts = _rendered_fields(gpu)
    pts, faces = vt.mesh(9)                                              # millimetres; the poses are in metres
    size = (320, 240)
    gt = np.stack([np.concatenate([po.rodrigues(rt[:3]), rt[3:].reshape(3, 1)], 1) for rt in rts])
    gt_renders = vt.render_batch(pts, faces, vt.scaled(gt, 1000.0), Kc, size)
    raw = np.stack([vt.scene_depth(90 + i, gt_renders[i:i + 1], occluder=False) for i in range(len(gt))])
    Pt, Kt, Gt, Rt = _t(gpu, P), _t(gpu, Kc), _t(gpu, gt), torch.from_numpy(raw).to(gpu)
    Mt = _t(gpu, (gt_renders > 0).astype(np.uint8))
    model = _t(gpu, pts) / 1000.0
    ev = VsdEvaluator(pts, faces, size, device=gpu)
    ref = IcpRefiner(pts, faces, size, device=gpu, min_mask_pixels=20)
    g = torch.Generator(device=gpu)
    g.manual_seed(5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o = {"seg": x[:, :2], "vertex": x[:, 2:]}
        decode_keypoint(o, un_pnp=True, weights=True, seed=3)
        solve_pose(o, Pt, Kt, un_pnp=True)
        refined, (i1, i2) = ref.icp_refine(o["pose"], Rt, Mt, Kt, generator=g, return_info=True)
        m0 = pose_metrics(o["pose"], Gt, model, Kt)
        m1 = pose_metrics(refined, Gt, model, Kt)
        ev.evaluate(refined[:, None], Gt[:, None], Rt, Kt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = ev.summarize()                                                   # the one read-back
    add0, add1 = m0["add"].cpu().numpy(), m1["add"].cpu().numpy()
    print("summarize:", s, "ADD before (mm)", (1e3 * add0).round(3).tolist(), "after", (1e3 * add1).round(3).tolist(),
          "status", _info(i1)[:, 0].tolist(), _info(i2)[:, 0].tolist())
    assert bool(torch.isfinite(refined).all()) and np.isfinite(add1).all()
    assert (_info(i1)[:, 0] == twin.REFINED).all() and (_info(i1)[:, 3] > 0).all()
    assert 0.0 <= s["vsd"] <= 1.0
