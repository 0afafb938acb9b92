"""The depth rasteriser and the VSD kernel on the MI355X at the cases where the result turns on an exact comparison
(include/pvnet_vsd.h): edges exactly through sample centres, shared edges, the 32 / 33-sample and 64 / 65-block size classes
of the sweep, near clipping on the plane, the far cut, the snap limit, the scalar tail of the resolve pass; a visibility
difference exactly delta, a cost exactly tau and one float32 step to either side, partial tiles.  Inputs are the constructed
ones of tests/vsd_twin.py (checked without a GPU in tests/test_vsd.py); the device must equal the numpy twin as float32 bit
patterns, a closed form written by hand, and the fixture the reference's own functions made (tests/golden/vsd_rules.npz).
Each test prints its sample counts: covered, on a boundary, with differing bits (expected 0)."""
import os

import numpy as np
import pytest

from tests import vsd_twin as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOUP_SIZES = ((37, 29), (5, 4), (67, 3), (1, 1))


def _t(gpu, a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=gpu)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device(gpu, m, faces=None, pose=None, K=None, near=None, far=None):
    """The device's render of a constructed mesh (one pose unless ``pose`` is a batch): numpy float32."""
    from clean_pvnet_amd.vsd import render_depth
    pose = np.asarray(m["pose"] if pose is None else pose, np.float64)
    out = render_depth(_t(gpu, m["pts"]), _t(gpu, m["faces"] if faces is None else faces), _t(gpu, pose.reshape(-1, 3, 4)),
                       _t(gpu, m["K"] if K is None else K), m["size"], m["near"] if near is None else near,
                       m["far"] if far is None else far).cpu().numpy()
    return out[0] if pose.ndim == 2 else out


def _twin(m, faces=None):
    return twin.render_depth(m["pts"], m["faces"] if faces is None else faces, m["pose"], m["K"], m["size"], m["near"], m["far"])


def _report(what, got, want, boundary=None):
    diff = int((_bits(got) != _bits(want)).sum())
    print("%s: covered %d, covered and on a boundary %s, samples with differing bits %d" %
          (what, int((want > 0).sum()), "n/a" if boundary is None else int((boundary & (want > 0)).sum()), diff))
    return diff


# ------------------------------------------------------------------------------------------------ 1. renders, bit for bit
@pytest.mark.parametrize("seed", range(6))
def test_lattice_soups_equal_the_twin_bit_for_bit(pkg, gpu, seed):
    """Edges exactly through sample centres, degenerate rows; 1 x 1, a 3-row and a 20-sample image; P*H*W % 4 = 0 and 1."""
    for size in SOUP_SIZES:
        m = twin.lattice_soup(seed, size)
        want = _twin(m)
        assert _report("soup %d %s" % (seed, size), _device(gpu, m), want, m["boundary"]) == 0
        if size == SOUP_SIZES[0]:
            assert (m["boundary"] & (want > 0)).any() and (m["boundary"] & ~(want > 0)).any()


@pytest.mark.parametrize("seed", (1, 4))
def test_partition_equals_the_closed_form_and_the_twin(pkg, gpu, seed):
    """Every interior edge is shared by two triangles and every outer one runs through sample centres or integers: the
    render is the hand-written rectangle of the ownership rule (independent of the twin), and the twin's."""
    m = twin.partition_mesh(seed, (26, 19))                              # 494 samples: P*H*W % 4 = 2
    got = _device(gpu, m)
    assert _report("partition %d, closed form" % seed, got, m["closed_form"]) == 0
    assert _report("partition %d, twin" % seed, got, _twin(m)) == 0


def test_size_classes_of_the_sweep(pkg, gpu):
    """32 and 33 samples (lane / wave), 65 and 153 blocks (two and three rounds of the wave), a sliver through 153 blocks,
    |U| = 2**28 kept and the next lattice step dropped, 300 faces (a partial second block); three pieces with blocks
    whose only inside sample is the corner at which an owning edge function is exactly 0 (a block may be rejected only
    when the largest value is negative)."""
    m = twin.size_class_mesh()
    want = _twin(m)
    got = _device(gpu, m)
    assert _report("size classes", got, want) == 0
    for name in ("whole", "box32", "box33", "sliver", "blocks65", "limit", "beyond", "beyond_v", "corner_col", "corner_row",
                 "corner_slant"):                                        # and each one alone
        f = m["faces"][m["named"][name]][None]
        alone = _twin(m, f)
        one = _device(gpu, m, faces=f)
        assert _report("size classes, %s alone" % name, one, alone) == 0
        assert (alone > 0).any() == (not name.startswith("beyond"))
        if name.startswith("corner"):
            corners = twin.block_corner_samples(m, m["named"][name])
            print("size classes, %s: block corners on an owning edge %s" % (name, corners))
            assert len(corners) >= 2 and all(one[y, x] == 2.0 and got[y, x] == 2.0 for x, y in corners)


def test_near_clipping_on_the_lattice(pkg, gpu):
    """Zero to three vertices inside, a vertex exactly on the plane, shared clipped edges, waves in which only some lanes
    have a second piece, a quad at Z == far (kept) and one a float32 step beyond (dropped)."""
    m = twin.clip_mesh()                                                 # 29 x 23: P*H*W % 4 = 3
    want = _twin(m)
    assert _report("clip mesh", _device(gpu, m), want) == 0
    kept, dropped = m["far_quads"]
    for what, k in (("quad at far", kept), ("quad beyond far", dropped)):
        f = m["faces"][k:k + 2]
        assert _report("clip mesh, %s" % what, _device(gpu, m, faces=f), _twin(m, f)) == 0
    fans = m["faces"][:9]                                                # the two fans alone: nothing hides a clipped edge
    assert _report("clip mesh, fans", _device(gpu, m, faces=fans), _twin(m, fans)) == 0


def test_rasteriser_rules_on_the_device(pkg, gpu):
    """The cases of tests/test_vsd.py::test_twin_rasteriser_rules against the arrays written out by hand there."""
    m = {"K": np.array([[100.0, 0.0, 0.0], [0.0, 100.0, 0.0], [0.0, 0.0, 1.0]]), "pose": twin.pose([0, 0, 0], [0, 0, 0]),
         "size": (5, 4), "near": 1.0, "far": 10.0,
         "pts": np.array([[0.02, 0.02, 2], [0.06, 0.02, 2], [0.06, 0.06, 2], [0.02, 0.06, 2]], np.float32),
         "faces": np.array([[0, 1, 2], [0, 2, 3]], np.int32)}
    f = m["faces"]
    want = np.zeros((4, 5), np.float32)
    want[1:3, 1:3] = 2.0                                                 # the square [1, 3]^2: samples 1.5 and 2.5
    np.testing.assert_array_equal(_bits(_device(gpu, m)), _bits(want))
    one, two = _device(gpu, m, faces=f[:1]) > 0, _device(gpu, m, faces=f[1:]) > 0
    diagonal = np.zeros((4, 5), bool)
    diagonal[1, 1] = diagonal[2, 2] = True                               # the samples the shared diagonal runs through
    assert not (one & two).any() and ((one | two) == (want > 0)).all()   # one owner each:
    assert (two & diagonal).sum() == 2 and not (one & diagonal).any()    # (0,2,3) walks it downwards (dy > 0) and owns it
    upper = np.zeros((4, 5), bool)
    upper[1, 2] = True                                                   # what is left for (0,1,2): the sample (2.5, 1.5)
    np.testing.assert_array_equal(one, upper)
    np.testing.assert_array_equal(_bits(_device(gpu, m, faces=f[:, ::-1].copy())), _bits(want))          # no culling
    # edges exactly through the samples (u, v in [1.5, 3.5]): the top and right edges own, the bottom and left do not
    m2 = dict(m, pts=np.array([[0.03, 0.03, 2], [0.07, 0.03, 2], [0.07, 0.07, 2], [0.03, 0.07, 2]], np.float32))
    want2 = np.zeros((4, 5), np.float32)
    want2[1:3, 2:4] = 2.0
    np.testing.assert_array_equal(_bits(_device(gpu, m2)), _bits(want2))
    np.testing.assert_array_equal(_bits(_twin(m2)), _bits(want2))
    # outside [near, far]; Z == near and Z == far are inside
    assert not _device(gpu, m, near=2.5, far=10.0).any() and not _device(gpu, m, near=0.5, far=1.5).any()
    np.testing.assert_array_equal(_bits(_device(gpu, m, near=2.0, far=2.0)), _bits(want))
    # bad face rows are skipped, a NaN pose gives an empty image
    bad = np.array([[0, 1, 2], [0, 2, 4], [-1, 2, 3]], np.int32)
    np.testing.assert_array_equal(_device(gpu, m, faces=bad) > 0, upper)
    Pn = m["pose"].copy()
    Pn[1, 2] = np.nan
    assert not _device(gpu, m, pose=Pn).any()


def test_one_batched_call(pkg, gpu):
    """P = 3 at 37 x 29 (3219 samples, % 4 = 3: the scalar tail), the middle pose NaN, a camera per pose with skew and a
    negative cx: each image equals the twin's, the call equals the three P = 1 calls, and two runs give the same bytes."""
    m = twin.lattice_soup(3, (37, 29))
    poses = np.stack([m["pose"], m["pose"], twin.pose([0.05, -0.08, 0.3], [0.02, -0.01, 0.5])])
    poses[1, 0, 3] = np.nan
    Ks = np.stack([np.array([[128.0, 0.5, -2.0], [0.0, 128.0, 0.0], [0.0, 0.0, 1.0]]), m["K"],
                   np.array([[120.0, -0.75, -3.25], [0.0, 131.0, 2.5], [0.0, 0.0, 1.0]])])
    got = _device(gpu, m, pose=poses, K=Ks)
    assert got.shape == (3, 29, 37) and got.size % 4 == 3
    for i in range(3):
        want = twin.render_depth(m["pts"], m["faces"], poses[i], Ks[i], m["size"], m["near"], m["far"])
        assert _report("batched call, pose %d" % i, got[i], want) == 0
        assert (want > 0).any() == (i != 1)
        one = _device(gpu, m, pose=poses[i:i + 1], K=Ks[i:i + 1])
        np.testing.assert_array_equal(_bits(one[0]), _bits(got[i]))
    np.testing.assert_array_equal(_bits(_device(gpu, m, pose=poses, K=Ks)), _bits(got))
    shared = _device(gpu, m, pose=poses, K=Ks[2])                        # one camera for all three
    np.testing.assert_array_equal(_bits(shared[2]), _bits(got[2]))


# ---------------------------------------------------------------------------------------------- 2. VSD from depth images
def _sensor(gpu, kind, depth):
    """(tensor [1,H,W], depth_scale) of one sensor image in the given element type."""
    import torch
    if kind == "float64":
        return _t(gpu, depth[None], torch.float64), 1.0
    if kind == "float32":
        assert np.array_equal(depth.astype(np.float32).astype(np.float64), depth)
        return _t(gpu, depth[None], torch.float32), 1.0
    return torch.from_numpy(twin.rules_uint16(depth)[None].copy()).to(gpu), 0.125


@pytest.mark.parametrize("kind", ("float64", "float32", "uint16"))
def test_vsd_from_depth_on_the_rules_fixture(pkg, gpu, kind):
    """Differences exactly delta and tau and a float32 step to either side, invalid pixels, 300 pixels (a partial second
    tile) and 37 (one partial tile), all zero: counts equal to the reference's, 'step' e bit for bit, 'tlinear' e equal
    to the twin's fixed-order sum and within tlinear_bound of the reference.  The two rows 2**-30 off need binary64 and
    are in the float64 run only."""
    import torch
    from clean_pvnet_amd.vsd import vsd_from_depth
    c = dict(np.load(os.path.join(GOLDEN, "vsd_rules.npz")))
    K, delta, tau = c["K"], float(c["delta"]), float(c["tau"])
    cases = ("f64", "f32", "small", "zero") if kind == "float64" else ("f32", "small", "zero")
    results = {}
    for name in cases:
        depth, gt, est = c[name + "_test"], c[name + "_gt"], c[name + "_est"]
        dt, scale = _sensor(gpu, kind, depth)
        args = (_t(gpu, est[None]), _t(gpu, gt[None]), dt, _t(gpu, K))
        kw = dict(delta=delta, tau=tau, depth_scale=scale)
        e, cnt = vsd_from_depth(*args, cost="step", return_counts=True, **kw)
        assert e.dtype == torch.float64 and tuple(e.shape) == (1,) + c[name + "_e_step"].shape
        counts = np.stack([cnt[k].cpu().numpy() for k in ("union", "inter", "cost")], -1)[0]
        print("%s %s: pixels %d, counts %s, e %s" % (kind, name, depth.size, counts.tolist(), e.cpu().numpy().tolist()))
        np.testing.assert_array_equal(counts, c[name + "_counts"])
        np.testing.assert_array_equal(e.cpu().numpy()[0].view(np.uint64), c[name + "_e_step"].view(np.uint64))
        tl, cnt_tl = vsd_from_depth(*args, cost="tlinear", return_counts=True, **kw)
        np.testing.assert_array_equal(np.stack([cnt_tl[k].cpu().numpy() for k in ("union", "inter", "cost")], -1)[0], counts)
        got = tl.cpu().numpy()[0]
        for a, b in np.ndindex(*got.shape):
            tw = twin.vsd_pair(est[a], gt[b], depth, K, delta, tau, "tlinear")
            want = float(c[name + "_e_tlinear"][a, b])
            bound = twin.tlinear_bound(want, int(counts[a, b, 1]), float(c[name + "_cost_sum"][a, b]), int(counts[a, b, 0]))
            print("%s %s[%d,%d] tlinear got %.17g twin %.17g reference %.17g |diff| %.3g bound %.3g" %
                  (kind, name, a, b, got[a, b], tw["e"], want, abs(got[a, b] - want), bound))
            assert got[a, b] == tw["e"]
            assert abs(got[a, b] - want) <= bound
        e2 = vsd_from_depth(*args, cost="step", **kw)                    # twice: the same bytes
        tl2 = vsd_from_depth(*args, cost="tlinear", **kw)
        assert torch.equal(e, e2) and torch.equal(tl, tl2)
        results[name] = (e, tl)
    assert float(results["zero"][0]) == 1.0 and float(results["zero"][1]) == 1.0          # union == 0
    # two images in one call, a camera per image, the second ground-truth slot of the second image masked
    if kind == "float64":
        names = ("f64", "f32")
        est, gt = (np.stack([c[n + w] for n in names]) for w in ("_est", "_gt"))
        dt = _t(gpu, np.stack([c[n + "_test"] for n in names]))
        valid = _t(gpu, [[True, True], [True, False]])
        for cost in ("step", "tlinear"):
            e = vsd_from_depth(_t(gpu, est), _t(gpu, gt), dt, _t(gpu, np.stack([K, K])), delta=delta, tau=tau, cost=cost,
                               depth_scale=1.0, gt_valid=valid)
            k = 0 if cost == "step" else 1
            assert torch.equal(e[0], results["f64"][k][0]) and torch.equal(e[1, :, 0], results["f32"][k][0, :, 0])
            assert bool(torch.isnan(e[1, :, 1]).all())


def test_vsd_is_render_depth_then_vsd_from_depth(pkg, gpu):
    import torch
    from clean_pvnet_amd.vsd import render_depth, vsd, vsd_from_depth
    c = dict(np.load(os.path.join(GOLDEN, "vsd_near.npz")))
    r = twin.regenerate("vsd_near", c)
    pts, faces, K, raw = _t(gpu, r["pts"]), _t(gpu, r["faces"]), _t(gpu, c["K"]), torch.from_numpy(r["raw"]).to(gpu)
    kw = dict(delta=float(c["delta"]), tau=float(c["tau"]), depth_scale=float(c["depth_scale"]))
    ts, near, far = float(c["t_scale"]), float(c["near"]), float(c["far"])
    n, p = c["pose_est"].shape[:2]
    g = c["pose_gt"].shape[1]
    H, W = r["size"][1], r["size"][0]
    d_est = render_depth(pts, faces, _t(gpu, twin.scaled(c["pose_est"], ts).reshape(-1, 3, 4)), K, r["size"], near, far)
    d_gt = render_depth(pts, faces, _t(gpu, twin.scaled(c["pose_gt"], ts).reshape(-1, 3, 4)), K, r["size"], near, far)
    for cost in ("step", "tlinear"):
        e, im = vsd(_t(gpu, c["pose_est"]), _t(gpu, c["pose_gt"]), raw, K, pts, faces, cost=cost, t_scale=ts, near=near, far=far,
                    return_images=True, **kw)
        e2, cnt = vsd_from_depth(d_est.view(n, p, H, W), d_gt.view(n, g, H, W), raw, K, cost=cost, return_counts=True, **kw)
        assert torch.equal(e.view(torch.int64), e2.view(torch.int64))
        assert torch.equal(im["depth_est"].view(torch.int32), d_est.view(n, p, H, W).view(torch.int32))
        assert torch.equal(im["depth_gt"].view(torch.int32), d_gt.view(n, g, H, W).view(torch.int32))
        assert sorted(cnt) == ["cost", "inter", "union"] and all(torch.equal(im[k], cnt[k]) for k in cnt)
        assert set(im) == {"depth_est", "depth_gt", "union", "inter", "cost"}
    print("vsd == render_depth + vsd_from_depth on vsd_near: e", e2.cpu().numpy().tolist())
