"""Detector decode, crops and the way back on the MI355X (clean_pvnet_amd.crop): every output equals the numpy twin
(tests/crop_twin.py, itself held to the reference's ``decode_ct_hm`` in tests/test_crop.py) bit for bit, on a side stream as on
the default stream; and the results feed ``decode_keypoint`` -> ``pose.pose_batched`` and ``icp.icp_refine`` as they are."""
import os

import numpy as np
import pytest

from tests import crop_twin as twin
from tests import vsd_twin as vt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("crop_ct_small", "crop_ct_seams", "crop_ct_full")
KW = dict(scale_ratio=twin.SCALE_RATIO, mean=twin.MEAN, std=twin.STD)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _t(gpu, a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=gpu)


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_np(v) for v in x)
    return x.cpu().numpy()


def _same(a, b):
    """Equal as bit patterns (dicts and tuples element-wise)."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def on_both_streams(f):
    """f() on a side stream and on the default stream: the two results are the same bits; returns them as numpy."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = f()
    side.synchronize()
    a = _np(a)
    b = _np(f())
    assert _same(a, b), "the side stream's result differs from the default stream's"
    return a


# ------------------------------------------------------------------------------------------------------------ 1. decode_ct_hm
def _decode(gpu, hm, wh, K, clip=True):
    from clean_pvnet_amd.crop import decode_ct_hm
    d_hm, d_wh = _t(gpu, hm), _t(gpu, wh)
    return on_both_streams(lambda: decode_ct_hm(d_hm, d_wh, K=K, clip=clip))


@pytest.mark.parametrize("name", FIXTURES)
def test_decode_equals_the_twin_and_the_reference_on_the_fixtures(pkg, gpu, name):
    c = load(name)
    hm, wh = twin.regenerate(c)
    K = int(c["K"])
    for clip, want in ((True, c["ref_detection_clip"]), (False, c["ref_detection"])):
        ct, det, count = _decode(gpu, hm, wh, K, clip)
        assert _same((ct, det, count), twin.decode_ct_hm(hm, wh, K=K, clip=clip))
        assert _same(det, want) and _same(ct, c["ref_ct"]) and _same(count, c["count"])      # the reference's own rows


def test_decode_ties_short_counts_and_the_plateau_across_a_seam(pkg, gpu):
    from clean_pvnet_amd.crop import decode_ct_hm
    for hm, wh, K in (twin.tie_case(), twin.short_case()):                      # (short_case: B=3, one image all zero)
        got = _decode(gpu, hm, wh, K)
        assert _same(got, twin.decode_ct_hm(hm, wh, K=K))
    assert got[2].tolist() == [3, 0, K]
    c = load("crop_ct_seams")
    for K in (64, 256):                                                          # the plateau and the background's peaks; the largest K
        got = _decode(gpu, c["ct_hm"], c["wh"], K, clip=False)
        assert _same(got, twin.decode_ct_hm(c["ct_hm"], c["wh"], K=K, clip=False))
    assert (got[1][0, :, 4] == np.float32(0.55)).sum() == 2
    hm, wh = twin.heat_maps(8, (2, 1, 4, 4))                                     # K = H*W: every candidate, then zero rows
    assert _same(_decode(gpu, hm, wh, 16), twin.decode_ct_hm(hm, wh, K=16))
    with pytest.raises(ValueError):
        decode_ct_hm(_t(gpu, hm), _t(gpu, wh), K=17)


# ------------------------------------------------------------------------------------------------------------ 2. crop_boxes
def _crop_inputs():
    img = np.stack([twin.image(1), twin.image(2)])
    boxes = np.concatenate([twin.BOXES[:2], [[3.0, np.inf, 9.0, 12.0]], twin.BOXES[2:]])        # one invalid box between valid ones
    index = np.array([0, 1, 1, 1, 0, 1])
    return img, boxes, index


@pytest.mark.parametrize("box_ratio", [None, twin.BOX_RATIO])
@pytest.mark.parametrize("out_size", [(32, 32), (256, 256)])
def test_crops_equal_the_twin(pkg, gpu, out_size, box_ratio):
    import torch
    from clean_pvnet_amd.crop import crop_boxes
    img, boxes, index = _crop_inputs()
    want = twin.crop_boxes(img, boxes, index, out_size, box_ratio=box_ratio, **KW)
    want.pop("u8")
    assert want["valid"].tolist() == [True, True, False, True, True, True]
    d_img = _t(gpu, img)
    for bdt, idt in ((torch.float64, torch.int64), (torch.float32, torch.int32)):  # (these boxes are exact in float32)
        d_boxes, d_index = _t(gpu, boxes, bdt), _t(gpu, index, idt)
        got = on_both_streams(lambda: crop_boxes(d_img, d_boxes, d_index, out_size, box_ratio=box_ratio, **KW))
        for k in want:
            assert _same(got[k], want[k]), k
    none = crop_boxes(d_img, d_boxes[:0], d_index[:0], out_size, box_ratio=box_ratio, **KW)       # N = 0
    assert tuple(none["inp"].shape) == (0, 3, out_size[1], out_size[0]) and tuple(none["trans"].shape) == (0, 2, 3)
    assert none["valid"].dtype == torch.bool and none["valid"].numel() == 0


def test_crop_of_an_odd_size_and_the_half_way_blanking_corner(pkg, gpu):
    """An output that fills neither a block's 64 columns nor its 4 rows, and the rectangle whose corners land on .5."""
    from clean_pvnet_amd.crop import crop_boxes
    img, boxes, index = _crop_inputs()
    d_img, d_boxes, d_index = _t(gpu, img), _t(gpu, boxes), _t(gpu, index)
    want = twin.crop_boxes(img, boxes, index, (70, 37), box_ratio=0.9, **KW)
    got = on_both_streams(lambda: crop_boxes(d_img, d_boxes, d_index, (70, 37), box_ratio=0.9, **KW))
    assert all(_same(got[k], want[k]) for k in got)
    box = np.array([[4.0, 4.0, 36.0, 36.0]])
    kw = dict(scale_ratio=1.0, box_ratio=25 / 32, mean=twin.MEAN, std=twin.STD)
    want = twin.crop_boxes(img, box, [1], (32, 32), **kw)
    got = _np(crop_boxes(d_img, _t(gpu, box), _t(gpu, [1]), (32, 32), **kw))
    assert all(_same(got[k], want[k]) for k in got)


# ------------------------------------------------------------------------------------------------------------ 3. the ways back
def test_uncrop_keypoints_equals_the_twin(pkg, gpu):
    import torch
    from clean_pvnet_amd.crop import uncrop_keypoints
    rng = np.random.default_rng(7)
    kpt = rng.random((5, 9, 2)) * 256 - 20                                       # K=9, N=5
    trans = np.stack([twin.box_transform(b, (256, 256), twin.SCALE_RATIO)[2] for b in twin.BOXES])
    trans[3] = 0                                                                 # an invalid box's map
    d_trans = _t(gpu, trans)
    for dt in (np.float64, np.float32):
        d_kpt = _t(gpu, kpt.astype(dt))
        got = on_both_streams(lambda: uncrop_keypoints(d_kpt, d_trans))
        assert _same(got, twin.uncrop_keypoints(kpt.astype(dt), trans))
    assert not got[3].any()
    assert tuple(uncrop_keypoints(d_kpt[:0], d_trans[:0]).shape) == (0, 9, 2)


@pytest.mark.parametrize("canvas", [(72, 54), (720, 540), (71, 53)])           # (71: the byte-wise store of a width that is no multiple of 4)
def test_uncrop_mask_equals_the_twin(pkg, gpu, canvas):
    import torch
    from clean_pvnet_amd.crop import uncrop_mask
    rng = np.random.default_rng(9)
    mask = (rng.random((3, 40, 48)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (3, 40, 48)).astype(np.uint8)
    f = canvas[0] / 72.0
    trans = np.stack([twin.box_transform(np.asarray(b) * f, (48, 40), twin.SCALE_RATIO)[2] for b in twin.BOXES[[0, 1, 4]]])   # N=3
    want = twin.uncrop_mask(mask, trans, canvas)
    assert want.any() and (want == 0).any()
    d_trans = _t(gpu, trans)
    for dt in (torch.uint8, torch.int64):
        d_mask = _t(gpu, mask, dt)
        got = on_both_streams(lambda: uncrop_mask(d_mask, d_trans, canvas))
        assert _same(got, want)
    d_bool = _t(gpu, mask != 0)
    assert _same(_np(uncrop_mask(d_bool, d_trans, canvas)), twin.uncrop_mask((mask != 0).astype(np.uint8), trans, canvas))


# ------------------------------------------------------------------------------------------------------------ 4. the chains
def _scene(gpu, size, cam_scale):
    """Two poses of the seeded mesh, their renders (mm) on the device, the boxes around them and 9 model keypoints."""
    import torch
    from clean_pvnet_amd import vsd as V
    pts, faces = vt.mesh(5)
    gt = np.stack([vt.pose([0.9, 0.4, -0.3], [-0.05, 0.02, 0.70]), vt.pose([0.3, -0.8, 0.5], [0.06, -0.01, 0.74])])
    K = vt.camera(cam_scale)
    d = {"pts": _t(gpu, pts), "faces": _t(gpu, faces), "K": _t(gpu, K), "gt": _t(gpu, gt)}
    d["depth"] = V.render_depth(d["pts"], d["faces"], _t(gpu, vt.scaled(gt, 1000.0)), d["K"], size)
    kpt_3d = pts[np.arange(9) * 131 % len(pts)].astype(np.float64) / 1000.0                      # metres; spread over the tube
    cam = np.einsum("pij,kj->pki", gt[:, :, :3], kpt_3d) + gt[:, None, :, 3]
    proj = np.einsum("ij,pkj->pki", K, cam)
    kpt_2d = proj[..., :2] / proj[..., 2:]
    boxes = np.concatenate([kpt_2d.min(1) - 6, kpt_2d.max(1) + 6], 1)
    return d, gt, K, kpt_3d, kpt_2d, boxes


def test_chain_crops_to_keypoints_to_pose(pkg, gpu):
    """crop_boxes -> a stand-in network (a vector field that points at the keypoints' crop positions) -> decode_keypoint ->
    uncrop_keypoints -> pose_batched.  The uncropped keypoints are the twin's map of the decoded ones, bit for bit; they lie
    within 0.01 image pixels of the projections the field was built from (unit vectors in float32 are good to 6e-8, the lever
    is at most 128 * sqrt 2 crop pixels: 1e-5 pixels per vote, two orders below the bound), and the pose found reprojects
    the model onto them within sqrt(9) * 0.01 pixels -- the ground-truth pose does, and the refinement minimises that sum."""
    import torch
    from clean_pvnet_amd import crop, decode, pose
    size, out = (360, 270), (128, 128)
    d, gt, K, kpt_3d, kpt_2d, boxes = _scene(gpu, size, 0.5)
    img = _t(gpu, np.stack([twin.image(3, 270, 360)] * 2))
    d_boxes, d_index = _t(gpu, boxes), _t(gpu, [0, 1])

    def chain():
        c = crop.crop_boxes(img, d_boxes, d_index, out, **KW)
        a, t = c["trans"][:, 0, 0], c["trans"][:, :, 2]
        kc = _t(gpu, kpt_2d) * a[:, None, None] + t[:, None, :]                                 # the keypoints in crop pixels
        ys, xs = torch.meshgrid(torch.arange(out[1], device=gpu, dtype=torch.float64),
                                torch.arange(out[0], device=gpu, dtype=torch.float64), indexing="ij")
        v = kc[:, :, None, None, :] - torch.stack([xs, ys], -1)                                 # [N,9,h,w,2]
        v = (v / v.norm(dim=-1, keepdim=True)).float()
        inside = ((xs - 64) ** 2 + (ys - 64) ** 2 < 50 ** 2).to(torch.float32)
        output = {"seg": torch.stack([1 - inside, inside])[None].repeat(2, 1, 1, 1),
                  "vertex": v.permute(0, 1, 4, 2, 3).reshape(2, 18, out[1], out[0]).contiguous()}
        decode.decode_keypoint(output, seed=11)
        back = crop.uncrop_keypoints(output["kpt_2d"], c["trans"])
        res = pose.pose_batched(back, _t(gpu, kpt_3d), d["K"])
        return {"valid": c["valid"], "trans": c["trans"], "kpt_crop": output["kpt_2d"], "kpt": back, "Rt": res["Rt"],
                "status": res["status"]}

    r = on_both_streams(chain)
    assert r["valid"].all() and (r["status"] >= 0).all() and r["kpt"].dtype == np.float64
    assert _same(r["kpt"], twin.uncrop_keypoints(r["kpt_crop"], r["trans"]))
    assert np.abs(r["kpt"] - kpt_2d).max() <= 0.01, np.abs(r["kpt"] - kpt_2d).max()
    cam = np.einsum("pij,kj->pki", r["Rt"][:, :, :3], kpt_3d) + r["Rt"][:, None, :, 3]
    proj = np.einsum("ij,pkj->pki", K, cam)
    assert np.abs(proj[..., :2] / proj[..., 2:] - r["kpt"]).max() <= 0.03


def test_chain_crop_masks_to_canvas_to_icp(pkg, gpu):
    """crop_boxes -> a stand-in network's mask (the object's silhouette sampled at the crop's pixel centres) -> uncrop_mask ->
    icp_refine.  The canvas mask is the twin's, bit for bit, and lies inside the silhouette grown by the crop's pixel pitch;
    icp_refine takes it as it is and refines both poses."""
    import torch
    from clean_pvnet_amd import crop, icp
    size, out = (360, 270), (64, 64)
    d, gt, K, kpt_3d, kpt_2d, boxes = _scene(gpu, size, 0.5)
    img = _t(gpu, np.stack([twin.image(3, 270, 360)] * 2))
    d_boxes, d_index = _t(gpu, boxes), _t(gpu, [0, 1])
    sil = d["depth"] > 0                                                                        # [2,270,360]
    est = np.stack([np.concatenate([vt.rodrigues(w) @ g[:, :3], (g[:, 3] + dt).reshape(3, 1)], 1)
                    for g, w, dt in zip(gt, ([0.03, -0.02, 0.03], [-0.02, 0.03, 0.02]), ([0.002, -0.002, 0.008], [-0.002, 0.001, -0.006]))])
    d_est = _t(gpu, est)

    def chain():
        c = crop.crop_boxes(img, d_boxes, d_index, out, **KW)
        a, t = c["trans"][:, 0, 0], c["trans"][:, :, 2]
        u = torch.arange(out[0], device=gpu, dtype=torch.float64)
        sx = ((u[None, :] - t[:, 0:1]) / a[:, None]).round().long().clamp(0, size[0] - 1)        # [N,w]
        sy = ((u[None, :] - t[:, 1:2]) / a[:, None]).round().long().clamp(0, size[1] - 1)        # [N,h]
        n = torch.arange(2, device=gpu)[:, None, None]
        mask = sil[n, sy[:, :, None], sx[:, None, :]].long()                                    # int64, as decode_keypoint's
        canvas = crop.uncrop_mask(mask, c["trans"], size)
        g = torch.Generator(device=gpu)
        g.manual_seed(3)
        refined, infos = icp.icp_refine(d_est, d["depth"], canvas, d["K"], d["pts"], d["faces"], depth_scale=1.0, generator=g,
                                        return_info=True)
        return {"trans": c["trans"], "mask": mask, "canvas": canvas, "refined": refined, "status": infos[1]["status"]}

    r = on_both_streams(chain)
    assert _same(r["canvas"], twin.uncrop_mask(r["mask"], r["trans"], size))
    s = _np(sil)
    grown = np.zeros_like(s)
    pitch = int(np.ceil(1.0 / r["trans"][:, 0, 0].min())) + 1
    for dy in range(-pitch, pitch + 1):
        for dx in range(-pitch, pitch + 1):
            grown |= np.roll(np.roll(s, dy, 1), dx, 2)
    assert r["canvas"].any() and not (r["canvas"].astype(bool) & ~grown).any()
    assert r["status"].tolist() == [0, 0] and np.isfinite(r["refined"]).all() and r["refined"].shape == (2, 3, 4)
