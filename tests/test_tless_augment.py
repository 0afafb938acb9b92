"""The T-LESS PVNet loader's training sample (clean_pvnet_amd.tless_augment, include/pvnet_vote.h, "T-LESS PVNet augmentation")
without a GPU: the module and its entry points exist and refuse bad arguments before any launch; what the host derives from the
draws equals the twin's values; the numpy twin of the contract (tests/tless_augment_twin.py) reproduces the reference's own code on
the fixtures of tests/golden/make_tless_augment_golden.py -- as bytes in the rotated sizes and matrices, the placements, both
canvases, the final image, the mask, the branch, ``visible``, ``pixel_num``, the box, ``center``, ``scale``, the magnified box, the
warped image and the warped mask; within derived bounds in ``trans_input``, the keypoints and the float image.  The GPU tests
(tests/test_gpu_tless_augment.py) then hold the device to the twin byte for byte."""
import os

import numpy as np
import pytest

from tests import capi, crop_twin
from tests import ct_augment_twin as ct
from tests import tless_augment_twin as twin
from tests.test_ct_augment import inp_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("tless_augment_mixed_30x50", "tless_augment_random_30x50")
SYMBOLS = {"pvv_tless_rotate_side", "pvv_tless_rotate", "pvv_tless_compose_workspace_bytes", "pvv_tless_compose",
           "pvv_tless_augment_workspace_bytes", "pvv_tless_augment"}
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def cases():
    """Each fixture (its two files) with the twin's results on it, computed once."""
    out = {}
    for name in FIXTURES:
        c = dict(np.load(os.path.join(GOLDEN, name + "_compose.npz")))
        c.update(np.load(os.path.join(GOLDEN, name + "_crop.npz")))
        c["fused_bg"] = twin.fused_backgrounds(c["bg"])
        c["compose"] = twin.compose(c["bg"], c["img"], c["mask"], c["kpt_2d"], c["other_img"], c["other_mask"], c["draws"], fused_bg=c["fused_bg"],
                                    num=c["num"], rot_max=c["rot_max"], ratio=float(c["ratio"]))
        c["kw"] = dict(input_size=tuple(int(v) for v in c["input_size"]), scale_train_ratio=tuple(c["scale_train_ratio"]),
                       box_train_ratio=tuple(c["box_train_ratio"]))
        k = c["compose"]
        c["augment"] = twin.augment(k["img"], k["mask"], k["kpt_2d"], k["bbox"], c["draws"], **c["kw"])
        out[name] = c
    return out


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import tless_augment as ta
    from clean_pvnet_amd.tless_augment import draws, rotate_image, tless_compose, tless_pvnet_augment, TlessPVNetAugment, COLUMNS
    assert all(callable(f) for f in (draws, rotate_image, tless_compose, tless_pvnet_augment, TlessPVNetAugment))
    assert COLUMNS == twin.COLUMNS and ta.N_SAMPLE == twin.N_SAMPLE == 14 and ta.PER_DISTRACTOR == twin.PER and ta.NORMAL_COLUMNS == twin.NORMAL_COLUMNS
    assert (ta.SCALE, ta.BOX, ta.TOP, ta.ROT, ta.DST_Y, ta.DST_X, ta.BLACK) == (twin.SCALE, twin.BOX, twin.TOP, twin.ROT, twin.DST_Y, twin.DST_X, twin.BLACK)
    from clean_pvnet_amd import ct_augment
    assert COLUMNS[3:10] == ct_augment.COLUMNS[3:10]                                # the colour columns lie where the detector's do
    assert ta.MAX_N == 16 and ta.CUT.itemsize == 112


def test_header_declares_and_library_exports_the_entry_points():
    raw = open(HEADER).read()
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in raw                                      # additive: the version did not move
    title = "T-LESS PVNet augmentation"
    assert title in raw and "#define PVV_TLESS_CUT_BYTES 112" in raw and "#define PVV_TLESS_MAX_N 16" in raw
    section = raw[raw.index(title):raw.index("Colour renders")]
    for cited in ("tless_train_utils.py", ":153-172", "tless_utils.py:86-97", "tless_train/pvnet.py", "tless_pvnet_utils.py", ":21-73", "data_utils.py"):
        assert cited in section


def test_draws_follow_torchs_generator(pkg):
    import torch
    from clean_pvnet_amd import tless_augment as ta
    torch.manual_seed(5)
    a = ta.draws(4, 6)
    torch.manual_seed(5)
    b = ta.draws(4, 6)
    c = ta.draws(4, 6, generator=torch.Generator().manual_seed(6))
    assert a.shape == (4, 14 + 18) and a.dtype == np.float64 and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    uni = np.delete(a, twin.NORMAL_COLUMNS, axis=1)
    assert ((uni >= 0) & (uni < 1)).all()
    normals = ta.draws(4000, 0, generator=torch.Generator().manual_seed(1))[:, list(twin.NORMAL_COLUMNS)]
    assert (normals < 0).any() and abs(normals.mean()) < 0.05 and abs(normals.std() - 1) < 0.05


# ------------------------------------------------------------------------------------------------ 1. the host's part
def test_the_plane_bounds_every_rotated_size_and_the_345_case_reaches_it(pkg):
    from clean_pvnet_amd import tless_augment as ta
    assert ta.rotate_side(12, 16) == twin.rotate_side(12, 16) == 20 and ta._lib.pvv_tless_rotate_side(12, 16) == 20
    M, bh, bw = twin.rotation(12, 16, twin.DEG_345)
    assert abs(M[0, 0] - 0.8) < 1e-15 and abs(M[0, 1] - 0.6) < 1e-15 and (bh, bw) == (19, 20)        # h s + w c = 20 lands on the integer: bound_w = D
    worst = 0
    for h, w in ((12, 16), (14, 18), (13, 17), (1, 1), (1, 40), (400, 400), (3, 4), (300, 400), (119, 120)):
        D = twin.rotate_side(h, w)
        assert D == ta._lib.pvv_tless_rotate_side(h, w) and D * D <= h * h + w * w < (D + 1) * (D + 1)
        degs = np.concatenate([np.linspace(0, 360, 721), np.degrees(np.arctan2(h, w)) + np.array([0, 90, 180, 270.]), np.degrees(np.arctan2(w, h)) + [0, 90.],
                               np.random.default_rng(h * w).random(200) * 360])
        for deg in degs:
            _, bh, bw = twin.rotation(h, w, deg)
            assert 0 <= bh <= D and 0 <= bw <= D, (h, w, deg, bh, bw, D)
            worst = max(worst, max(bh, bw) / D)
    assert worst == 1.0
    assert twin.rotation(14, 18, 0.)[1:] == (14, 18) and twin.rotation(14, 18, 180.)[1:] == (14, 18)
    M, bh, bw = twin.rotation(14, 18, 90.)
    assert 0 < abs(M[0, 0]) < 1e-16 and (bh, bw) == (18, 14)                                              # the |cos| ~ 6e-17 term does not reach the next integer


def test_cut_records_equal_the_twins_values(pkg):
    from clean_pvnet_amd import tless_augment as ta
    deg = np.concatenate([[0., 90., 180., 45., twin.DEG_345, 360.], np.random.default_rng(3).random(40) * 360]).reshape(2, 23)
    rec = ta.cut_records(13, 17, deg)
    assert rec.shape == (2, 23) and rec.dtype.itemsize == 112
    for i in np.ndindex(deg.shape):
        M, bh, bw = twin.rotation(13, 17, deg[i])
        assert rec["M"][i].tobytes() == M.tobytes() and (rec["bh"][i], rec["bw"][i]) == (bh, bw)
        assert rec["inv"][i].tobytes() == crop_twin.invert_affine(M).tobytes()
    d = twin.draws_for(5, 2, 4)
    cuts, u, flags = ta.host_block(d, 2, 14, 18, 13, 17, np.array([360., 0., 90., 360., 360.]))
    assert cuts.shape == (5, 3) and u.shape == (5, 3, 2) and flags.shape == (5, 2) and flags.dtype == np.int32
    assert cuts["M"][1, 0].tolist() == [1., 0., 0., -0., 1., 0.] and (cuts["bh"][1, 0], cuts["bw"][1, 0]) == (14, 18)      # rot_max 0: unrotated
    assert cuts["M"][2, 0].tobytes() == twin.rotation(14, 18, d[2, twin.ROT] * 90.)[0].tobytes()
    assert cuts["M"][3, 2].tobytes() == twin.rotation(13, 17, d[3, twin.N_SAMPLE + 3] * 360.)[0].tobytes()
    assert np.array_equal(u[:, 0], d[:, [twin.DST_Y, twin.DST_X]]) and np.array_equal(u[:, 2], d[:, twin.N_SAMPLE + 4:twin.N_SAMPLE + 6])
    assert np.array_equal(flags[:, 0], d[:, twin.TOP] < 0.5) and np.array_equal(flags[:, 1], d[:, twin.BLACK] >= 0.9)
    factor, ratio = ta.ratios(d, (1.8, 2.4), (1.0, 1.2))
    assert factor.dtype == F32 and ratio.dtype == F64
    for b in range(5):
        f, r = twin.ratios(d[b])
        assert factor[b].tobytes() == f.tobytes() and ratio[b] == r


def _meta(*shape, dtype=None):
    import torch
    return torch.empty(*shape, dtype=dtype or torch.uint8, device="meta")


def test_arguments_are_refused_before_any_launch(pkg):
    import torch
    from clean_pvnet_amd import tless_augment as ta
    d = twin.draws_for(2, 2, 1)
    z = lambda *s, dtype=torch.uint8: torch.zeros(*s, dtype=dtype)                 # noqa: E731
    host = (z(2, 16, 16, 3), z(2, 8, 8, 3), z(2, 8, 8), z(2, 3, 2, dtype=torch.float64), z(2, 2, 8, 8, 3), z(2, 2, 8, 8))
    with pytest.raises(RuntimeError, match="bg must be a CUDA tensor; there is no CPU fallback"):
        ta.tless_compose(*host, d)
    with pytest.raises(RuntimeError, match="img must be a CUDA tensor"):
        ta.tless_pvnet_augment(z(2, 16, 16, 3), z(2, 16, 16), z(2, 3, 2, dtype=torch.float64), z(2, 4, dtype=torch.int32), d)
    with pytest.raises(RuntimeError, match="img must be a CUDA tensor"):
        ta.rotate_image(z(2, 8, 8), np.zeros(2))
    with pytest.raises(RuntimeError, match="bg must be a CUDA tensor"):
        ta.TlessPVNetAugment()(*host)
    real_need, real_call = ta._native.need_cuda, ta._call

    def no_launch(*a):
        raise AssertionError("a launch was reached")
    ta._native.need_cuda, ta._call = (lambda *a: None), no_launch                  # past the device check
    try:
        bg, img, mask, kpt, oi, om = (_meta(2, 16, 16, 3), _meta(2, 8, 8, 3), _meta(2, 8, 8), _meta(2, 3, 2, dtype=torch.float64), _meta(2, 2, 8, 8, 3),
                                      _meta(2, 2, 8, 8))
        for ratio in (0, 0.0, -0.5, float("nan")):
            with pytest.raises(ValueError, match="ratio must be > 0"):
                ta.tless_compose(bg, img, mask, kpt, oi, om, d, ratio=ratio)
        with pytest.raises(ValueError, match="interp must be 'linear' or 'nearest'"):
            ta.tless_compose(bg, img, mask, kpt, oi, om, d, interp="cubic")
        with pytest.raises(TypeError, match="bg must be \\[B,H,W,3\\] uint8"):
            ta.tless_compose(_meta(2, 16, 16, 3, dtype=torch.float32), img, mask, kpt, oi, om, d)
        with pytest.raises(TypeError, match="mask and other_mask uint8 or bool"):
            ta.tless_compose(bg, img, _meta(2, 8, 8, dtype=torch.int64), kpt, oi, om, d)
        with pytest.raises(TypeError, match="kpt_2d float32 or float64"):
            ta.tless_compose(bg, img, mask, _meta(2, 3, 2, dtype=torch.int32), oi, om, d)
        with pytest.raises(ValueError, match="img must be \\[B = 2, h, w, 3\\] and mask"):
            ta.tless_compose(bg, img, _meta(2, 8, 7), kpt, oi, om, d)
        with pytest.raises(ValueError, match="other_img must be"):
            ta.tless_compose(bg, img, mask, kpt, _meta(3, 2, 8, 8, 3), _meta(3, 2, 8, 8), d)
        with pytest.raises(ValueError, match="kpt_2d must be \\[B = 2"):
            ta.tless_compose(bg, img, mask, _meta(2, 3, 3, dtype=torch.float64), oi, om, d)
        with pytest.raises(ValueError, match="N must lie in \\[0, 16\\]"):
            ta.tless_compose(bg, img, mask, kpt, _meta(2, 17, 8, 8, 3), _meta(2, 17, 8, 8), twin.draws_for(2, 17, 1))
        with pytest.raises(TypeError, match="fused_bg must be"):
            ta.tless_compose(bg, img, mask, kpt, oi, om, d, fused_bg=_meta(2, 16, 15, 3))
        with pytest.raises(TypeError, match="num must be \\[B = 2\\]"):
            ta.tless_compose(bg, img, mask, kpt, oi, om, d, num=_meta(3, dtype=torch.int64))
        with pytest.raises(ValueError, match="rot_max must be"):
            ta.tless_compose(bg, img, mask, kpt, oi, om, d, rot_max=np.zeros(3))
        bad = [d[:1], d[:, :19], d.astype(np.float32), np.where(np.arange(20) == 12, 1.0, d), np.where(np.arange(20) == 0, -0.1, d),
               np.where(np.arange(20) == 8, np.nan, d)]
        for draws in bad:
            with pytest.raises(ValueError, match="draws must|must lie in \\[0, 1\\)"):
                ta.tless_compose(bg, img, mask, kpt, oi, om, draws)
        cimg, cmask, box = _meta(2, 16, 16, 3), _meta(2, 16, 16), _meta(2, 4, dtype=torch.int32)
        with pytest.raises(TypeError, match="mask must be \\[2, 16, 16\\]"):
            ta.tless_pvnet_augment(cimg, _meta(2, 16, 15), kpt, box, d)
        with pytest.raises(TypeError, match="bbox must be \\[B = 2, 4\\] int32"):
            ta.tless_pvnet_augment(cimg, cmask, kpt, _meta(2, 4, dtype=torch.int64), d)
        with pytest.raises(TypeError, match="kpt_2d must be"):
            ta.tless_pvnet_augment(cimg, cmask, _meta(2, 3, dtype=torch.float64), box, d)
        with pytest.raises(ValueError, match="scale_train_ratio must be"):
            ta.tless_pvnet_augment(cimg, cmask, kpt, box, d, scale_train_ratio=(0.0, 1.0))
        with pytest.raises(ValueError, match="box_train_ratio must be"):
            ta.tless_pvnet_augment(cimg, cmask, kpt, box, d, box_train_ratio=(1.2, 1.0))
        with pytest.raises(ValueError, match="sides of input_size"):
            ta.tless_pvnet_augment(cimg, cmask, kpt, box, d, input_size=(0, 32))
        with pytest.raises(ValueError, match="draws must"):
            ta.tless_pvnet_augment(cimg, cmask, kpt, box, d[:, :13])
        with pytest.raises(TypeError, match="img must be \\[2\\] \\+ \\[h,w\\] or \\[h,w,3\\]"):
            ta.rotate_image(_meta(2, 8, 8, 4), np.zeros(2))
        with pytest.raises(TypeError, match="uint8 or bool"):
            ta.rotate_image(_meta(2, 8, 8, dtype=torch.float32), np.zeros(2))
        with pytest.raises(ValueError, match="deg must be finite"):
            ta.rotate_image(_meta(2, 8, 8), np.array([0., np.inf]))
        with pytest.raises(ValueError, match="interp must be"):
            ta.rotate_image(_meta(2, 8, 8), np.zeros(2), interp="area")
    finally:
        ta._native.need_cuda, ta._call = real_need, real_call


# ------------------------------------------------------------------------------------------------ 2. the twin against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_equals_the_reference_as_bytes(cases, name):
    c = cases[name]
    comp, aug, ran = c["compose"], c["augment"], c["ran"]
    B, N = len(ran), c["other_img"].shape[1]
    assert ran.sum() >= B - 1
    for b in np.flatnonzero(ran):
        used = [0] + [1 + n for n in range(N) if n < c["num"][b] and c["other_mask"][b, n].any()]
        degs = [c["draws"][b, twin.ROT] * c["rot_max"][b]] + [c["draws"][b, twin.N_SAMPLE + twin.PER * n] * 360. for n in range(N)]
        for j in used:                                                                                    # the rotated sizes and matrices
            src = c["mask"][b] if j == 0 else c["other_mask"][b, j - 1]
            M, bh, bw = twin.rotation(src.shape[0], src.shape[1], degs[j])
            assert (bh, bw) == tuple(c["ref_size"][b, j]) and M.tobytes() == c["ref_rot"][b, j].tobytes(), (name, b, j)
            assert tuple(comp["place"][b, j, 4:]) == tuple(c["ref_dst"][b, j]), (name, b, j)             # the placements
        for got, ref in (("train_img", "ref_train_img"), ("train_mask", "ref_train_mask"), ("fused_img", "ref_fused_img"), ("fused_mask", "ref_fused_mask"),
                         ("img", "ref_img"), ("mask", "ref_mask"), ("path", "ref_path"), ("bbox", "ref_bbox")):
            assert comp[got][b].dtype == c[ref][b].dtype and comp[got][b].tobytes() == c[ref][b].tobytes(), (name, b, got)
        assert comp["visible"][b, 1] == c["ref_visible"][b, 1]                                           # pixel_num
        assert comp["path"][b] == 0 or comp["visible"][b, 0] == c["ref_visible"][b, 0]                   # (on top by draw the reference does not count)
        assert aug["center"][b].tobytes() == c["ref_center"][b].tobytes() and aug["scale"][b].tobytes() == c["ref_scale"][b].tobytes()
        assert c["ref_scale"].dtype == F32 and c["ref_center"].dtype == F64
        for got, ref in (("box", "ref_box"), ("orig_img", "ref_orig"), ("mask", "ref_mask_out")):
            assert aug[got][b].dtype == c[ref][b].dtype and aug[got][b].tobytes() == c[ref][b].tobytes(), (name, b, got)
    assert set(comp["path"][ran].tolist()) >= {0, 1, 2} and (aug["mask"][ran].reshape(ran.sum(), -1) != 0).any(axis=1).all()


def kpt_bound(M, pts):
    """[K,2]: how far ``np.dot(pts, M[:, :2].T) + M[:, 2]`` may lie from ``(M00 x + M01 y) + M02`` evaluated in that order: 4 * 2^-53 of
    the magnitudes (``np.matmul`` may fuse or reorder the two products and the sum)."""
    x, y = np.abs(pts[:, 0]), np.abs(pts[:, 1])
    return 4 * 2.0 ** -53 * np.stack([np.abs(M[0, 0]) * x + np.abs(M[0, 1]) * y + np.abs(M[0, 2]), np.abs(M[1, 0]) * x + np.abs(M[1, 1]) * y + np.abs(M[1, 2])], 1)


@pytest.mark.parametrize("name", FIXTURES)
def test_transform_and_keypoints_agree_within_the_derived_bounds(cases, name):
    """``trans_input``: ct_augment_twin.trans_bound (the three-point solve's float32 source points against the closed form).  The
    keypoints: the rotation within ``kpt_bound``; the shift ``(k - min) + dst`` rounds twice on either side, so a difference e grows
    by at most one spacing of each intermediate; the crop's map adds |a| e, its own ``kpt_bound`` and what the two transforms'
    difference (lin, tr) moves a point by: lin (|x| + |y|) + tr."""
    c = cases[name]
    comp, aug = c["compose"], c["augment"]
    iw, ih = int(c["input_size"][1]), int(c["input_size"][0])
    worst = [0.0, 0.0, 0.0]
    for b in np.flatnonzero(c["ran"]):
        lin, tr = ct.trans_bound(aug["center"][b], aug["scale"][b], (iw, ih))
        diff = np.abs(aug["trans_input"][b] - c["ref_trans_input"][b])
        assert diff[:, :2].max() <= lin and diff[:, 2].max() <= tr, (name, b, diff, lin, tr)
        worst[0] = max(worst[0], diff[:, :2].max() / lin, diff[:, 2].max() / tr)
        M = c["ref_rot"][b, 0]
        e1 = kpt_bound(M, c["kpt_2d"][b])
        rec = comp["place"][b, 0]
        mid = c["ref_kpt_rotated"][b] - np.array([rec[1], rec[0]], F64)
        e2 = e1 + np.spacing(np.abs(mid) + e1) + np.spacing(np.abs(c["ref_kpt_composed"][b]) + e1)
        d2 = np.abs(comp["kpt_2d"][b] - c["ref_kpt_composed"][b])
        assert (d2 <= e2).all(), (name, b, d2, e2)
        T = aug["trans_input"][b]
        k = c["ref_kpt_composed"][b]
        e3 = np.abs(T[0, 0]) * e2 + kpt_bound(T, k) + (lin * (np.abs(k[:, 0]) + np.abs(k[:, 1])) + tr)[:, None]
        d3 = np.abs(aug["kpt_2d"][b] - c["ref_kpt"][b])
        assert (d3 <= e3).all(), (name, b, d3, e3)
        worst[1], worst[2] = max(worst[1], (d2 / e2).max()), max(worst[2], (d3 / e3).max())
    print("%s: observed / bound: trans %.3g, composed keypoints %.3g, final keypoints %.3g" % (name, *worst))


@pytest.mark.parametrize("name", FIXTURES)
def test_inp_agrees_with_the_reference_within_the_derived_bound(cases, name):
    """The bound tests/test_ct_augment.py derives for the grey mean (numpy's float32 pairwise mean against the fixed binary64 tree),
    here over the blanked image."""
    c = cases[name]
    got, ref = c["augment"]["inp"], c["ref_inp"]
    assert ref.dtype == F32 and got.shape == ref.shape
    n = got.shape[2] * got.shape[3]
    worst = 0.0
    for b in np.flatnonzero(c["ran"]):
        bound = inp_bound(c["draws"][b], n, ct.grey_mean(c["augment"]["orig_img"][b]), ref[b])
        diff = float(np.abs(got[b] - ref[b]).max())
        worst = max(worst, diff / bound)
        assert diff <= bound, (name, b, diff, bound)
    print("%s: inp observed / bound = %.3g" % (name, worst))


# ------------------------------------------------------------------------------------------------ 3. the required cases
def test_the_mixed_fixture_holds_the_required_cases(cases):
    c = cases["tless_augment_mixed_30x50"]
    comp, aug, d = c["compose"], c["augment"], c["draws"]
    i = {name: k for k, name in enumerate(twin.MIXED_CASES)}
    assert len(c["ran"]) == len(twin.MIXED_CASES) and not c["ran"][i["an empty target"]] and c["ran"].sum() == len(i) - 1
    sizes = {name: tuple(c["ref_size"][i[name], 0]) for name in ("angle 0", "angle 90", "angle 180", "angle 45", "3-4-5")}
    assert sizes == {"angle 0": (12, 16), "angle 90": (16, 12), "angle 180": (12, 16), "angle 45": (19, 19), "3-4-5": (19, 20)}
    assert twin.rotate_side(12, 16) == 20
    b = i["angle 0"]
    assert comp["place"][b, 0, 2] == np.ptp(np.nonzero(c["mask"][b])[0]) and comp["place"][b, 0, 3] == np.ptp(np.nonzero(c["mask"][b])[1])
    assert comp["path"][i["on top by draw"]] == 0 and d[i["on top by draw"], twin.TOP] < 0.5
    want = {"occluded and kept": (1, 14), "ratio met exactly": (1, 12), "just below the ratio": (2, 11), "fully occluded": (2, 0)}
    for name, (path, visible) in want.items():
        assert (comp["path"][i[name]], tuple(comp["visible"][i[name]])) == (path, (visible, 16)), name
    assert 12 / 16 == float(c["ratio"])                                                                   # exactly the ratio: kept, the test is strict
    assert (comp["mask"][i["ratio met exactly"]] != 0).sum() == 12 and (comp["mask"][i["fully occluded"]] != 0).sum() == 16
    b = i["black fused background"]
    assert d[b, twin.BLACK] >= 0.9 and not comp["fused_img"][b][comp["fused_mask"][b] == 0].any() and not comp["img"][b][(comp["mask"][b] == 0) & (comp["fused_mask"][b] == 0)].any()
    b = i["num = 0"]
    assert c["num"][b] == 0 and (comp["place"][b, 1:, 2] == -1).all() and not comp["fused_mask"][b].any()
    b = i["an empty distractor"]
    assert tuple(comp["place"][b, 1]) == (0, 0, -1, -1, 0, 0) and comp["place"][b, 2, 2] >= 0
    b = i["an empty target"]
    assert comp["path"][b] == 3 and comp["bbox"][b].tolist() == [0, 0, 49, 29] and not comp["mask"][b].any() and comp["visible"][b].tolist() == [0, 0]
    assert comp["img"][b].tobytes() == comp["fused_img"][b].tobytes()
    b = i["the target touches its cut-out's border"]
    assert tuple(comp["place"][b, 0, :4]) == (0, 0, 11, 15) and c["mask"][b].max() == 255 and comp["visible"][b, 1] == 255 * (12 * 6 + 1)
    assert comp["visible"][:, 1].max() > 255 * 16                                                        # pixel_num sums the values, not the pixels
    b = i["the box clips"]
    assert aug["box"][b].tolist() == [0, 0, 31, 23]
    T, (x0, y0, x1, y1), r = aug["trans_input"][b], comp["bbox"][b], twin.ratios(d[b], **{k: c["kw"][k] for k in ("scale_train_ratio", "box_train_ratio")})[1]
    px, py = np.array([x0, x1]) * T[0, 0] + T[0, 2], np.array([y0, y1]) * T[1, 1] + T[1, 2]
    raw = np.rint(np.concatenate([(px - px.mean()) * r + px.mean(), (py - py.mean()) * r + py.mean()]))
    assert raw[0] < 0 and raw[1] > 31 and raw[2] < 0 and raw[3] > 23                                     # all four sides clip
    b = i["a tie in np.round"]
    assert aug["scale"][b].tolist() == [32., 32.] and aug["box"][b].tolist() == [8, 10, 24, 14] and aug["center"][b].tolist() == [8.5 + comp["place"][b, 0, 5] - 1, 22.5]
    assert np.rint(8.5) == 8 and np.rint(23.5) == 24                                                     # half to even, both ways


def test_a_rotated_cutout_larger_than_the_canvas_is_placed_at_zero():
    bg, img, mask, kpt, oi, om, d, kw = twin.oversize_batch()
    out = twin.compose(bg, img, mask, kpt, oi, om, d, **kw)
    assert bg.shape[1:3] == (10, 12) and (out["place"][0, :, 2] > 10).all() and (out["place"][0, :, 3] > 12).all() and not out["place"][0, :, 4:].any()
    assert out["path"][0] in (1, 2) and out["mask"].any()


def test_nearest_and_linear_differ_and_bool_masks_count_pixels():
    bg, img, mask, kpt, oi, om, d = twin.batch(2, 7)
    lin = twin.compose(bg, img, mask, kpt, oi, om, d)
    near = twin.compose(bg, img, mask, kpt, oi, om, d, interp="nearest")
    assert lin["img"].tobytes() != near["img"].tobytes()
    as_bool = twin.compose(bg, img, mask != 0, kpt, oi, om != 0, d, interp="nearest")
    assert as_bool["visible"][0, 1] == (twin.rotate((mask[0] != 0).astype(np.uint8), d[0, twin.ROT] * 360., "nearest")[0] != 0).sum()
    assert as_bool["img"][0].tobytes() == near["img"][0].tobytes() and mask[0].max() == 1         # (a mask of 255 has another pixel_num: D:74)
