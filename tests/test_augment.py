"""PVNet's augmentation and loader transforms (clean_pvnet_amd.augment, include/pvnet_vote.h, "Training augmentation") without a GPU: the
module and its entry points exist and refuse bad arguments before any launch; the numpy twin of the contract
(tests/augment_twin.py) reproduces the reference's own control flow on the fixtures of tests/golden/make_augment_golden.py, its
colour jitter is PIL's byte for byte, its fixed-point resampling and blur stay within derived bounds of plain binary64
samplers, and the degenerate cases take the stated paths.  The GPU tests (tests/test_gpu_augment.py) then hold the device to
the twin byte for byte."""
import os

import numpy as np
import pytest

from tests import augment_twin as twin
from tests import capi, crop_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("augment_mixed_40x66", "augment_mixed_44x40", "augment_defaults_40x66")
SYMBOLS = {"pvv_augment_workspace_bytes", "pvv_pvnet_augment", "pvv_transform_workspace_bytes", "pvv_pvnet_transform"}
FACTORS = (0.0, 0.5, 0.9, 0.95, 1.0, 1.05, 1.1, 1.5, 2.0)          # the extremes and the middle of the reference's and of wide ranges
HUES = (-0.5, -0.05, 0.0, 0.05, 0.5)


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import augment
    assert all(callable(getattr(augment, f)) for f in ("draws", "pvnet_augment", "pvnet_transform", "PVNetAugment"))
    assert augment.ORDERS == twin.ORDERS and augment.BLUR_TAPS == twin.BLUR_TAPS and augment.MEAN == twin.MEAN and augment.STD == twin.STD
    assert [augment.blur_taps(k)[4 - k // 2:5 + k // 2] for k in (3, 5, 7, 9)] == [twin.blur_taps(k) for k in (3, 5, 7, 9)]
    assert sum(twin.blur_taps(9)) == 256 and twin.blur_taps(9) == twin.blur_taps(9)[::-1]


def test_header_declares_and_library_exports_the_entry_points():
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in open(HEADER).read()                      # additive: the version did not move


def test_draws_follow_torchs_generator(pkg):
    import torch
    from clean_pvnet_amd import augment
    torch.manual_seed(5)
    a = augment.draws(4)
    torch.manual_seed(5)
    b = augment.draws(4)
    c = augment.draws(4, generator=torch.Generator().manual_seed(6))
    assert a.shape == (4, 12) and a.dtype == np.float64 and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert ((a >= 0) & (a < 1)).all()


def test_host_blocks_equal_the_twins_values(pkg):
    from clean_pvnet_amd import augment
    d = twin.draws_for(40, 3)
    g = augment.geometry_params(d, (40, 66), [-30.0, 30.0], [0.8, 1.2])
    j = augment.jitter_params(d, 0.5, [0.1, 0.1, 0.05, 0.05])
    for b, u in enumerate(d):
        cs, sn = twin.cos_sin(twin.degree_of(u[0]))
        ratio = twin.uniform(0.8, 1.2, u[1])
        assert (g[b]["cos"], g[b]["sin"], g[b]["ratio"], g[b]["th"], g[b]["tw"]) == (cs, sn, ratio, int(40 * ratio), int(66 * ratio))
        k, f, ops = twin.jitter_of(u)
        assert j[b]["k"] == k and [op for op in j[b]["order"] if op >= 0] == ops and j[b]["hue"] == twin.hue_shift(f[3])
        assert j[b]["f"].tobytes() == np.array(f[:3], np.float32).tobytes()
        assert not k or list(j[b]["w"][4 - k // 2:5 + k // 2]) == twin.blur_taps(k)
    assert {int(k) for k in j["k"]} == {0, 3, 5, 7, 9}


def _meta(*shape, dtype=None):
    import torch
    return torch.empty(*shape, dtype=dtype or torch.float32, device="meta")


def test_arguments_are_refused_before_any_launch(pkg):
    import torch
    from clean_pvnet_amd import augment
    u8 = torch.uint8
    d = twin.draws_for(2, 1)
    with pytest.raises(RuntimeError, match="img must be a CUDA tensor; there is no CPU fallback"):
        augment.pvnet_augment(torch.zeros(2, 16, 16, 3, dtype=u8), torch.zeros(2, 16, 16, dtype=u8), torch.zeros(2, 9, 2), (8, 8), d)
    with pytest.raises(RuntimeError, match="img must be a CUDA tensor"):
        augment.pvnet_transform(torch.zeros(2, 16, 16, 3, dtype=u8), d, mean=twin.MEAN, std=twin.STD)
    real_need, real_call = augment._native.need_cuda, augment._call

    def no_launch(*a):
        raise AssertionError("a launch was reached")
    augment._native.need_cuda, augment._call = (lambda *a: None), no_launch             # past the device check
    try:
        img, mask, kpt = _meta(2, 16, 16, 3, dtype=u8), _meta(2, 16, 16, dtype=u8), _meta(2, 9, 2)
        with pytest.raises(TypeError, match="img must be \\[B,H,W,3\\] uint8"):
            augment.pvnet_augment(_meta(2, 16, 16, 3), mask, kpt, (8, 8), d)
        with pytest.raises(TypeError, match="mask must be uint8 or bool"):
            augment.pvnet_augment(img, _meta(2, 16, 16, dtype=torch.int64), kpt, (8, 8), d)
        with pytest.raises(TypeError, match="kpt_2d must be float32 or float64"):
            augment.pvnet_augment(img, mask, _meta(2, 9, 2, dtype=torch.float16), (8, 8), d)
        with pytest.raises(ValueError, match="mask must be \\[2, 16, 16\\]"):
            augment.pvnet_augment(img, _meta(2, 16, 15, dtype=u8), kpt, (8, 8), d)
        with pytest.raises(ValueError, match="kpt_2d must be"):
            augment.pvnet_augment(img, mask, _meta(3, 9, 2), (8, 8), d)
        for size in ((7, 8), (8, 7), (8, 16385)):
            with pytest.raises(ValueError, match="out_size sides must lie in \\[8, 16384\\]"):
                augment.pvnet_augment(img, mask, kpt, size, d)
        bad = [d[:1], d[:, :11], d.astype(np.float32), np.where(np.arange(12) == 3, 1.0, d), np.where(np.arange(12) == 0, -0.1, d),
               np.where(np.arange(12) == 5, np.nan, d)]
        for table in bad:
            with pytest.raises(ValueError, match="draws must"):
                augment.pvnet_augment(img, mask, kpt, (8, 8), table)
            with pytest.raises(ValueError, match="draws must"):
                augment.pvnet_transform(img, table, mean=twin.MEAN, std=twin.STD)
        with pytest.raises(ValueError, match="overlap_ratio"):
            augment.pvnet_augment(img, mask, kpt, (8, 8), d, overlap_ratio=1.5)
        with pytest.raises(ValueError, match="rotate and resize_ratio"):
            augment.pvnet_augment(img, mask, kpt, (8, 8), d, resize_ratio=(0.0, 1.0))
        with pytest.raises(ValueError, match="gives a window"):
            augment.pvnet_augment(img, mask, kpt, (8, 8), d, resize_ratio=(0.01, 0.02))
        with pytest.raises(TypeError, match="img must be \\[B,H,W,3\\] uint8"):
            augment.pvnet_transform(_meta(2, 3, 16, 16, dtype=u8), d, mean=twin.MEAN, std=twin.STD)
        with pytest.raises(ValueError, match="sides must be at least 8"):
            augment.pvnet_transform(_meta(2, 7, 16, 3, dtype=u8), d, mean=twin.MEAN, std=twin.STD)
        with pytest.raises(ValueError, match="jitter must be"):
            augment.pvnet_transform(img, d, jitter=(0.1, 0.1, 0.05, 0.6), mean=twin.MEAN, std=twin.STD)
        with pytest.raises(ValueError, match="jitter must be"):
            augment.pvnet_transform(img, d, jitter=(-0.1, 0.1, 0.05, 0.05), mean=twin.MEAN, std=twin.STD)
        with pytest.raises(ValueError, match="blur_prob"):
            augment.pvnet_transform(img, d, blur_prob=1.5, mean=twin.MEAN, std=twin.STD)
    finally:
        augment._native.need_cuda, augment._call = real_need, real_call


# ------------------------------------------------------------------------------------------------ 1. the reference's control flow
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_reproduces_the_references_control_flow(name):
    """``img``, ``mask``, the branch and ``ToTensor`` + ``Normalize`` as bytes.  ``kpt_2d``: the reference's ``np.matmul`` may fuse
    or reorder the three products of a row, each order rounding at most three times at magnitudes <= |M00 x| + |M01 y| + |M02|,
    against the twin's two: the bound is 4 * 2^-53 * that sum; the subtraction of the window, the addition of the pad and the
    division by the ratio are the same operations on both sides, so the difference only passes through the division."""
    c = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    kw = dict(rotate=tuple(c["rotate"]), overlap_ratio=float(c["overlap_ratio"]), resize_ratio=tuple(c["resize_ratio"]))
    out_size = tuple(int(v) for v in c["out_size"])
    got = twin.pvnet_augment(c["img"], c["mask"], c["kpt_2d"], out_size, c["draws"], **kw)
    assert got["img"].shape == c["ref_img"].shape and got["img"].tobytes() == c["ref_img"].tobytes()
    assert got["mask"].shape == c["ref_mask"].shape and got["mask"].tobytes() == c["ref_mask"].tobytes()
    assert (np.minimum(got["path"], 1) == c["ref_path"]).all() and set(c["ref_path"]) == {0, 1} and (got["path"] != 2).all()
    assert twin.pvnet_transform(got["img"], None).tobytes() == c["ref_inp"].tobytes() and c["ref_inp"].dtype == np.float32
    worst = 0.0
    for b in range(len(c["img"])):
        x, y = c["kpt_2d"][b, :, 0], c["kpt_2d"][b, :, 1]
        if got["path"][b] != 1:
            assert got["kpt_2d"][b].tobytes() == c["kpt_2d"][b].tobytes() == c["ref_kpt_2d"][b].tobytes()
            continue
        ys, xs = np.nonzero(c["mask"][b])
        M = twin.getRotationMatrix2D((xs.mean(), ys.mean()), twin.degree_of(c["draws"][b, 0], kw["rotate"]), 1)
        ratio = twin.uniform(kw["resize_ratio"][0], kw["resize_ratio"][1], c["draws"][b, 1])
        for row, col in ((0, 0), (1, 1)):
            bound = 4 * 2.0 ** -53 * (np.abs(M[row, 0] * x) + np.abs(M[row, 1] * y) + abs(M[row, 2])) / ratio
            err = np.abs(got["kpt_2d"][b, :, col] - c["ref_kpt_2d"][b, :, col])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all()
    print("%s: the keypoints use at most %.2f of their bound" % (name, worst))


# ------------------------------------------------------------------------------------------------ 2. the jitter against PIL
def _sweep():
    """[1037, 256, 3]: a 64^3 lattice with 0 and 255 among its levels (2^18 colours, the cube's corners among them), all greys, and
    the cube's twelve edges at all 256 levels."""
    lv = np.round(np.linspace(0, 255, 64)).astype(np.uint8)
    lattice = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)
    g = np.arange(256, dtype=np.uint8)
    edges = []
    for axis in range(3):
        for a in (0, 255):
            for b in (0, 255):
                e = np.zeros((256, 3), np.uint8)
                e[:, axis], e[:, (axis + 1) % 3], e[:, (axis + 2) % 3] = g, a, b
                edges.append(e)
    colours = np.concatenate([lattice, np.stack([g, g, g], 1)] + edges)
    assert len(lattice) == 1 << 18 and len(colours) % 256 == 0
    return colours.reshape(-1, 256, 3)


def _pil_enhance(img, op, f):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(img)
    if op == twin.HUE:                                                             # torchvision's adjust_hue on a PIL image
        h, s, v = im.convert("HSV").split()
        np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + (int(f * 255) & 255)).astype(np.uint8)
        return np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
    enhancer = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
    return np.asarray(enhancer(im).enhance(f))


def test_hsv_round_trip_is_pils_on_every_colour():
    from PIL import Image
    sweep = _sweep()
    hsv = np.asarray(Image.fromarray(sweep).convert("HSV"))
    assert twin.rgb2hsv(sweep).tobytes() == hsv.tobytes()
    every = np.stack(np.meshgrid(*[np.arange(256, dtype=np.uint8)] * 3, indexing="ij"), -1).reshape(4096, 4096, 3)[::3]   # as HSV triples
    assert twin.hsv2rgb(every).tobytes() == np.asarray(Image.fromarray(every, "HSV").convert("RGB")).tobytes()


@pytest.mark.parametrize("op", [twin.BRIGHTNESS, twin.CONTRAST, twin.SATURATION, twin.HUE])
def test_each_jitter_operation_is_pils_on_the_colour_sweep(op):
    sweep = _sweep()
    for f in (HUES if op == twin.HUE else FACTORS):
        got, want = twin.enhance(sweep, op, f), _pil_enhance(sweep, op, f)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (op, f, int((got != want).sum()))


def test_all_24_orders_are_pils_on_one_image():
    img = twin.image(5, 40, 66)
    amp = (0.4, 0.4, 0.4, 0.5)
    seen = set()
    for i in range(24):
        u = twin.draws_for(1, 100 + i)[0]
        u[4], u[10] = 0.9, (i + 0.5) / 24
        k, f, ops = twin.jitter_of(u, jitter=amp)
        assert k == 0 and tuple(ops) == twin.ORDERS[i]
        seen.add(tuple(ops))
        want = img
        for op in ops:
            want = _pil_enhance(want, op, f[op])
        assert twin.transform_one(img, u, jitter=amp, u8=True).tobytes() == want.tobytes(), ops
    assert len(seen) == 24


def test_contrast_mean_on_a_half_boundary():
    from PIL import Image, ImageStat
    img = twin.contrast_boundary_image()
    assert ImageStat.Stat(Image.fromarray(img).convert("L")).mean[0] == 100.5 and twin.contrast_grey(img) == 101
    for f in FACTORS:
        assert twin.enhance(img, twin.CONTRAST, f).tobytes() == _pil_enhance(img, twin.CONTRAST, f).tobytes()


# ------------------------------------------------------------------------------------------------ 3. the resampling and the blur
def _half_ulp_f32(v):
    return 2.0 ** (int(np.ceil(np.log2(v))) - 24)


def _rotate_bound(D):
    """the final rounding, and per axis a coordinate off by 1/64 + 1/1024 on a surface of slope <= D."""
    return 0.5 + 2 * D * (1 / 64 + 1 / 1024)


def _resize_bound(D, side):
    """The final rounding; per axis two 11-bit weights, each off by at most 0.5 + 2^-12 units of 1/2048 (rint, and the float32
    ``1 - f``) on taps that sum to at most 510, the row pass's error then passing through column weights that sum to at most
    2049/2048; per axis a float32 coordinate off by half a unit in the last place on a surface of slope <= D."""
    return 0.5 + 2 * (510 * (0.5 + 2.0 ** -12) / 2048) * (2049 / 2048) + 2 * D * _half_ulp_f32(side)


def test_fixed_point_resampling_against_binary64_samplers():
    img = twin.image(1)
    H, W = img.shape[:2]
    D = crop_twin.neighbour_difference(img)
    worst = {"rotate": 0.0, "resize": 0.0, "chain": 0.0}
    for deg in (-30.0, -7.3, 12.9, 30.0):
        M = twin.getRotationMatrix2D((33.7, 22.1), deg, 1)
        rot, rot64 = twin.warpAffine(img, M, (W, H)), twin.rotate_f64(img, M)
        worst["rotate"] = max(worst["rotate"], float(np.abs(rot - rot64).max()))
        for size in ((66, 40), (84, 57), (53, 37), (70, 48)):
            out = twin.resize(rot, size).astype(np.float64)
            worst["resize"] = max(worst["resize"], float(np.abs(out - twin.resize_f64(rot, size)).max()))
            worst["chain"] = max(worst["chain"], float(np.abs(out - twin.resize_f64(rot64, size)).max()))
    b_rot, b_res = _rotate_bound(D), _resize_bound(255, max(H, W))
    b_chain = b_res + b_rot * (2049 / 2048) ** 2                               # the first stage's error through the second's weights
    print("D = %d: rotate worst %.4f bound %.4f; resize worst %.4f bound %.4f; chain worst %.4f bound %.4f"
          % (D, worst["rotate"], b_rot, worst["resize"], b_res, worst["chain"], b_chain))
    assert 0 < worst["rotate"] <= b_rot and 0 < worst["resize"] <= b_res and 0 < worst["chain"] <= b_chain


def test_resize_to_the_same_size_is_the_identity():
    img = twin.image(2)
    assert twin.resize(img, (70, 48)).tobytes() == img.tobytes()
    assert twin.resize(img[..., 0], (70, 48), twin.INTER_NEAREST).tobytes() == img[..., 0].tobytes()


@pytest.mark.parametrize("shape", [(12, 9), (40, 66)])
def test_blur_against_a_binary64_convolution(shape):
    """The row pass is exact in integers; the column pass rounds once: at most half a grey level (and binary64's own rounding)."""
    img = twin.image(3, *shape)
    for k in (3, 5, 7, 9):
        got, want = twin.blur(img, k), twin.blur_f64(img, k)
        worst = float(np.abs(got - want).max())
        print("%s k = %d: worst %.4f" % (shape, k, worst))
        assert 0 < worst <= 0.5 + 1e-9 and (got != img).any()
    flat = np.full(shape + (3,), 77, np.uint8)
    assert all(twin.blur(flat, k).tobytes() == flat.tobytes() for k in (3, 5, 7, 9))          # the weights sum to 256


# ------------------------------------------------------------------------------------------------ 4. degenerate cases
def _one(mask, out_size, u, **kw):
    H, W = mask.shape
    img, kpt = twin.image(9, H, W), twin.keypoints(mask, 9, 4)
    o = twin.augment_one(img, mask, kpt, out_size, u, **kw)
    assert o[0].shape == tuple(out_size) + (3,) and o[1].shape == tuple(out_size) and o[0].dtype == o[1].dtype == np.uint8
    assert o[2].shape == (9, 2) and o[2].dtype == np.float64 and np.isfinite(o[2]).all()
    return img, kpt, o


def test_an_empty_randint_range_gives_its_lower_end():
    """A two-row object at the top: hmin + 0.8 * fh = 0.8, so hrmax = hrmin = 0, where the reference's randint raises."""
    mask = twin.blob(48, 70, 0, 2, 30, 40)
    u = twin.draws_for(1, 2)[0]
    img, kpt, (o_img, o_mask, o_kpt, path, win) = _one(mask, (40, 66), u, rotate=(0, 0), resize_ratio=(1.0, 1.0))
    assert path == 1 and win.tolist()[:3] == [40, 66, 0] and win.tolist()[4:] == [0, 0]
    wbeg = int(win[3])
    assert o_img.tobytes() == img[0:40, wbeg:wbeg + 66].tobytes() and o_mask.tobytes() == mask[0:40, wbeg:wbeg + 66].tobytes()
    assert np.array_equal(o_kpt, kpt - [wbeg, 0])


def test_single_pixel_and_border_masks_keep_keypoints_on_the_object():
    """The keypoint that sits on the object's centre lands on the output mask's centre: the image and the keypoints move together."""
    for mask in (twin.blob(48, 70, 25, 26, 37, 38), twin.blob(48, 70, 0, 9, 0, 12), twin.blob(48, 70, 40, 48, 58, 70)):
        for seed in range(6):
            u = twin.draws_for(1, 40 + seed)[0]
            H, W = mask.shape
            ys, xs = np.nonzero(mask)
            kpt = np.array([[xs.mean(), ys.mean()]] * 9)
            o_img, o_mask, o_kpt, path, win = twin.augment_one(twin.image(9, H, W), mask, kpt, (40, 66), u)
            assert path == 1 and o_mask.any()
            oy, ox = np.nonzero(o_mask)
            inside = (0 <= o_kpt[0, 0] < 66) and (0 <= o_kpt[0, 1] < 40)
            if inside and len(xs) == 1:
                assert abs(ox.mean() - o_kpt[0, 0]) <= 1.5 and abs(oy.mean() - o_kpt[0, 1]) <= 1.5
            th, tw, hbeg, wbeg, ph, pw = win.tolist()
            assert 0 <= hbeg <= max(H - th, 0) and 0 <= wbeg <= max(W - tw, 0)


def test_pad_on_one_axis_only():
    for out_size, rows in (((40, 66), False), ((44, 40), True)):
        img, mask, kpt, d = twin.mixed_batch(out_size)
        o = twin.augment_one(img[2], mask[2], kpt[2], out_size, d[2], **twin.MIXED_KW)
        th, tw, hbeg, wbeg, ph, pw = o[4].tolist()
        assert (th >= 48, tw >= 70) == (rows, not rows)
        assert (ph, pw) == ((th - 48) // 2 if rows else 0, 0 if rows else (tw - 70) // 2) and (hbeg == 0 if rows else wbeg == 0)


def test_empty_mask_and_empty_rotated_mask():
    u = twin.draws_for(1, 6)[0]
    empty = np.zeros((48, 70), np.uint8)
    img, kpt, (o_img, o_mask, o_kpt, path, win) = _one(empty, (40, 66), u)
    th, tw, hbeg, wbeg, ph, pw = win.tolist()
    assert path == 0 and (th, tw, ph, pw) == (40, 66, 0, 0) and (hbeg, wbeg) == (int(u[2] * 8), int(u[3] * 4))
    assert o_img.tobytes() == img[hbeg:hbeg + 40, wbeg:wbeg + 66].tobytes() and not o_mask.any() and np.array_equal(o_kpt, kpt)
    img, kpt, (o_img, o_mask, o_kpt, path, win) = _one(empty, (56, 80), u)                      # pad on both axes, centred
    assert path == 0 and win.tolist() == [56, 80, 0, 0, 4, 5] and o_img[4:52, 5:75].tobytes() == img.tobytes()
    assert not o_img[:4].any() and not o_img[52:].any() and not o_img[:, :5].any() and not o_img[:, 75:].any()
    m2, u2 = twin.empty_rotation_case()
    img, kpt, (o_img, o_mask, o_kpt, path, win) = _one(m2, (40, 66), u2)
    hbeg, wbeg = int(win[2]), int(win[3])
    assert path == 2 and o_img.tobytes() == img[hbeg:hbeg + 40, wbeg:wbeg + 66].tobytes() and np.array_equal(o_kpt, kpt)
    assert o_mask.tobytes() == m2[hbeg:hbeg + 40, wbeg:wbeg + 66].tobytes()
