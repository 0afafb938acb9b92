"""Detector decode, crops and the way back (include/pvnet_vote.h's last section, clean_pvnet_amd.crop) without a GPU: the module
and its five entry points exist, the numpy twin of the contracts (tests/crop_twin.py) reproduces the reference's own
``decode_ct_hm`` on the fixtures of tests/golden/make_crop_golden.py bit for bit, its tie and short-count rules, its fixed-point
warp against a plain binary64 bilinear sampler, and the two ways back against what they invert.  The GPU tests
(tests/test_gpu_crop.py) then hold the device to the twin bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from tests import capi
from tests import crop_twin as twin
from tests import tolerances as tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("crop_ct_small", "crop_ct_seams", "crop_ct_full")
SYMBOLS = {"pvv_ct_decode", "pvv_ct_workspace_bytes", "pvv_crop_boxes", "pvv_uncrop_keypoints", "pvv_uncrop_mask"}
KW = dict(scale_ratio=twin.SCALE_RATIO, mean=twin.MEAN, std=twin.STD)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import crop
    assert crop.MAX_K == twin.MAX_K
    assert all(callable(getattr(crop, f)) for f in ("decode_ct_hm", "crop_boxes", "uncrop_keypoints", "uncrop_mask"))


def test_header_declares_and_library_exports_the_five_entry_points():
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in open(HEADER).read()                      # additive: the version did not move


def test_host_side_argument_checks():
    L = capi.load()
    up = lambda n: (n + 255) // 256 * 256                                          # noqa: E731
    # 135 x 180 = 5 x 6 tiles, 30 classes: 900 lists of 100 keys, then 29
    assert L.pvv_ct_workspace_bytes(1, 30, 135, 180, 100) == up(900 * 100 * 8) + up(29 * 100 * 8)
    assert L.pvv_ct_workspace_bytes(1, 1, 8, 8, 257) == 0 and b"PVV_CT_MAX_K" in L.pvv_last_error()
    assert L.pvv_ct_workspace_bytes(1, 1, 2, 2, 5) == 0 and b"H*W" in L.pvv_last_error()
    assert L.pvv_ct_workspace_bytes(1, 1 << 20, 64, 64, 5) == 0 and b"2^31" in L.pvv_last_error()
    assert L.pvv_ct_decode(None, None, 1, 1, 8, 8, 5, 1, None, 0, None, None, None, None) == -1          # NULL before any launch
    assert L.pvv_crop_boxes(None, 1, 8, 8, None, None, 1, 32, 32, ctypes.c_double(1.2), 0, ctypes.c_double(0), None, None, None, 0,
                            None, None, None, None, None, None) == -1
    assert L.pvv_uncrop_keypoints(None, 0, None, 1, 9, None, None) == -1
    assert L.pvv_uncrop_mask(None, 4, 8, 8, None, 1, 8, 8, None, None) == -1 and b"mask_elem_size" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 1. the twin against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_reproduces_the_reference_fixture(name):
    c = load(name)
    hm, wh = twin.regenerate(c)
    assert tuple(hm.shape) == tuple(c["shape"])
    K = int(c["K"])
    for clip, want in ((False, c["ref_detection"]), (True, c["ref_detection_clip"])):
        ct, det, count = twin.decode_ct_hm(hm, wh, K=K, clip=clip)
        np.testing.assert_array_equal(_bits32(det), _bits32(want))                # all six columns
        np.testing.assert_array_equal(_bits32(ct), _bits32(c["ref_ct"]))
        np.testing.assert_array_equal(count, c["count"])
    assert (c["ref_detection_clip"] != c["ref_detection"]).any()                  # the clip is exercised


def test_seams_fixture_holds_the_cases_the_checks_need():
    c = load("crop_ct_seams")
    hm = c["ct_hm"]
    _, C, H, W = hm.shape
    assert H > 2 * 32 and W > 2 * 32 and H % 32 and W % 32                         # 3 x 3 tiles, neither side a multiple
    pk = twin.peaks(hm[0]) & (hm[0] >= np.float32(0.55))
    for s in (32, 64):
        assert pk[:, :, s - 1].any() and pk[:, :, s].any() and pk[:, s - 1, :].any() and pk[:, s, :].any()
    for cl in range(C):
        assert pk[cl, 0, 0] and pk[cl, 0, W - 1] and pk[cl, H - 1, 0] and pk[cl, H - 1, W - 1]
    assert pk[0, 50, 31] and pk[0, 50, 32] and hm[0, 0, 50, 31] == hm[0, 0, 50, 32]   # the plateau across the seam: both are peaks
    # with a larger K the plateau is part of the result, its left pixel first
    _, det, _ = twin.decode_ct_hm(hm, c["wh"], K=64, clip=False)
    rows = np.flatnonzero(det[0, :, 4] == np.float32(0.55))
    assert len(rows) == 2 and rows[1] == rows[0] + 1


# ------------------------------------------------------------------------------------------------ 2. ties, short counts, limits
def test_a_tie_goes_to_the_lower_flat_index():
    hm, wh, K = twin.tie_case()
    ct, det, count = twin.decode_ct_hm(hm, wh, K=K)
    assert count.tolist() == [K]
    assert det[0, :, 4].tolist() == [np.float32(v) for v in (0.9, 0.9, 0.7, 0.7, 0.5)]
    assert det[0, :, 5].tolist() == [0, 1, 0, 0, 1]
    assert ct[0].tolist() == [[2, 2], [5, 5], [4, 6], [5, 6], [1, 1]]


def test_fewer_candidates_than_K_give_count_and_zero_rows():
    hm, wh, K = twin.short_case()
    ct, det, count = twin.decode_ct_hm(hm, wh, K=K)
    assert count.tolist() == [3, 0, K]
    assert not det[0, 3:].any() and not ct[0, 3:].any() and not det[1].any() and not ct[1].any()
    assert det[0, :3, 4].tolist() == [np.float32(v) for v in (0.3, 0.2, 0.1)] and det[0, :3, 5].tolist() == [0, 1, 1]
    assert (det[2, :, 4] > 0).all()


def test_K_beyond_the_limits_raises():
    hm, wh = twin.heat_maps(1, (1, 1, 3, 3))
    for K in (0, 10, twin.MAX_K + 1):
        with pytest.raises(ValueError):
            twin.decode_ct_hm(hm, wh, K=K)
    twin.decode_ct_hm(hm, wh, K=9)


# ------------------------------------------------------------------------------------------------ 3. the warp
@pytest.mark.parametrize("out_size", [(32, 32), (256, 256)])
def test_fixed_point_warp_against_a_binary64_bilinear_sampler(out_size):
    """|fixed point - exact| <= 0.5 + 2 D (1/64 + 1/1024): 0.5 from the final rounding to 8 bits; per axis, a coordinate that is
    off by at most 1/64 pixel (the 5 fractional bits kept, rounded to nearest) plus 1/1024 (the two roundings to 10 bits, half a
    unit each) moves a bilinear surface whose slope is at most D, the largest neighbour difference, the zero border included."""
    img = twin.image(1)
    D = twin.neighbour_difference(img)
    bound = 0.5 + 2 * D * (1 / 64 + 1 / 1024)
    worst = 0.0
    for box in twin.BOXES:
        _c, _s, trans, valid = twin.box_transform(box, out_size, twin.SCALE_RATIO)
        assert valid
        got = twin.warp_u8(img, trans, out_size).astype(np.float64)
        worst = max(worst, float(np.abs(got - twin.bilinear_f64(img, trans, out_size)).max()))
    print("out %s: worst %.3f grey levels, bound %.3f at D = %d" % (out_size, worst, bound, D))
    assert worst <= bound
    assert worst > 0                                                               # (the comparison is not of a thing with itself)


def test_crop_twin_outputs_and_the_invalid_box():
    img = np.stack([twin.image(1), twin.image(2)])
    boxes = np.concatenate([twin.BOXES[:2], [[3.0, np.nan, 9.0, 12.0]], twin.BOXES[2:], [[10.0, 10.0, 10.0, 10.0]]])
    index = np.arange(len(boxes)) % 2
    out = twin.crop_boxes(img, boxes, index, (32, 32), **KW)
    assert out["valid"].tolist() == [True, True, False, True, True, True, False]
    zero = twin.normalise(np.zeros((32, 32, 3), np.uint8), twin.MEAN, twin.STD)
    for n in (2, 6):                                                               # a NaN entry; scale 0
        assert not out["trans"][n].any() and not out["center"][n].any() and out["scale"][n] == 0
        np.testing.assert_array_equal(out["inp"][n], zero)
    np.testing.assert_array_equal(out["center"][0], np.float32([35, 27]))
    assert out["scale"][0] == np.float32(30 * 1.2) and out["trans"].dtype == np.float64
    a = 32 / np.float64(out["scale"][0])
    np.testing.assert_array_equal(out["trans"][0], [[a, 0, 16 - a * 35], [0, a, 16 - a * 27]])
    # the box over the corner reads the zero border; the whole-image crop holds the image's corners inside
    assert (out["u8"][1][0, 0] == 0).all() and out["u8"][1].any()
    # the same boxes as float32 are the same boxes: these are exact in float32
    out32 = twin.crop_boxes(img, boxes.astype(np.float32), index, (32, 32), **KW)
    np.testing.assert_array_equal(out32["inp"], out["inp"])


def test_blanking_rectangle_rounds_half_to_even():
    """A box whose corners land on (0, 0) and (32, 32) of the crop (scale_ratio 1, a = 1): 25/32 spreads them to 3.5 and 28.5,
    27/32 to 2.5 and 29.5 -- half to even gives 4, 28 and 2, 30 (half up would give 4, 29 and 3, 30)."""
    box, size = [4.0, 4.0, 36.0, 36.0], (32, 32)
    _c, _s, trans, _v = twin.box_transform(box, size, 1.0)
    np.testing.assert_array_equal(trans, [[1, 0, -4], [0, 1, -4]])
    assert twin.blank_rect(box, trans, size, 25 / 32) == (4, 4, 28, 28)
    assert twin.blank_rect(box, trans, size, 27 / 32) == (2, 2, 30, 30)
    assert twin.blank_rect(box, trans, size, 1.2) == (0, 0, 31, 31)                # clipped to the crop
    img = np.full((1, 54, 72, 3), 200, np.uint8)
    out = twin.crop_boxes(img, [box], [0], size, scale_ratio=1.0, box_ratio=25 / 32, mean=twin.MEAN, std=twin.STD)
    kept = out["u8"][0].any(2)
    assert kept[4:29, 4:29].all() and kept.sum() == 25 * 25


# ------------------------------------------------------------------------------------------------ 4. the ways back
def test_uncrop_keypoints_returns_the_points_it_was_projected_from():
    rng = np.random.default_rng(5)
    pts = rng.random((len(twin.BOXES), 9, 2)) * [72, 54]
    trans = np.stack([twin.box_transform(b, (256, 256), twin.SCALE_RATIO)[2] for b in twin.BOXES])
    crop = pts * trans[:, None, [0, 1], [0, 1]] + trans[:, None, :, 2]
    back = twin.uncrop_keypoints(crop, trans)
    assert back.dtype == np.float64
    tol.assert_means_close(back, pts, what="uncropped keypoints")
    tol.assert_means_close(twin.uncrop_keypoints(crop.astype(np.float32), trans), pts, extra=256 * 2.0 ** -24 / trans[:, None, [0, 1], [0, 1]],
                           what="uncropped float32 keypoints")                    # (+ the float32 rounding of a crop coordinate < 256)
    assert not twin.uncrop_keypoints(crop[:1], np.zeros((1, 2, 3))).any()          # an invalid box: zeros, not NaN


def test_uncrop_mask_puts_a_one_to_one_crop_back_where_it_was_cut():
    rng = np.random.default_rng(6)
    canvas = (rng.random((2, 54, 72)) < 0.4).astype(np.uint8) * np.uint8(3)
    bx, by, w, h = 17, 9, 30, 20
    crop = canvas[:, by:by + h, bx:bx + w]
    trans = np.tile(np.array([[1., 0., -bx], [0., 1., -by]]), (2, 1, 1))
    back = twin.uncrop_mask(crop, trans, (72, 54))
    want = np.zeros_like(canvas)
    want[:, by:by + h, bx:bx + w] = crop
    np.testing.assert_array_equal(back, want)
    np.testing.assert_array_equal(twin.uncrop_mask(crop.astype(np.int64), trans, (72, 54)), want)
    # through a real crop transform: the crop-sized all-ones mask comes back as the box's square, clipped to the canvas
    _c, s, t, _v = twin.box_transform(twin.BOXES[0], (32, 32), twin.SCALE_RATIO)
    sq = twin.uncrop_mask(np.ones((1, 32, 32), np.uint8), t[None], (72, 54))[0]
    ys, xs = np.nonzero(sq)
    assert abs((xs.max() - xs.min() + 1) - float(s)) <= 1 and abs((ys.max() - ys.min() + 1) - float(s)) <= 1
    assert sq[27, 35] == 1 and sq.sum() == (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)
