"""The detector's training batch and input preparation (clean_pvnet_amd.ct_augment, include/pvnet_vote.h, "Detector augmentation")
without a GPU: the module and its entry points exist and refuse bad arguments before any launch; the host's block equals the
twin's values; the numpy twin of the contract (tests/ct_augment_twin.py) reproduces the reference's own code on the fixtures of
tests/golden/make_ct_augment_golden.py -- as bytes in the canvas, the label map, centre, scale, both sets of boxes and the warped
image, within derived bounds in the two transforms and the float image -- its warp stays within section 12's bound of a binary64
sampler and its ownership rule is the binary64 bilinear sample of the mask.  The GPU tests (tests/test_gpu_ct_augment.py) then
hold the device to the twin byte for byte."""
import math
import os

import numpy as np
import pytest

from tests import capi, crop_twin
from tests import ct_augment_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("ct_augment_mixed_30x50", "ct_augment_wide_30x50", "ct_augment_test_30x50")
SYMBOLS = {"pvv_ct_compose", "pvv_ct_augment_workspace_bytes", "pvv_ct_augment"}
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def cases():
    """Each fixture with the twin's results on it, computed once."""
    out = {}
    for name in FIXTURES:
        c = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        c["N"], c["is_train"] = c["cls"].shape[1], bool(c["train"])
        c["compose"] = twin.compose(c["bg"], c["inst_img"], c["inst_mask"], c["num"], c["draws"])
        kw = dict(train=c["is_train"], input_size=tuple(int(v) for v in c["input_size"]), n_instances=c["N"])
        c["linear"] = twin.augment(c["compose"]["img"], c["compose"]["label"], c["draws"], boxes="linear", **kw)
        c["nearest"] = twin.augment(c["compose"]["img"], c["compose"]["label"], c["draws"], boxes="nearest", **kw)
        out[name] = c
    return out


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import ct_augment
    assert all(callable(getattr(ct_augment, f)) for f in ("draws", "ct_compose", "ct_augment", "CtAugment"))
    assert ct_augment.ORDERS == twin.ORDERS and ct_augment.N_SAMPLE == twin.N_SAMPLE and ct_augment.NORMAL_COLUMNS == twin.NORMAL_COLUMNS
    assert (ct_augment.MEAN, ct_augment.STD, ct_augment.EIG_VAL, ct_augment.EIG_VEC) == (twin.MEAN, twin.STD, twin.EIG_VAL, twin.EIG_VEC)
    assert ct_augment.MAX_N == 16 and ct_augment.PARAM.itemsize == 160


def test_header_declares_and_library_exports_the_entry_points():
    raw = open(HEADER).read()
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in raw                                      # additive: the version did not move
    assert "Detector augmentation" in raw and "#define PVV_CT_AUGMENT_PARAM_BYTES 160" in raw and "#define PVV_CT_AUGMENT_MAX_N 16" in raw
    section = raw[raw.index("Detector augmentation"):raw.index("Detector training")]
    for cited in ("tless_utils.py", "tless/ct.py:58-70", "tless_train/ct.py:75-76", "data_utils.py"):
        assert cited in section


def test_draws_follow_torchs_generator(pkg):
    import torch
    from clean_pvnet_amd import ct_augment
    torch.manual_seed(5)
    a = ct_augment.draws(4, 6)
    torch.manual_seed(5)
    b = ct_augment.draws(4, 6)
    c = ct_augment.draws(4, 6, generator=torch.Generator().manual_seed(6))
    assert a.shape == (4, 11 + 12) and a.dtype == np.float64 and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    uni = np.delete(a, twin.NORMAL_COLUMNS, axis=1)
    assert ((uni >= 0) & (uni < 1)).all()
    normals = ct_augment.draws(4000, 0, generator=torch.Generator().manual_seed(1))[:, list(twin.NORMAL_COLUMNS)]
    assert (normals < 0).any() and abs(normals.mean()) < 0.05 and abs(normals.std() - 1) < 0.05     # standard normals, not uniforms
    assert len(ct_augment.COLUMNS) == 11 and ct_augment.COLUMNS[0] == "scale" and ct_augment.COLUMNS[3] == "order" and ct_augment.COLUMNS[10] == "rot"


@pytest.mark.parametrize("train,rot", [(True, 0.0), (True, 30.0), (False, 0.0)])
def test_host_block_equals_the_twins_values(pkg, train, rot):
    from clean_pvnet_amd import ct_augment
    d = twin.draws_for(40, 0, 3)
    H, W, size = 30, 50, (44, 72)
    block, meta = ct_augment.host_block(d, H, W, train=train, input_size=size, rot=rot)
    ih, iw = size if train else (32, 64)
    assert meta["sizes"] == (ih, iw, ih // 4, iw // 4)
    seen = set()
    for b, u in enumerate(d):
        c, s = twin.center_scale(H, W, u, train=train)
        t_in, t_out = twin.affine(c, s, rot, (iw, ih)), twin.affine(c, s, rot, (iw // 4, ih // 4))
        assert meta["center"][b].tobytes() == c.tobytes() and meta["scale"][b].tobytes() == s.tobytes()
        assert meta["trans_input"][b].tobytes() == t_in.tobytes() and meta["trans_output"][b].tobytes() == t_out.tobytes()
        assert block["inv_in"][b].tobytes() == crop_twin.invert_affine(t_in).tobytes()
        assert block["inv_out"][b].tobytes() == crop_twin.invert_affine(t_out).tobytes()
        if train:
            order, alpha, light = twin.colour_params(u)
            assert tuple(block["order"][b]) == order and block["light"][b].tobytes() == np.asarray(light, F64).tobytes()
            assert block["a"][b].tobytes() == np.array(alpha, F32).tobytes()
            assert block["oma"][b].tobytes() == np.array([1 - v for v in alpha], F32).tobytes()
            seen.add(order)
    assert not train or len(seen) == 6


def test_the_closed_form_is_the_similarity_the_three_points_define():
    """A property of the map, for a rotation too: the centre goes to the middle of the destination, the point half a scale above
    the centre, turned by rot, to the middle of the top edge, and the map is a similarity of factor dw / scale."""
    c, s, size = np.array([21., 13.], F32), np.array([37.5, 37.5], F32), (72, 44)
    for rot in (0.0, 30.0, -60.0):
        T = twin.affine(c, s, rot, size)
        rad = math.pi * rot / 180
        up = np.array([c[0] + 18.75 * math.sin(rad), c[1] - 18.75 * math.cos(rad)])
        assert np.allclose(T[:, :2] @ c + T[:, 2], [36, 22], atol=1e-12) and np.allclose(T[:, :2] @ up + T[:, 2], [36, 22 - 36], atol=1e-12)
        assert np.allclose(T[:, :2] @ T[:, :2].T, np.eye(2) * (72 / 37.5) ** 2, atol=1e-12) and np.linalg.det(T[:, :2]) > 0


def _meta(*shape, dtype=None):
    import torch
    return torch.empty(*shape, dtype=dtype or torch.uint8, device="meta")


def test_arguments_are_refused_before_any_launch(pkg):
    import torch
    from clean_pvnet_amd import ct_augment
    u8 = torch.uint8
    d = twin.draws_for(2, 3, 1)
    z = lambda *s, dtype=u8: torch.zeros(*s, dtype=dtype)                         # noqa: E731
    with pytest.raises(RuntimeError, match="bg must be a CUDA tensor; there is no CPU fallback"):
        ct_augment.ct_compose(z(2, 16, 16, 3), z(2, 3, 8, 8, 3), z(2, 3, 8, 8), z(2, dtype=torch.int64), d)
    with pytest.raises(RuntimeError, match="img must be a CUDA tensor"):
        ct_augment.ct_augment(z(2, 16, 16, 3), z(2, 16, 16), d)
    with pytest.raises(RuntimeError, match="bg must be a CUDA tensor"):
        ct_augment.CtAugment()(z(2, 16, 16, 3), z(2, 3, 8, 8, 3), z(2, 3, 8, 8), z(2, 3, dtype=torch.int64), z(2, dtype=torch.int64), d)
    real_need, real_call = ct_augment._native.need_cuda, ct_augment._call

    def no_launch(*a):
        raise AssertionError("a launch was reached")
    ct_augment._native.need_cuda, ct_augment._call = (lambda *a: None), no_launch             # past the device check
    try:
        bg, ii, im, num = _meta(2, 16, 16, 3), _meta(2, 3, 8, 8, 3), _meta(2, 3, 8, 8), _meta(2, dtype=torch.int64)
        with pytest.raises(TypeError, match="bg must be \\[B,H,W,3\\] uint8"):
            ct_augment.ct_compose(_meta(2, 16, 16, 3, dtype=torch.float32), ii, im, num, d)
        with pytest.raises(TypeError, match="inst_mask uint8 or bool"):
            ct_augment.ct_compose(bg, ii, _meta(2, 3, 8, 8, dtype=torch.int64), num, d)
        with pytest.raises(TypeError, match="num int32 or int64"):
            ct_augment.ct_compose(bg, ii, im, _meta(2, dtype=torch.float32), d)
        with pytest.raises(ValueError, match="inst_img must be"):
            ct_augment.ct_compose(bg, _meta(3, 3, 8, 8, 3), im, num, d)
        with pytest.raises(ValueError, match="inst_mask must be \\[2, 3, 8, 8\\]"):
            ct_augment.ct_compose(bg, ii, _meta(2, 3, 8, 7), num, d)
        with pytest.raises(ValueError, match="num must be \\[B = 2\\]"):
            ct_augment.ct_compose(bg, ii, im, _meta(3, dtype=torch.int64), d)
        with pytest.raises(ValueError, match="N must lie in \\[1, 16\\]"):
            ct_augment.ct_compose(bg, _meta(2, 17, 8, 8, 3), _meta(2, 17, 8, 8), num, twin.draws_for(2, 17, 1))
        bad = [d[:1], d[:, :16], d.astype(np.float32), np.where(np.arange(17) == 12, 1.0, d), np.where(np.arange(17) == 0, -0.1, d),
               np.where(np.arange(17) == 8, np.nan, d)]
        for draws in bad:
            with pytest.raises(ValueError, match="draws must|must lie in \\[0, 1\\)"):
                ct_augment.ct_compose(bg, ii, im, num, draws)
        img, label = _meta(2, 16, 16, 3), _meta(2, 16, 16)
        with pytest.raises(TypeError, match="label must be \\[2, 16, 16\\] uint8"):
            ct_augment.ct_augment(img, _meta(2, 16, 16, dtype=torch.int64), d)
        with pytest.raises(TypeError, match="label must be"):
            ct_augment.ct_augment(img, _meta(2, 16, 15), d)
        with pytest.raises(ValueError, match="n_instances must lie in \\[1, 16\\]"):
            ct_augment.ct_augment(img, label, d, n_instances=17)
        with pytest.raises(ValueError, match="boxes must be 'linear' or 'nearest'"):
            ct_augment.ct_augment(img, label, d, boxes="cubic")
        with pytest.raises(ValueError, match="train=True needs draws"):
            ct_augment.ct_augment(img, None, None)
        with pytest.raises(ValueError, match="input_size sides"):
            ct_augment.ct_augment(img, label, d, input_size=(3, 72))
        with pytest.raises(ValueError, match="draws must"):
            ct_augment.ct_augment(img, label, d[:, :10], n_instances=3)
    finally:
        ct_augment._native.need_cuda, ct_augment._call = real_need, real_call


# ------------------------------------------------------------------------------------------------ 1. the twin against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_equals_the_reference_as_bytes(cases, name):
    c = cases[name]
    comp, lin, near = c["compose"], c["linear"], c["nearest"]
    assert comp["img"].tobytes() == c["ref_img"].tobytes()                                              # the canvas
    ids = np.concatenate([np.zeros((len(c["ref_ids"]), 1), np.int64), c["ref_ids"]], axis=1)            # label -> the reference's id
    mapped = np.stack([ids[b][comp["label"][b]] for b in range(len(ids))])
    assert mapped.astype(np.int16).tobytes() == c["ref_label"].tobytes()
    assert (c["ref_center"] == np.rint(c["ref_center"])).all() or not c["is_train"]
    assert lin["center"].tobytes() == c["ref_center"].astype(F32).tobytes() and (lin["center"].astype(F64) == c["ref_center"]).all()
    assert lin["scale"].tobytes() == c["ref_scale"].astype(F32).tobytes() and (lin["scale"].astype(F64) == c["ref_scale"]).all()
    assert lin["boxes"].tobytes() == c["ref_boxes_linear"].tobytes() and near["boxes"].tobytes() == c["ref_boxes_nearest"].tobytes()
    assert lin["orig_img"].tobytes() == c["ref_orig"].tobytes() and near["orig_img"].tobytes() == c["ref_orig"].tobytes()
    assert lin["boxes"].any() and (lin["orig_img"] != 0).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_transforms_agree_with_the_three_point_solve_within_the_derived_bound(cases, name):
    """twin.trans_bound states the derivation: the solve's float32 source points against the closed form's exact ones."""
    c = cases[name]
    ih, iw, oh, ow = (int(v) for v in c["ref_sizes"][0])
    worst = 0.0
    for b in range(len(c["bg"])):
        ctr, s = c["linear"]["center"][b], c["linear"]["scale"][b]
        for key, ref, size, rot in (("trans_input", c["ref_trans_input"][b], (iw, ih), 0.0), ("trans_output", c["ref_trans_output"][b], (ow, oh), 0.0),
                                    ("rot", c["ref_trans_rot"][b], (iw, ih), float(c["rot_probe"]))):
            got = c["linear"][key][b] if rot == 0 else twin.affine(ctr, s, rot, size)
            lin, tr = twin.trans_bound(ctr, s, size)
            diff = np.abs(got - ref)
            worst = max(worst, diff[:, :2].max() / lin, diff[:, 2].max() / tr)
            assert diff[:, :2].max() <= lin and diff[:, 2].max() <= tr, (name, b, key, diff, lin, tr)
    print("%s: trans observed / bound = %.3g" % (name, worst))


def grey_mean_bound(n, mean):
    """|float32 pairwise mean - the fixed-tree binary64 mean rounded once| for n grey levels in [0, 1].  numpy's pairwise sum adds
    blocks of at most 128 in 8 accumulators (15 additions each, 3 levels to combine them) and halves above that: an element passes
    through d = 18 + ceil(log2(n / 128)) additions at the most, each of relative error 2^-24, so the float32 sum is within
    d 2^-24 (1 + d 2^-24) of the exact one, relative (all terms are non-negative); the division by n rounds once more (2^-24).  The
    binary64 tree is exact to n 2^-53 and its one rounding to float32 adds half an ulp, 2^-24 relative."""
    d = 18 + max(0, math.ceil(math.log2(n / 128)))
    return mean * ((d * 2.0 ** -24) * (1 + d * 2.0 ** -24) + 2.0 ** -24 + 2.0 ** -24 + n * 2.0 ** -53)


def inp_bound(u, n, gm, ref_inp, std=twin.STD, mean=twin.MEAN):
    """How far two runs of the same float32 program may end apart when gs_mean differs by delta = grey_mean_bound.  The contrast
    step adds t = float32(gs_mean * (1 - alpha)): the two t differ by |1 - alpha| delta plus one spacing of t (two roundings, half
    each).  Every later float32 operation maps a difference E to |gain| E plus one spacing of its result: the contrast's own sum,
    the product with alpha of each later step (gain alpha) and that step's sum, the lighting sum, the subtraction of the mean and
    the division by std (gain 1 / std).  Spacings are taken at twice the largest magnitude before the normalisation (a later
    product with alpha >= 0.6 may have shrunk a value) and at the largest magnitude after it."""
    order, alpha, _light = twin.colour_params(u)
    at = order.index(twin.CONTRAST)
    delta = grey_mean_bound(n, float(gm))
    pre = np.abs(ref_inp * np.asarray(std, F32)[:, None, None] + np.asarray(mean, F32)[:, None, None]).max()
    u_pre, u_post = float(np.spacing(F32(2 * max(1.0, pre)))), float(np.spacing(F32(np.abs(ref_inp).max())))
    E = abs(1 - alpha[at]) * delta + float(np.spacing(F32(abs(float(gm) * (1 - alpha[at])))))
    E += u_pre                                                    # x * a + t
    for s in range(at + 1, 3):
        E = abs(alpha[s]) * E + u_pre
        if order[s] != twin.BRIGHTNESS:
            E += u_pre
    E += u_pre                                                    # the lighting vector
    E += u_pre                                                    # - mean
    return E / min(std) + u_post


@pytest.mark.parametrize("name", FIXTURES)
def test_inp_agrees_with_the_reference_within_the_derived_bound(cases, name):
    c = cases[name]
    got, ref = c["linear"]["inp"], c["ref_inp"]
    assert ref.dtype == F32 and got.shape == ref.shape
    if not c["is_train"]:
        assert got.tobytes() == ref.tobytes()                     # no mean enters: bit for bit
        return
    n = got.shape[2] * got.shape[3]
    worst = 0.0
    for b in range(len(got)):
        bound = inp_bound(c["draws"][b], n, twin.grey_mean(c["linear"]["orig_img"][b]), ref[b])
        diff = float(np.abs(got[b] - ref[b]).max())
        worst = max(worst, diff / bound)
        assert diff <= bound, (name, b, diff, bound)
    print("%s: inp observed / bound = %.3g" % (name, worst))


# ------------------------------------------------------------------------------------------------ 2. the required cases
def test_the_mixed_fixture_holds_the_required_cases(cases):
    c = cases["ct_augment_mixed_30x50"]
    d, comp, lin, near = c["draws"], c["compose"], c["linear"], c["nearest"]
    oh, ow = 11, 18
    assert [twin.colour_params(u)[0] for u in d[:6]] == list(twin.ORDERS)                          # all six colour orders
    assert lin["scale"][0, 0] < 50 <= lin["scale"][1, 0]                                            # both sides of scale < width
    assert lin["scale"][6, 0] >= 30 and lin["center"][6, 1] == 15                                   # border_r = border + 1 fixes the centre
    assert (comp["place"][2, :, 4:] == comp["place"][2, 0, 4:]).all() and comp["label"][2, 12, 23] == 3      # three overlap: the last wins
    assert not lin["boxes"][2, :2].any() and lin["boxes"][2, 2].any()
    assert tuple(comp["place"][3, 0, :4]) == (5, 6, 0, 0) and (comp["label"][3] == 1).sum() == 1   # a single pixel: h = w = 0
    assert tuple(comp["place"][3, 1]) == (0, 0, -1, -1, 0, 0) and not (comp["label"][3] == 2).any() and not lin["boxes"][3, 1].any()    # empty
    assert c["num"][4] == 1 and set(np.unique(comp["label"][4])) == {0, 1} and not lin["boxes"][4, 1:].any()        # num[b] < N
    assert (comp["label"][6] > 0).any() and not lin["boxes"][6].any() and not near["boxes"][6].any()               # warped wholly outside
    own = twin.owners(comp["label"][7], lin["trans_output"][7], oh, ow, 3, "linear")
    assert own[0][:, ow - 1].any() and lin["boxes"][7, 0, 2] == ow - 1                              # x_max + 1 = ow, clamped by ow - 1
    assert own[1].any() and lin["boxes"][7, 1, 2] == lin["boxes"][7, 1, 0] == ow - 1                # a box collapsing to x2 == x0
    assert (lin["boxes"] != near["boxes"]).any()                                                    # the two rules differ here


def test_unit_alphas_and_a_zero_lighting_vector_leave_x_unchanged(cases):
    c = cases["ct_augment_mixed_30x50"]
    order, alpha, light = twin.colour_params(c["draws"][5])
    assert alpha == [1.0, 1.0, 1.0] and not np.asarray(light).any()
    orig = c["linear"]["orig_img"][5]
    plain = twin.colour(orig, None, train=False)
    assert c["linear"]["inp"][5].tobytes() == plain.tobytes()
    assert c["ref_inp"][5].tobytes() == plain.tobytes()                                             # the reference's too: no mean enters


def test_compose_drops_what_leaves_the_canvas():
    """An instance larger than the canvas takes lo = 0; its pixels outside are dropped (the reference raises)."""
    bg = np.zeros((1, 6, 8, 3), np.uint8)
    img, mask = np.full((1, 1, 12, 14, 3), 9, np.uint8), np.ones((1, 1, 12, 14), np.uint8)
    out = twin.compose(bg, img, mask, np.array([1]), twin.draws_for(1, 1, 2))
    assert tuple(out["place"][0, 0]) == (0, 0, 11, 13, 0, 0) and (out["label"] == 1).all() and (out["img"] == 9).all()


# ------------------------------------------------------------------------------------------------ 3. the samplers
def test_warp_against_a_binary64_bilinear_sampler(cases):
    """Section 12's bound: |fixed point - exact| <= 0.5 + 2 D (1/64 + 1/1024), D the largest neighbour difference."""
    c = cases["ct_augment_mixed_30x50"]
    worst = 0.0
    for b in range(len(c["bg"])):
        img, trans = c["compose"]["img"][b], c["linear"]["trans_input"][b]
        D = crop_twin.neighbour_difference(img)
        bound = 0.5 + 2 * D * (1 / 64 + 1 / 1024)
        diff = float(np.abs(c["linear"]["orig_img"][b].astype(F64) - crop_twin.bilinear_f64(img, trans, (72, 44))).max())
        worst = max(worst, diff / bound)
        assert diff <= bound
    print("warp: worst / bound = %.3f" % worst)
    assert worst > 0


def test_linear_ownership_is_a_nonzero_bilinear_sample_of_the_mask():
    """On a constructed label map: a pixel belongs to instance i iff a binary64 bilinear sample of the 0 / 1 mask of i at the
    quantised coordinate (the 5 fractional bits the rule keeps) is non-zero."""
    rng = np.random.default_rng(5)
    label = np.zeros((30, 50), np.uint8)
    label[4:9, 6:20], label[8:20, 15:18], label[25, 40], label[0:2, 47:50] = 1, 2, 3, 4
    label[rng.integers(0, 30, 40), rng.integers(0, 50, 40)] = 0
    for scale, ctr, size in ((41.3, (22., 13.), (18, 11)), (50., (25., 15.), (50, 30)), (68., (30., 2.), (66, 12))):
        T = twin.affine(np.array(ctr, F32), np.array([scale, scale], F32), 0.0, size)
        ow, oh = size
        sx, sy, a, b = twin.linear_coords(crop_twin.invert_affine(T), oh, ow)
        fx, fy = a / 32., b / 32.
        own = twin.owners(label, T, oh, ow, 4, "linear")
        for i in range(4):
            m = (label == i + 1).astype(F64)
            t = lambda yy, xx: twin._tap2(m, yy, xx)                              # noqa: E731
            v = t(sy, sx) * (1 - fx) * (1 - fy) + t(sy, sx + 1) * fx * (1 - fy) + t(sy + 1, sx) * (1 - fx) * fy + t(sy + 1, sx + 1) * fx * fy
            assert np.array_equal(own[i], v != 0)
            assert np.array_equal(own[i], twin.warp_f32(m.astype(F32), T, size) != 0)
        assert own.any()
