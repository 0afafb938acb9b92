"""The T-LESS PVNet loader's training sample on the MI355X (clean_pvnet_amd.tless_augment) against the numpy twin
(tests/tless_augment_twin.py, itself pinned in tests/test_tless_augment.py): every output of ``rotate_image``, ``tless_compose`` and
``tless_pvnet_augment`` as bytes -- keypoints and ``trans_input`` included: both sides run the same binary64 operations -- an identity
case that does not go through the twin, reruns, strided and bool inputs, the chain under the sync debug mode, and the chain between
``render.render_color`` and ``train.pvnet_loss``.

The shapes are the smallest at which these kernels can go wrong: a 30 x 50 canvas (a width that is a multiple of neither 4 nor 64),
14 x 18 target cut-outs and odd 13 x 17 distractors (planes of 22 x 22 and 21 x 21: more than one 4-row block, rows shorter than
a wave), ``input_size`` (24, 32), non-square so that a swap of width and height shows, K = 3, N = 2, N = 16 once and N = 0 once, B = 1 and 3; the
mixed batch turns a 12 x 16 target, whose 3-4-5 angle fills the plane's width exactly."""
import numpy as np
import pytest

from tests import tless_augment_twin as twin

pytestmark = pytest.mark.gpu


def _t(gpu, a):
    import torch
    return None if a is None else torch.tensor(np.asarray(a), device=gpu)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        diff = np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)
        print("%s: %s: %d of %d bytes differ" % (what, k, diff.sum(), diff.size))
    assert all(got[k].tobytes() == want[k].tobytes() for k in keys), what


def _chain(gpu, batch, ckw, akw):
    """(compose, augment) of the device as numpy."""
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = batch
    ckw = dict(ckw, **{k: _t(gpu, ckw[k]) for k in ("fused_bg", "num") if ckw.get(k) is not None})
    c = ta.tless_compose(_t(gpu, bg), _t(gpu, img), _t(gpu, mask), _t(gpu, kpt), _t(gpu, oi), _t(gpu, om), d, **ckw)
    a = ta.tless_pvnet_augment(c["img"], c["mask"], c["kpt_2d"], c["bbox"], d, **akw)
    return _np(c), _np(a)


def _check_chain(gpu, batch, what, ckw, akw):
    bg, img, mask, kpt, oi, om, d = batch
    want_c = twin.compose(bg, img, mask, kpt, oi, om, d, **ckw)
    want_a = twin.augment(want_c["img"], want_c["mask"], want_c["kpt_2d"], want_c["bbox"], d, **akw)
    got_c, got_a = _chain(gpu, batch, ckw, akw)
    _assert_same(got_c, want_c, twin.COMPOSE_KEYS, what + " compose")
    _assert_same(got_a, want_a, twin.AUGMENT_KEYS, what + " augment")
    return want_c, want_a


AKW = dict(input_size=twin.INPUT_SIZE)


# ------------------------------------------------------------------------------------------------------------ 1. against the twin
@pytest.mark.parametrize("B,N,interp", [(1, 2, "linear"), (3, 2, "nearest"), (3, 2, "linear"), (1, 16, "nearest"), (1, 0, "linear")])
def test_the_chain_equals_the_twin(pkg, gpu, B, N, interp):
    batch = twin.batch(B, 50 + B + N, N=N)
    c, a = _check_chain(gpu, batch, "B=%d N=%d %s" % (B, N, interp), dict(interp=interp, fused_bg=twin.fused_backgrounds(batch[0])), AKW)
    assert c["mask"].any() and a["mask"].any() and (c["place"][:, :, 2] >= 0).all()


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_the_required_cases_as_one_mixed_batch(pkg, gpu, interp):
    """tests/test_tless_augment.py asserts, on the twin, that each sample is the case its name says (with 'linear')."""
    *batch, kw = twin.mixed_batch()
    c, _a = _check_chain(gpu, batch, "mixed " + interp, dict(kw, interp=interp, fused_bg=twin.fused_backgrounds(batch[0])), twin.MIXED_AUGMENT_KW)
    assert set(c["path"].tolist()) == {0, 1, 2, 3}


def test_train_false_leaves_the_colour_steps_out(pkg, gpu):
    _c, a = _check_chain(gpu, twin.batch(3, 77), "train=False", {}, dict(AKW, train=False))
    plain = (a["orig_img"].astype(np.float32) / np.float32(255) - np.asarray(twin.MEAN, np.float32)) / np.asarray(twin.STD, np.float32)
    assert a["inp"].tobytes() == np.ascontiguousarray(plain.transpose(0, 3, 1, 2)).tobytes()


def test_a_rotated_cutout_larger_than_the_canvas(pkg, gpu):
    *batch, kw = twin.oversize_batch()
    c, _a = _check_chain(gpu, batch, "oversize", kw, AKW)
    assert (c["place"][0, :, 2] > 10).all() and not c["place"][0, :, 4:].any()


def test_rotate_image_alone_and_its_bytes_on_the_composers_route(pkg, gpu):
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = twin.batch(3, 71)
    d[0, twin.N_SAMPLE], d[0, twin.N_SAMPLE + twin.PER], d[1, twin.N_SAMPLE], d[1, twin.N_SAMPLE + twin.PER] = 0., 0.25, 0.5, 0.125
    deg = d[:, twin.N_SAMPLE::twin.PER] * 360.                                                    # [B,N]: the composer's angles; 0, 90, 180, 45 first
    for interp in ("linear", "nearest"):
        for src in (oi, om, om != 0):
            got = _np(ta.rotate_image(_t(gpu, src), deg, interp))
            _assert_same(got, twin.rotate_image(src, deg, interp), ("out", "size", "rot"), "rotate_image %s %s %s" % (interp, src.dtype, src.shape))
        assert got["out"].shape == (3, 2, 21, 21) and got["size"][0].tolist() == [[13, 17], [17, 13]] and got["size"][1].tolist() == [[13, 17], [21, 21]]
    one = _np(ta.rotate_image(_t(gpu, img[0]), np.float64(33.)))                                  # no leading dimension
    _assert_same(one, twin.rotate_image(img[0], np.float64(33.)), ("out", "size", "rot"), "rotate_image one")
    # the composer samples the owner's colour through the same rule: a distractor's visible pixels are rotate_image's bytes
    d[:, twin.TOP] = 0.75
    rot_i, rot_m = (_np(ta.rotate_image(_t(gpu, v), deg))["out"] for v in (oi, om))
    c = _np(ta.tless_compose(_t(gpu, bg), _t(gpu, img), _t(gpu, mask), _t(gpu, kpt), _t(gpu, oi), _t(gpu, om), d, ratio=1e-9))
    assert (c["path"] == 1).all()
    seen = 0
    for b in range(3):
        y_min, x_min, h, w, dy, dx = c["place"][b, 2]                                             # the last distractor: nothing covers it
        ys, xs = np.nonzero(rot_m[b, 1])
        assert (ys.min(), xs.min(), np.ptp(ys), np.ptp(xs)) == (y_min, x_min, h, w)
        assert np.array_equal(c["img"][b, ys - y_min + dy, xs - x_min + dx], rot_i[b, 1, ys, xs])
        seen += len(ys)
    assert seen > 100


def test_identity_without_the_twin(pkg, gpu):
    """Angle 0, no distractors, on top: the canvas is ``bg`` with the cut-out's masked pixels at ``place``, in torch ops; the mask is
    the cut-out's, the keypoints are shifted by dst - min, the box is the mask's."""
    import torch
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = twin.batch(3, 72)
    d[:, twin.TOP], d[:, twin.BLACK] = 0.25, 0.5
    g = [_t(gpu, v) for v in (bg, img, mask, kpt, oi, om)]
    c = ta.tless_compose(*g, d, num=torch.zeros(3, dtype=torch.int64, device=gpu), rot_max=0.)
    want_img, want_mask = g[0].clone(), torch.zeros(3, twin.H0, twin.W0, dtype=torch.uint8, device=gpu)
    place = c["place"].cpu()
    for b in range(3):
        y_min, x_min, h, w, dy, dx = (int(v) for v in place[b, 0])
        m = g[2][b, y_min:y_min + h + 1, x_min:x_min + w + 1] != 0
        want_img[b, dy:dy + h + 1, dx:dx + w + 1][m] = g[1][b, y_min:y_min + h + 1, x_min:x_min + w + 1][m]
        want_mask[b, dy:dy + h + 1, dx:dx + w + 1][m] = 1
        ys, xs = torch.nonzero(g[2][b], as_tuple=True)
        assert (y_min, x_min, h, w) == (int(ys.min()), int(xs.min()), int(ys.max() - ys.min()), int(xs.max() - xs.min()))
        assert 0 <= dy <= twin.H0 - h - 1 and 0 <= dx <= twin.W0 - w - 1
        assert c["bbox"][b].tolist() == [dx, dy, dx + w, dy + h]
        assert torch.equal(c["kpt_2d"][b], g[3][b] - torch.tensor([x_min, y_min], device=gpu) + torch.tensor([dx, dy], device=gpu))
        assert c["visible"][b].tolist() == [int(m.sum()), int(g[2][b].to(torch.int64).sum())]
    assert torch.equal(c["img"], want_img) and torch.equal(c["mask"], want_mask) and c["path"].tolist() == [0, 0, 0]
    assert (place[:, 1:, 2] == -1).all()


# ------------------------------------------------------------------------------------------------------------ 2. how it runs
def test_reruns_give_the_same_bytes(pkg, gpu):
    batch = twin.batch(3, 73)
    first = _chain(gpu, batch, {}, AKW)
    for _ in range(3):
        again = _chain(gpu, batch, {}, AKW)
        assert all(again[0][k].tobytes() == first[0][k].tobytes() for k in twin.COMPOSE_KEYS)
        assert all(again[1][k].tobytes() == first[1][k].tobytes() for k in twin.AUGMENT_KEYS)


def test_strided_and_bool_inputs(pkg, gpu):
    import torch
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = twin.batch(3, 74)
    mask, om = mask != 0, om != 0
    want_c = twin.compose(bg, img, mask, kpt, oi, om, d)
    want_a = twin.augment(want_c["img"], want_c["mask"], want_c["kpt_2d"], want_c["bbox"], d, **AKW)
    wide_bg = torch.zeros(3, 30, 100, 3, dtype=torch.uint8, device=gpu)
    wide_bg[:, :, ::2] = _t(gpu, bg)
    wide_img = torch.zeros(3, 28, 18, 3, dtype=torch.uint8, device=gpu)
    wide_img[:, ::2] = _t(gpu, img)
    wide_oi = torch.zeros(3, 4, 13, 17, 3, dtype=torch.uint8, device=gpu)
    wide_oi[:, ::2] = _t(gpu, oi)
    wide_kpt = torch.zeros(3, 3, 4, dtype=torch.float32, device=gpu)
    wide_kpt[..., ::2] = _t(gpu, kpt.astype(np.float32))                                          # float32 keypoints, every other column
    want32 = twin.compose(bg, img, mask, kpt.astype(np.float32), oi, om, d)
    c = ta.tless_compose(wide_bg[:, :, ::2], wide_img[:, ::2], _t(gpu, mask), wide_kpt[..., ::2], wide_oi[:, ::2], _t(gpu, om), d)
    _assert_same(_np(c), want32, twin.COMPOSE_KEYS, "strided compose")
    c = ta.tless_compose(_t(gpu, bg), _t(gpu, img), _t(gpu, mask), _t(gpu, kpt), _t(gpu, oi), _t(gpu, om), d)
    wide_c = torch.zeros(3, 60, 50, 3, dtype=torch.uint8, device=gpu)
    wide_c[:, ::2] = c["img"]
    wide_m = torch.zeros(3, 30, 50, 2, dtype=torch.uint8, device=gpu)
    wide_m[..., 0] = c["mask"]
    wide_b = torch.zeros(3, 8, dtype=torch.int32, device=gpu)
    wide_b[:, ::2] = c["bbox"]
    a = ta.tless_pvnet_augment(wide_c[:, ::2], wide_m[..., 0], c["kpt_2d"], wide_b[:, ::2], d, **AKW)
    _assert_same(_np(a), want_a, twin.AUGMENT_KEYS, "strided augment")


def test_the_chain_reads_nothing_back(pkg, gpu):
    import torch
    from clean_pvnet_amd import tless_augment as ta
    bg, img, mask, kpt, oi, om, d = twin.batch(3, 75)
    args = [_t(gpu, v) for v in (bg, img, mask, kpt, oi, om)]
    aug = ta.TlessPVNetAugment(input_size=twin.INPUT_SIZE)
    deg = np.full((3, 2), 30.)
    aug(*args, draws=d)                                                   # (the first call may allocate)
    ta.rotate_image(args[4], deg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = aug(*args, draws=d)
        rot = ta.rotate_image(args[4], deg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert batch["inp"].shape == (3, 3, 24, 32) and rot["out"].shape == (3, 2, 21, 21, 3)


def test_render_color_feeds_the_composer_and_the_batch_feeds_pvnet_loss(pkg, gpu):
    """mesh + poses -> ``render_color`` -> ``TlessPVNetAugment`` -> ``train.pvnet_loss(kpt_2d=...)`` on one stream: the rendered image and
    its label are the target's cut-out; the batch equals the twin's on the rendered bytes and a step of the wrapper runs."""
    import torch
    from clean_pvnet_amd import render, tless_augment as ta, train
    from tests.test_gpu_render import _scene
    s = _scene()
    r = render.render_color(_t(gpu, s["pts"]), _t(gpu, s["colors"]), _t(gpu, s["faces"]), _t(gpu, s["pose"]), _t(gpu, s["K"]), s["size"],
                            ranges=s["ranges"], obj=_t(gpu, s["obj"]), near=s["near"], far=s["far"], ambient=s["ambient"])
    B = 2
    bg, _i, _m, _k, oi, om, d = twin.batch(B, 76)
    kpt = np.random.default_rng(4).random((B, twin.K0, 2)) * [s["size"][0], s["size"][1]]
    g = [_t(gpu, bg), r["img"], r["label"], _t(gpu, kpt), _t(gpu, oi), _t(gpu, om)]
    assert r["label"].any()
    batch = ta.TlessPVNetAugment(input_size=twin.INPUT_SIZE)(*g, draws=d)
    img, label = r["img"].cpu().numpy(), r["label"].cpu().numpy()
    want_c = twin.compose(bg, img, label, kpt, oi, om, d)
    want_a = twin.augment(want_c["img"], want_c["mask"], want_c["kpt_2d"], want_c["bbox"], d, **AKW)
    assert set(batch) == {"inp", "mask", "kpt_2d", "meta"} and batch["meta"] == {}
    _assert_same(_np({k: batch[k] for k in ("inp", "mask", "kpt_2d")}), want_a, ("inp", "mask", "kpt_2d"), "render -> batch")
    assert want_a["mask"].any()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 2 * twin.K0 + 2, 3, padding=1)

        def forward(self, x):
            y = self.conv(x)
            return {"vertex": y[:, :2 * twin.K0], "seg": y[:, 2 * twin.K0:]}
    torch.manual_seed(0)
    wrapper = train.NetworkWrapper(Net().to(gpu))
    _out, loss, stats, _ = wrapper(batch)
    loss.backward()
    assert torch.isfinite(loss).item() and set(stats) == {"vote_loss", "seg_loss", "loss"} and wrapper.net.conv.weight.grad is not None
    vote, seg = train.pvnet_loss(_out["vertex"], _out["seg"], batch["mask"], kpt_2d=batch["kpt_2d"])
    assert torch.isfinite(vote).item() and torch.isfinite(seg).item()
