"""The detector's training batch and input preparation on the MI355X (clean_pvnet_amd.ct_augment) against the numpy twin
(tests/ct_augment_twin.py, itself pinned in tests/test_ct_augment.py): every output of ``ct_compose`` and ``ct_augment`` as bytes, an
identity case that does not go through the twin, reruns, strided and bool inputs, the chain under the sync debug mode and
``CtAugment`` -> ``ct_train.ct_targets`` against tests/ct_train_twin.py.

The base shapes are the smallest at which these kernels can go wrong: a 30 x 50 canvas (a width that is a multiple of neither 4
nor 64), 12 x 14 cut-outs (168 bytes: the 4-byte mask loads) and 11 x 13 ones (the byte loads), N = 3, ``input_size`` (44, 72) with
an 11 x 18 output map, (48, 264) with a 12 x 66 map whose rows cross a 64-lane block and whose boxes span two blocks, and
(44, 70), whose width takes the one-pixel-per-lane colour kernel."""
import numpy as np
import pytest

from tests import ct_augment_twin as twin
from tests import ct_train_twin

pytestmark = pytest.mark.gpu
COMPOSE_KEYS = ("img", "label", "place")
AUGMENT_KEYS = ("inp", "orig_img", "boxes", "center", "scale", "trans_input", "trans_output")


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, keys, what):
    for k in keys:
        if k not in want:
            assert k not in got, (what, k)
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        diff = np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)
        print("%s: %s: %d of %d bytes differ" % (what, k, diff.sum(), diff.size))
    assert all(got[k].tobytes() == want[k].tobytes() for k in keys if k in want), what


def _chain(gpu, bg, inst_img, inst_mask, num, d, **kw):
    """(compose, augment) of the device as numpy."""
    from clean_pvnet_amd import ct_augment
    c = ct_augment.ct_compose(_t(gpu, bg), _t(gpu, inst_img), _t(gpu, inst_mask), _t(gpu, num), d)
    a = ct_augment.ct_augment(c["img"], c["label"], d, n_instances=inst_img.shape[1], **kw)
    return _np(c), _np(a)


def _check_chain(gpu, batch, what, **kw):
    bg, inst_img, inst_mask, _cls, num, d = batch
    want_c = twin.compose(bg, inst_img, inst_mask, num, d)
    want_a = twin.augment(want_c["img"], want_c["label"], d, n_instances=inst_img.shape[1], **kw)
    got_c, got_a = _chain(gpu, bg, inst_img, inst_mask, num, d, **kw)
    _assert_same(got_c, want_c, COMPOSE_KEYS, what + " compose")
    _assert_same(got_a, want_a, AUGMENT_KEYS, what + " augment")
    return want_c, want_a


# ------------------------------------------------------------------------------------------------------------ 1. against the twin
@pytest.mark.parametrize("B,input_size,boxes", [(1, (44, 72), "linear"), (5, (44, 72), "nearest"), (33, (44, 72), "linear"),
                                                (1, (48, 264), "nearest"), (5, (48, 264), "linear"), (33, (48, 264), "nearest"),
                                                (5, (44, 70), "linear")])
def test_the_chain_equals_the_twin(pkg, gpu, B, input_size, boxes):
    _c, a = _check_chain(gpu, twin.batch(B, 50 + B), "B=%d %s %s" % (B, input_size, boxes), input_size=input_size, boxes=boxes)
    assert a["boxes"].any()
    if input_size == (48, 264) and B > 1:
        assert (a["boxes"][..., 2] > 64).any() and ((a["boxes"][..., 0] < 64) & (a["boxes"][..., 2] > 64)).any()   # a box over two blocks


@pytest.mark.parametrize("boxes", ["linear", "nearest"])
def test_the_required_cases_as_one_mixed_batch(pkg, gpu, boxes):
    _check_chain(gpu, twin.mixed_batch(), "mixed " + boxes, input_size=(44, 72), boxes=boxes)


def test_byte_loads_of_odd_cutouts_and_sixteen_instances(pkg, gpu):
    bg = np.stack([twin.image(70 + b) for b in range(2)])
    inst_img, inst_mask = twin.cutouts(2, 16, 11, 13, seed=9)
    num, d = np.array([16, 9], np.int32), twin.draws_for(2, 16, 77)
    want_c, _a = _check_chain(gpu, (bg, inst_img, inst_mask, None, num, d), "11x13 N=16", input_size=(44, 72))
    assert want_c["label"].max() == 16 and want_c["label"][1].max() == 9


def test_the_test_split_and_the_inference_path(pkg, gpu):
    from clean_pvnet_amd import ct_augment
    batch = twin.batch(3, 61)
    _c, want = _check_chain(gpu, batch, "train=False", train=False)
    assert want["inp"].shape == (3, 3, 32, 64) and want["boxes"].any()
    got = _np(ct_augment.ct_augment(_t(gpu, batch[0]), None, None, train=False))                  # augment(img, 'test'): no label, no draws
    plain = twin.augment(batch[0], None, None, train=False)
    assert "boxes" not in got
    _assert_same(got, plain, AUGMENT_KEYS, "inference")


def test_a_rotation_equals_the_twin(pkg, gpu):
    _c, a = _check_chain(gpu, twin.batch(5, 62), "rot=30", input_size=(44, 72), rot=30.0)
    assert a["trans_input"][0, 0, 1] != 0 and a["boxes"].any()


def test_a_rotation_with_nearest_boxes_equals_the_twin(pkg, gpu):
    """``boxes='nearest'`` where one sample's output map looks past all four sides of the canvas (three of these five do): the
    other nearest cases reach every side, but never all four in one sample."""
    _c, a = _check_chain(gpu, twin.batch(5, 62), "rot=30 nearest", input_size=(44, 72), rot=30.0, boxes="nearest")
    assert a["boxes"].any()


def test_identity_without_the_twin(pkg, gpu):
    """Unit scale (50 on a 30 x 50 canvas at input_size (30, 50)), the centre in the middle, alphas of 1, no lighting,
    down_ratio 1: orig_img is the canvas, inp its normalisation, and every box is its instance's visible rectangle."""
    from clean_pvnet_amd import ct_augment
    bg, inst_img, inst_mask, _cls, num, d = twin.batch(2, 63)
    inst_mask[:] = 0
    inst_mask[:, 0, 2:9, 3:11], inst_mask[:, 1, 0:4, 0:5], inst_mask[:, 2, 5:6, 7:8] = 1, 1, 1
    d[:, 1:3], d[:, 4:7], d[:, 7:10] = 0.5, 0.5, 0.0
    d[:, twin.N_SAMPLE:] = [0.0, 0.0, 0.5, 0.5, 0.99, 0.99]              # apart: the corner, the middle, the far corner
    c = ct_augment.ct_compose(_t(gpu, bg), _t(gpu, inst_img), _t(gpu, inst_mask), _t(gpu, num), d)
    a = ct_augment.ct_augment(c["img"], c["label"], d, input_size=(30, 50), down_ratio=1, scale_range=(1.0, 1.0), n_instances=3)
    c, a = _np(c), _np(a)
    assert a["center"].tolist() == [[25.0, 15.0]] * 2 and a["scale"].tolist() == [[50.0, 50.0]] * 2
    assert np.array_equal(a["trans_input"], np.tile(np.array([[1., 0., 0.], [0., 1., 0.]]), (2, 1, 1)))
    assert a["orig_img"].tobytes() == c["img"].tobytes()
    x = c["img"].astype(np.float32) / np.float32(255)
    want = ((x - np.asarray(twin.MEAN, np.float32)) / np.asarray(twin.STD, np.float32)).transpose(0, 3, 1, 2)
    assert a["inp"].tobytes() == np.ascontiguousarray(want).tobytes()
    for b in range(2):
        for n, (h, w) in enumerate(((6, 7), (3, 4), (0, 0))):
            y_min, x_min, ph, pw, dy, dx = c["place"][b, n]
            assert (ph, pw) == (h, w) and (c["label"][b, dy:dy + h + 1, dx:dx + w + 1] == n + 1).all()
            assert a["boxes"][b, n].tolist() == [dx, dy, min(dx + w + 1, 49), min(dy + h + 1, 29)]
            assert np.array_equal(c["img"][b, dy:dy + h + 1, dx:dx + w + 1], inst_img[b, n, y_min:y_min + h + 1, x_min:x_min + w + 1])


# ------------------------------------------------------------------------------------------------------------ 2. how it runs
def test_reruns_give_the_same_bytes(pkg, gpu):
    bg, inst_img, inst_mask, _cls, num, d = twin.batch(33, 64)
    first = _chain(gpu, bg, inst_img, inst_mask, num, d, input_size=(48, 264))
    for _ in range(3):
        again = _chain(gpu, bg, inst_img, inst_mask, num, d, input_size=(48, 264))
        assert all(again[0][k].tobytes() == first[0][k].tobytes() for k in COMPOSE_KEYS)
        assert all(again[1][k].tobytes() == first[1][k].tobytes() for k in AUGMENT_KEYS)


def test_strided_and_bool_inputs(pkg, gpu):
    import torch
    from clean_pvnet_amd import ct_augment
    bg, inst_img, inst_mask, _cls, num, d = twin.batch(5, 65)
    want_c = twin.compose(bg, inst_img, inst_mask, num, d)
    want_a = twin.augment(want_c["img"], want_c["label"], d, n_instances=3)
    wide_bg = torch.zeros(5, 30, 100, 3, dtype=torch.uint8, device=gpu)
    wide_bg[:, :, ::2] = _t(gpu, bg)
    wide_img = torch.zeros(5, 6, 12, 14, 3, dtype=torch.uint8, device=gpu)
    wide_img[:, ::2] = _t(gpu, inst_img)
    c = ct_augment.ct_compose(wide_bg[:, :, ::2], wide_img[:, ::2], _t(gpu, inst_mask != 0), _t(gpu, num.astype(np.int32)), d)
    _assert_same(_np(c), want_c, COMPOSE_KEYS, "strided compose")
    wide_c = torch.zeros(5, 60, 50, 3, dtype=torch.uint8, device=gpu)
    wide_c[:, ::2] = c["img"]
    wide_l = torch.zeros(5, 30, 50, 2, dtype=torch.uint8, device=gpu)
    wide_l[..., 0] = c["label"]
    a = ct_augment.ct_augment(wide_c[:, ::2], wide_l[..., 0], d, input_size=(44, 72), n_instances=3)
    _assert_same(_np(a), want_a, AUGMENT_KEYS, "strided augment")


def test_the_chain_reads_nothing_back(pkg, gpu):
    import torch
    from clean_pvnet_amd import ct_augment
    bg, inst_img, inst_mask, cls, num, d = twin.batch(5, 66)
    args = [_t(gpu, v) for v in (bg, inst_img, inst_mask, cls, num)]
    aug = ct_augment.CtAugment(num_classes=5, input_size=(44, 72))
    aug(*args, draws=d)                                                   # (the first call may allocate)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = aug(*args, draws=d)
        plain = ct_augment.ct_augment(args[0], None, None, train=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert batch["inp"].shape == (5, 3, 44, 72) and plain["inp"].shape == (5, 3, 32, 64)


def test_ct_augment_feeds_ct_targets(pkg, gpu):
    """``CtAugment`` -> ``ct_train.ct_targets`` against tests/ct_train_twin.py on the twin's boxes, and a step of the wrapper."""
    import torch
    from clean_pvnet_amd import ct_augment, ct_train
    bg, inst_img, inst_mask, cls, num, d = twin.mixed_batch()
    C = 5
    want_c = twin.compose(bg, inst_img, inst_mask, num, d)
    want_a = twin.augment(want_c["img"], want_c["label"], d, n_instances=3)
    want_t = ct_train_twin.ct_targets(want_a["boxes"], cls, num, C, 11, 18)
    batch = ct_augment.CtAugment(num_classes=C, input_size=(44, 72))(*[_t(gpu, v) for v in (bg, inst_img, inst_mask, cls, num)], draws=d)
    assert batch["inp"].cpu().numpy().tobytes() == want_a["inp"].tobytes() and batch["boxes"].cpu().numpy().tobytes() == want_a["boxes"].tobytes()
    for k in ("ct_hm", "wh", "ct_cls", "ct_ind", "ct_01", "ct_num"):
        got = batch[k].cpu().numpy()
        assert got.dtype == want_t[k].dtype and got.tobytes() == want_t[k].tobytes(), k
    assert want_t["ct_num"].sum() > 0 and want_t["ct_num"][6] == 0

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, C + 2, 4, stride=4)

        def forward(self, x):
            y = self.conv(x)
            return {"ct_hm": y[:, :C], "wh": y[:, C:]}
    torch.manual_seed(0)
    wrapper = ct_train.NetworkWrapper(Net().to(gpu))
    _out, loss, stats, _ = wrapper(batch)
    loss.backward()
    assert torch.isfinite(loss).item() and set(stats) == {"ct_loss", "wh_loss", "loss"} and wrapper.net.conv.weight.grad is not None
