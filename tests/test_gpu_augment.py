"""PVNet's augmentation and loader transforms on the MI355X (clean_pvnet_amd.augment) against the numpy twin
(tests/augment_twin.py, itself pinned in tests/test_augment.py): all five outputs of ``pvnet_augment`` and the float output of
``pvnet_transform`` as bytes, an identity case that does not go through the twin, reruns, strided inputs, float32 keypoints, and
the chain ``PVNetAugment`` -> ``train.pvnet_loss(kpt_2d=...)`` against tests/train_twin.py.

The base shape is 48 x 70 (a width that is a multiple of neither 4 nor 64; two blocks of 64 lanes per row) with ``out_size``
(40, 66).  At that pair a window can pad both axes or the columns alone, never the rows alone (th / 48 < tw / 70 for every
ratio), so the mixed batch runs a second time at ``out_size`` (44, 40), where it is the rows: between them crop on both axes,
pad on both, pad on either axis alone, an empty mask and a single-pixel mask, at the degrees -30, 0 and 30."""
import numpy as np
import pytest

from tests import augment_twin as twin
from tests import train_twin

pytestmark = pytest.mark.gpu
KEYS = ("img", "mask", "kpt_2d", "path", "window")
JITTER = (0.1, 0.1, 0.05, 0.05)                 # transforms.py:86


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _augment(gpu, img, mask, kpt, out_size, d, **kw):
    from clean_pvnet_amd.augment import pvnet_augment
    out = pvnet_augment(_t(gpu, img), _t(gpu, mask), _t(gpu, kpt), out_size, d, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        diff = got[k].view(np.uint8) != want[k].view(np.uint8)
        print("%s: %s: %d of %d bytes differ" % (what, k, diff.sum(), diff.size))
    assert all(got[k].tobytes() == want[k].tobytes() for k in KEYS), what


def _tiled(B, out_size):
    """The mixed batch repeated to ``B`` samples with fresh draws in the placement columns."""
    img, mask, kpt, d = twin.mixed_batch(out_size)
    idx = np.arange(B) % 5
    d = d[idx].copy()
    d[:, 2:] = twin.draws_for(B, 5)[:, 2:]
    return img[idx], mask[idx], kpt[idx], d


# ------------------------------------------------------------------------------------------------------------ 1. the geometry
@pytest.mark.parametrize("out_size", [(40, 66), (44, 40)])
def test_geometry_equals_the_twin_on_the_mixed_batch(pkg, gpu, out_size):
    img, mask, kpt, d = twin.mixed_batch(out_size)
    want = twin.pvnet_augment(img, mask, kpt, out_size, d, **twin.MIXED_KW)
    w = want["window"]
    H, W = mask.shape[1:]
    assert want["path"].tolist() == [1, 1, 1, 0, 1]
    assert w[0, 0] < H and w[0, 1] < W and w[1, 0] >= H and w[1, 1] >= W and (w[2, 0] >= H) != (w[2, 1] >= W)     # crop, pad, one axis
    assert (w[2, 0] >= H) == (out_size == (44, 40))                                                # the rows alone at (44, 40)
    assert [twin.degree_of(u, twin.MIXED_ROTATE) for u in d[:, 0]] == [-30, 0, 30, 30, -30]
    _assert_same(_augment(gpu, img, mask, kpt, out_size, d, **twin.MIXED_KW), want, "B=5 %s" % (out_size,))


@pytest.mark.parametrize("B", [1, 33])
def test_geometry_equals_the_twin_at_other_batch_sizes(pkg, gpu, B):
    img, mask, kpt, d = _tiled(B, (40, 66))
    want = twin.pvnet_augment(img, mask, kpt, (40, 66), d, **twin.MIXED_KW)
    _assert_same(_augment(gpu, img, mask, kpt, (40, 66), d, **twin.MIXED_KW), want, "B=%d" % B)


def test_default_ranges_and_the_empty_rotation_equal_the_twin(pkg, gpu):
    """The default ranges on seeded draws, and path 2: two pixels in opposite corners leave the image under a rotation of -30
    degrees around their centre, so the rotated mask is empty and the sample takes the steps of path 0."""
    img, mask, kpt, _ = twin.mixed_batch((40, 66))
    d = twin.draws_for(5, 77)
    want = twin.pvnet_augment(img, mask, kpt, (40, 66), d)
    _assert_same(_augment(gpu, img, mask, kpt, (40, 66), d), want, "defaults")
    m2, d2 = twin.empty_rotation_case()
    want = twin.pvnet_augment(img[:1], m2[None], kpt[:1], (40, 66), d2[None])
    assert want["path"].tolist() == [2]
    _assert_same(_augment(gpu, img[:1], m2[None], kpt[:1], (40, 66), d2[None]), want, "empty rotation")


def test_identity_returns_the_input(pkg, gpu):
    """Degree 0, ratio 1, out_size = the input's size: nothing is resampled off the grid.  Independent of the twin."""
    img, mask, kpt, d = twin.mixed_batch((40, 66))
    H, W = mask.shape[1:]
    got = _augment(gpu, img, mask, kpt, (H, W), d, rotate=(0, 0), resize_ratio=(1.0, 1.0))
    assert got["img"].tobytes() == img.tobytes() and got["mask"].tobytes() == mask.tobytes()
    assert got["kpt_2d"].tobytes() == kpt.tobytes()
    assert got["window"].tolist() == [[H, W, 0, 0, 0, 0]] * 5 and got["path"].tolist() == [1, 1, 1, 0, 1]


def test_reruns_strides_and_float32_keypoints(pkg, gpu):
    from clean_pvnet_amd.augment import pvnet_augment
    img, mask, kpt, d = twin.mixed_batch((40, 66))
    a = _augment(gpu, img, mask, kpt, (40, 66), d, **twin.MIXED_KW)
    _assert_same(_augment(gpu, img, mask, kpt, (40, 66), d, **twin.MIXED_KW), a, "rerun")
    wide_i, wide_m, wide_k = _t(gpu, np.concatenate([img, img], 2)), _t(gpu, np.concatenate([mask, mask], 2)), _t(gpu, np.concatenate([kpt, kpt], 2))
    vi, vm, vk = wide_i[:, :, :70], wide_m[:, :, :70], wide_k[:, :, :2]
    assert not vi.is_contiguous() and not vm.is_contiguous() and not vk.is_contiguous()
    out = pvnet_augment(vi, vm, vk, (40, 66), d, **twin.MIXED_KW)
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, a, "strided views")
    out = pvnet_augment(_t(gpu, img), _t(gpu, mask != 0), _t(gpu, kpt), (40, 66), d, **twin.MIXED_KW)        # a bool mask
    want = twin.pvnet_augment(img, (mask != 0).astype(np.uint8), kpt, (40, 66), d, **twin.MIXED_KW)
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, "bool mask")
    k32 = kpt.astype(np.float32)
    assert (k32.astype(np.float64) != kpt).any()
    got = _augment(gpu, img, mask, k32, (40, 66), d, **twin.MIXED_KW)
    assert got["kpt_2d"].dtype == np.float64
    _assert_same(got, twin.pvnet_augment(img, mask, k32.astype(np.float64), (40, 66), d, **twin.MIXED_KW), "float32 keypoints")


# ------------------------------------------------------------------------------------------------------------ 2. the transforms
def _transform(gpu, img, d, **kw):
    from clean_pvnet_amd.augment import pvnet_transform
    kw.setdefault("mean", twin.MEAN)
    kw.setdefault("std", twin.STD)
    return pvnet_transform(_t(gpu, img), d, **kw).cpu().numpy()


def _same_floats(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print("%s: %d of %d floats differ" % (what, diff.sum(), diff.size))
    assert not diff.any(), what


@pytest.mark.parametrize("shape", [(12, 9), (40, 66)])
def test_blur_equals_the_twin(pkg, gpu, shape):
    """Blur off and k = 3, 5, 7, 9 in one batch, no jitter; at 12 x 9 the reflection of 4 pixels reaches across most of the image."""
    img = np.stack([twin.image(40 + i, *shape) for i in range(5)])
    d = twin.draws_for(5, 8)
    d[:, 4], d[:, 5] = [0.9, 0.1, 0.1, 0.1, 0.1], [0.0, 0.0, 0.25, 0.5, 0.75]
    assert [twin.jitter_of(u)[0] for u in d] == [0, 3, 5, 7, 9]
    want = twin.pvnet_transform(img, d, jitter=(0, 0, 0, 0))
    assert (want[1:] != twin.pvnet_transform(img[1:], None)).any()
    _same_floats(_transform(gpu, img, d, jitter=(0, 0, 0, 0)), want, "blur %s" % (shape,))


def test_jitter_equals_the_twin(pkg, gpu):
    """Each operation alone (the other amplitudes 0), then four of the 24 orders with a blur in front."""
    img = np.stack([twin.image(50 + i, 40, 66) for i in range(4)])
    d = twin.draws_for(4, 9)
    d[:, 4] = 0.9
    for amp in ((0.4, 0, 0, 0), (0, 0.4, 0, 0), (0, 0, 0.4, 0), (0, 0, 0, 0.5)):
        _same_floats(_transform(gpu, img, d, jitter=amp), twin.pvnet_transform(img, d, jitter=amp), "alone %s" % (amp,))
    d[:, 4], d[:, 10] = 0.1, (np.array([0, 7, 14, 21]) + 0.5) / 24
    orders = [twin.jitter_of(u, jitter=(0.4, 0.4, 0.4, 0.5))[2] for u in d]
    assert orders == [[0, 1, 2, 3], [1, 0, 3, 2], [2, 1, 0, 3], [3, 1, 2, 0]]
    want = twin.pvnet_transform(img, d, jitter=(0.4, 0.4, 0.4, 0.5))
    _same_floats(_transform(gpu, img, d, jitter=(0.4, 0.4, 0.4, 0.5)), want, "orders %s" % (orders,))
    _same_floats(_transform(gpu, img, d, jitter=JITTER), twin.pvnet_transform(img, d, jitter=JITTER), "the reference's amplitudes")


def test_contrast_boundary_and_no_draws(pkg, gpu):
    """Half the pixels at L = 100 and half at 101: the mean is 100.5 and the grey level int(100.5 + 0.5) = 101."""
    img = twin.contrast_boundary_image()
    assert twin.contrast_grey(img) == 101 and int(twin.luma(img).sum()) * 2 == 201 * img.shape[0] * img.shape[1]
    d = twin.draws_for(1, 10)
    d[0, 4], d[0, 7] = 0.9, 0.95
    want = twin.pvnet_transform(img[None], d, jitter=(0, 0.5, 0, 0))
    _same_floats(_transform(gpu, img[None], d, jitter=(0, 0.5, 0, 0)), want, "contrast boundary")
    _same_floats(_transform(gpu, img[None], None), twin.pvnet_transform(img[None], None), "normalisation only")
    tiny = twin.image(3, 5, 6)[None]                                             # below 8 pixels: fine without draws
    _same_floats(_transform(gpu, tiny, None), twin.pvnet_transform(tiny, None), "5 x 6, normalisation only")


def test_transform_reruns_and_strides(pkg, gpu):
    from clean_pvnet_amd.augment import pvnet_transform
    img = np.stack([twin.image(60 + i, 40, 66) for i in range(3)])
    d = twin.draws_for(3, 12)
    d[:, 4] = 0.1
    a = _transform(gpu, img, d, jitter=JITTER)
    _same_floats(_transform(gpu, img, d, jitter=JITTER), a, "rerun")
    view = _t(gpu, np.concatenate([img, img], 2))[:, :, 66:]
    assert not view.is_contiguous()
    _same_floats(pvnet_transform(view, d, jitter=JITTER, mean=twin.MEAN, std=twin.STD).cpu().numpy(), a, "strided view")


# ------------------------------------------------------------------------------------------------------------ 3. the chain
def test_chain_into_the_training_loss(pkg, gpu):
    """``PVNetAugment`` -> ``train.pvnet_loss(kpt_2d=...)`` on one stream: the batch equals the twin's as bytes and the losses
    equal tests/train_twin.py on the twin's outputs under test_gpu_train's rule (vote loss as bytes, seg loss within a
    neighbouring float32)."""
    import torch
    from clean_pvnet_amd.augment import PVNetAugment
    from clean_pvnet_amd.train import pvnet_loss
    H, W, K, C, size = 48, 70, 9, 2, (40, 66)
    masks = np.stack([twin.blob(H, W, 14, 33, 22, 51), twin.blob(H, W, 5, 20, 40, 69), np.zeros((H, W), np.uint8)])
    img = np.stack([twin.image(70 + i, H, W) for i in range(3)])
    kpt = np.stack([twin.keypoints(masks[i], K, 80 + i) for i in range(3)])
    d = twin.draws_for(3, 13)
    aug = PVNetAugment()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    rng = np.random.default_rng(14)
    vp, sp = rng.standard_normal((3, 2 * K, *size)).astype(np.float32), rng.standard_normal((3, C, *size)).astype(np.float32)
    ti, tm, tk, tvp, tsp = _t(gpu, img), _t(gpu, masks), _t(gpu, kpt), _t(gpu, vp), _t(gpu, sp)
    torch.cuda.synchronize(gpu)
    with torch.cuda.stream(side):
        batch = aug(ti, tm, tk, *size, draws=d)
        vote, seg = pvnet_loss(tvp, tsp, batch["mask"], kpt_2d=batch["kpt_2d"])
    side.synchronize()
    g = twin.pvnet_augment(img, masks, kpt, size, d)
    inp = twin.pvnet_transform(g["img"], d)
    assert batch["mask"].cpu().numpy().tobytes() == g["mask"].tobytes() and batch["kpt_2d"].cpu().numpy().tobytes() == g["kpt_2d"].tobytes()
    _same_floats(batch["inp"].cpu().numpy(), inp, "inp")
    target = train_twin.compute_vertex(g["mask"], g["kpt_2d"])
    want_vote, want_seg = train_twin.vote_loss(vp, target, g["mask"])[0], train_twin.seg_loss(sp, g["mask"])[0]
    print("vote %r twin %r; seg %r twin %r" % (vote.item(), want_vote, seg.item(), want_seg))
    assert np.isfinite(want_vote) and vote.cpu().numpy().tobytes() == np.float32(want_vote).tobytes()
    assert train_twin.ulp_apart(seg.cpu().numpy(), np.float32(want_seg)) <= 1
    ev = PVNetAugment(train=False)(ti, tm, tk, *size)
    _same_floats(ev["inp"].cpu().numpy(), twin.pvnet_transform(img, None), "train=False")
    assert ev["mask"] is tm and ev["kpt_2d"] is tk
