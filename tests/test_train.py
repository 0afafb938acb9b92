"""PVNet's vote targets and training loss (include/pvnet_vote.h's last section, clean_pvnet_amd.train) without a GPU: the numpy
twin of the contract (tests/train_twin.py) reproduces what the reference's own ``compute_vertex`` and ``NetworkWrapper`` gave
on the CPU (tests/golden/train_*.npz, made by tests/golden/make_train_golden.py) -- target and vote gradient bit for bit, the
losses and the seg gradient within the bounds derived in the twin; its sums do not depend on the order tiles are evaluated in;
the header, the symbols, the host-side refusals and the wrapper's checks are there.  The GPU tests (tests/test_gpu_train.py)
then hold the device to the twin."""
import os

import numpy as np
import pytest

from tests import capi
from tests import train_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
SYMBOLS = {"pvv_vertex_target", "pvv_pvnet_loss_workspace_bytes", "pvv_pvnet_loss_forward", "pvv_pvnet_loss_backward"}


@pytest.fixture(scope="module", params=list(twin.GOLDEN_CASES))
def case(request):
    """(name, the stored results, the regenerated inputs)."""
    g, d = twin.load_golden(request.param), twin.golden_inputs(request.param)
    assert np.array_equal(g["mask"], d["mask"]) and g["kpt_2d"].tobytes() == d["kpt_2d"].tobytes()
    assert d["vertex_pred"].astype(np.float64).sum() == g["vertex_pred_sum"] and d["seg_pred"].astype(np.float64).sum() == g["seg_pred_sum"]
    return request.param, g, d


# ------------------------------------------------------------------------------------------------ 1. the twin against the reference
def test_golden_cases_hold_what_the_issue_asks():
    g, d = twin.load_golden("k9_c2_37x53"), twin.golden_inputs("k9_c2_37x53")
    assert tuple(g["sizes"][:5]) == (2, 9, 2, 37, 53)
    mask, kpt = d["mask"], d["kpt_2d"]
    for b in range(2):                                            # on a pixel centre, 5e-4 px and 1.5e-3 px from one
        y, x = np.argwhere(mask[b] == 1).T
        near = np.sqrt((kpt[b, :3, None, 0] - x) ** 2 + (kpt[b, :3, None, 1] - y) ** 2).min(1)
        assert near[0] == 0 and abs(near[1] - 5e-4) < 1e-9 and abs(near[2] - 1.5e-3) < 1e-9
    dd, _ = twin.vote_d(d["vertex_pred"], d["target"], mask)
    assert (dd > 1).sum() > 100 and (dd < -1).sum() > 100          # saturated on both sides
    assert (d["seg_pred"] == 40).any() and (d["seg_pred"] == -40).any()
    assert set(np.unique(twin.golden_inputs("k1_c3_8x12")["mask"])) == {0, 1, 2}
    e = twin.golden_inputs("empty_beside")["mask"]
    assert not e[0].any() and e[1].any()


def test_target_equals_the_references_bit_for_bit(case):
    name, g, d = case
    got = twin.compute_vertex(d["mask"], d["kpt_2d"])
    assert got.dtype == np.float32 and got.tobytes() == g["target"].tobytes()
    got32 = twin.compute_vertex(d["mask"], d["kpt_2d"].astype(np.float32))         # float32 keypoints are widened exactly
    want32 = twin.compute_vertex(d["mask"], d["kpt_2d"].astype(np.float32).astype(np.float64))
    assert got32.tobytes() == want32.tobytes()


def test_vote_gradient_equals_autograd_bit_for_bit(case):
    name, g, d = case
    got = twin.vote_grad(d["vertex_pred"], g["target"], d["mask"])
    assert got.tobytes() == g["vote_grad"].tobytes()


def test_vote_loss_is_within_its_bounds(case):
    name, g, d = case
    got, _ = twin.vote_loss(d["vertex_pred"], g["target"], d["mask"])
    e64, e32 = abs(float(got) - float(g["vote_loss64"])), abs(float(got) - float(g["vote_loss"]))
    b64, b32 = twin.vote_bound_f64(g["vote_loss64"]), twin.vote_bound_f32(g["vote_loss"], d["vertex_pred"].size)
    print("%s vote loss %.9g: |diff| to the float64 run %.3g (bound %.3g), to the float32 run %.3g (bound %.3g)" % (name, got, e64, b64, e32, b32))
    assert got.dtype == np.float32 and e64 <= b64 and e32 <= b32


def test_seg_loss_is_within_its_bounds(case):
    name, g, d = case
    B, K, C, H, W, _ = g["sizes"]
    got, _ = twin.seg_loss(d["seg_pred"], d["mask"])
    e64, e32 = abs(float(got) - float(g["seg_loss64"])), abs(float(got) - float(g["seg_loss"]))
    b64 = twin.seg_bound_f64(g["seg_loss64"])
    b32 = twin.seg_bound_f32(g["seg_loss"], B * H * W, C, float(np.abs(d["seg_pred"]).max()))
    print("%s seg loss %.9g: |diff| to the float64 run %.3g (bound %.3g), to the float32 run %.3g (bound %.3g)" % (name, got, e64, b64, e32, b32))
    assert got.dtype == np.float32 and e64 <= b64 and e32 <= b32


def test_seg_gradient_is_within_its_bound_of_the_float64_run(case):
    name, g, d = case
    B, K, C, H, W, _ = g["sizes"]
    got32, got64 = twin.seg_grad(d["seg_pred"], d["mask"])
    zrange = float(d["seg_pred"].max() - d["seg_pred"].min())
    bound = twin.seg_grad_bound_f64(C, zrange, 1.0, B * H * W)
    err = np.abs(got64 - g["seg_grad64"]).max()
    print("%s seg gradient: max |diff| to the float64 run %.3g, bound %.3g" % (name, err, bound))
    assert err <= bound and got32.tobytes() == got64.astype(np.float32).tobytes()
    label = d["mask"].astype(np.int64)[:, None]
    at_label = np.arange(C)[None, :, None, None] == label
    assert (got64[at_label] <= 0).all() and (got64[~at_label] >= 0).all()          # the label's entry is never p - 1 rounded up


def test_an_upstream_gradient_scales_as_the_contract_says():
    d, g = twin.golden_inputs("k1_c3_8x12"), twin.load_golden("k1_c3_8x12")
    go = np.float32(-0.37)
    dd, w = twin.vote_d(d["vertex_pred"], g["target"], d["mask"])
    s = (go / np.float32(2)) / np.float32(twin.mask_sum(d["mask"]))
    want = np.where(dd < -1, -s, np.where(dd > 1, s, s * dd)) * w
    assert twin.vote_grad(d["vertex_pred"], g["target"], d["mask"], go).tobytes() == want.astype(np.float32).tobytes()
    g1, g2 = twin.seg_grad(d["seg_pred"], d["mask"], 1.0)[1], twin.seg_grad(d["seg_pred"], d["mask"], 2.0)[1]
    assert np.array_equal(g2, 2 * g1)                              # a power of two scales every operation exactly


# ------------------------------------------------------------------------------------------------ 2. the sums
def test_sum_does_not_depend_on_the_order_tiles_are_evaluated_in():
    rng = np.random.default_rng(3)
    terms = rng.random(300 * twin.TILE - 517) * 10.0 ** rng.integers(-8, 8, 300 * twin.TILE - 517)   # 300 tiles, the last partial
    in_order = twin.tile_sums(terms)
    assert in_order.shape == (300,)
    order = rng.permutation(300)
    shuffled = np.empty(300)
    for chunk in np.array_split(order, 7):                        # another grid: seven launches over tiles in any order
        shuffled[chunk] = twin.tile_sums(terms, chunk)
    assert shuffled.tobytes() == in_order.tobytes()
    total = twin.image_sum(in_order)
    assert twin.image_sum(shuffled).tobytes() == total.tobytes()
    assert total != np.sum(terms) or total != np.add.reduce(terms[::-1])   # (an order does matter for these terms)
    exact = float(sum(map(__import__("fractions").Fraction, terms.tolist())))
    assert abs(total - exact) <= terms.size * twin.V * exact


def test_block_sum_order():
    a = 2.0 ** -np.arange(256.0)                                    # slot 0 meets slot 128 first: 1 + 2^-128 rounds to 1
    want = a.copy()
    s = 128
    while s:
        want[:s] += want[s:2 * s]
        s //= 2
    assert twin.block_sum(a) == want[0]
    assert twin.tile_sums(np.ones(5))[0] == 5 and twin.tile_sums(np.ones(1025)).tolist() == [1024.0, 1.0]


# ------------------------------------------------------------------------------------------------ 3. the header and the symbols
def test_header_declares_and_library_exports_the_entry_points(pkg):
    raw = open(HEADER).read()
    declared = list(capi.native.declarations("pvnet_vote.h"))                       # in the header's order
    assert SYMBOLS <= set(declared) and set(declared[-4:]) == SYMBOLS               # the last section of the header
    assert "Training: vote targets and the PVNet loss" in raw
    section = raw[raw.index("Training: vote targets and the PVNet loss"):]
    for cite in ("pvnet_data_utils.py:30-44", "lib/train/trainers/pvnet.py:25-34", "resnet18.py:93-94"):
        assert cite in section
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in raw                                      # additive: the version did not move
    import lib
    table = lib.load_build().HIP_LIBS
    assert len(table) == 7 and list(table)[-1] == "icp"
    for name, value in (("LANE_PIXELS", twin.LANE), ("TILE", twin.TILE), ("IMAGE_SLOTS", twin.SLOTS), ("MAX_K", twin.MAX_K), ("MAX_C", twin.MAX_C)):
        assert "#define PVV_TRAIN_%s %d" % (name, value) in raw


def test_module_imports(pkg):
    from clean_pvnet_amd import train
    assert all(callable(getattr(train, f)) for f in ("compute_vertex", "pvnet_loss", "PVNetLoss", "NetworkWrapper"))
    assert (train.MAX_K, train.MAX_C) == (twin.MAX_K, twin.MAX_C)


# ------------------------------------------------------------------------------------------------ 4. the host-only checks
def _workspace(B, H, W):
    """What the layout of the header gives: per (image, tile) two binary64 and two int64, the same per image, each of the four
    parts rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256                                           # noqa: E731
    tiles = -(-H * W // twin.TILE)
    return up(B * tiles * 16) + up(B * tiles * 16) + up(B * 16) + up(B * 16)


@pytest.mark.parametrize("B,H,W", [(1, 37, 53), (1, 480, 640), (64, 480, 640)])
def test_workspace_sizes(B, H, W):
    got = capi.load().pvv_pvnet_loss_workspace_bytes(B, H, W)
    assert got == _workspace(B, H, W) and got % 256 == 0
    assert got < 1 << 20                                                            # partials, not fields


def test_host_side_refusals():
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced

    def fwd(B=1, K=9, C=2, H=8, W=8, kpt=x, target=None, vp=x, strides=None, kind=0, ws=x, nbytes=1 << 20):
        vs, ss, ts = strides or (2 * K * H * W, C * H * W, 2 * K * H * W)
        return L.pvv_pvnet_loss_forward(vp, vs, x, ss, x, kind, kpt, 0, target, ts, B, K, C, H, W, ws, nbytes, x, x, None)

    def bwd(B=1, K=9, C=2, H=8, W=8, kpt=x, target=None, state=x):
        return L.pvv_pvnet_loss_backward(x, 2 * K * H * W, x, C * H * W, x, 0, kpt, 0, target, 2 * K * H * W, B, K, C, H, W, state, x, x, x, None)

    for f in (fwd, bwd):
        assert f(C=17) == -1 and b"C must lie in [1, 16]" in L.pvv_last_error()
        assert f(K=65) == -1 and b"K must lie in [1, 64]" in L.pvv_last_error()
        assert f(K=0) == -1 and f(C=0) == -1 and f(B=0) == -1 and b"positive" in L.pvv_last_error()
        assert f(H=46341, W=46341) == -1 and b"2^31" in L.pvv_last_error()         # H*W itself
        assert f(K=64, H=4096, W=4096) == -1 and b"2^31" in L.pvv_last_error()     # 2K*H*W
        assert f(B=65536) == -1 and b"65535" in L.pvv_last_error()
        assert f(kpt=x, target=x) == -1 and b"exactly one" in L.pvv_last_error()
        assert f(kpt=None, target=None) == -1 and b"exactly one" in L.pvv_last_error()
    assert fwd(vp=None) == -1 and b"NULL" in L.pvv_last_error()
    assert fwd(kind=3) == -1 and b"mask_kind" in L.pvv_last_error()
    assert fwd(B=2, strides=(2 * 9 * 64 - 1, 2 * 64, 0)) == -1 and b"image stride" in L.pvv_last_error()
    assert fwd(B=2, kpt=None, target=x, strides=(2 * 9 * 64, 2 * 64, 2 * 9 * 64 - 1)) == -1 and b"image stride" in L.pvv_last_error()
    assert fwd(ws=None) == -1 and b"NULL workspace" in L.pvv_last_error()
    assert fwd(ws=264) == -1 and b"256-byte aligned" in L.pvv_last_error()
    assert fwd(nbytes=255) == -2 and b"too small" in L.pvv_last_error()
    assert bwd(state=None) == -1 and b"NULL" in L.pvv_last_error()
    assert L.pvv_pvnet_loss_workspace_bytes(1, 46341, 46341) == 0 and b"2^31" in L.pvv_last_error()
    assert L.pvv_pvnet_loss_workspace_bytes(0, 8, 8) == 0 and b"positive" in L.pvv_last_error()
    assert L.pvv_vertex_target(x, 0, x, 0, 1, 65, 8, 8, x, None) == -1 and b"K must lie" in L.pvv_last_error()
    assert L.pvv_vertex_target(x, 0, None, 0, 1, 9, 8, 8, x, None) == -1 and b"NULL" in L.pvv_last_error()
    assert L.pvv_vertex_target(x, 7, x, 0, 1, 9, 8, 8, x, None) == -1 and b"mask_kind" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 5. the wrapper's checks
def _meta(*shape, **kw):
    import torch
    return torch.empty(*shape, device="meta", **kw)


def test_cpu_tensors_are_refused(pkg):
    import torch
    from clean_pvnet_amd import train
    vp, sp, m, kp = torch.zeros(1, 4, 3, 5), torch.zeros(1, 2, 3, 5), torch.zeros(1, 3, 5, dtype=torch.uint8), torch.zeros(1, 2, 2)
    with pytest.raises(RuntimeError, match="vertex_pred must be a CUDA tensor; there is no CPU fallback"):
        train.pvnet_loss(vp, sp, m, kpt_2d=kp)
    with pytest.raises(RuntimeError, match="mask must be a CUDA tensor"):
        train.compute_vertex(m, kp)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        train.PVNetLoss()(vp, sp, m, vertex=torch.zeros(1, 4, 3, 5))


def test_dtypes_forms_and_shapes_are_refused_in_that_order(pkg):
    import torch
    from clean_pvnet_amd import train
    vp, sp, m, kp, tg = _meta(2, 4, 3, 5), _meta(2, 2, 3, 5), _meta(2, 3, 5, dtype=torch.uint8), _meta(2, 2, 2), _meta(2, 4, 3, 5)
    with pytest.raises(ValueError, match="exactly one of kpt_2d and vertex"):
        train.pvnet_loss(vp, sp, m, kpt_2d=kp, vertex=tg)
    with pytest.raises(ValueError, match="exactly one of kpt_2d and vertex"):
        train.pvnet_loss(vp, sp, m)
    real_need = train._native.need_cuda
    train._native.need_cuda = lambda *a: None                                       # past the device check: dtype, grad, then shapes
    try:
        with pytest.raises(RuntimeError, match="vertex_pred must be float32, got torch.float16"):
            train.pvnet_loss(_meta(2, 4, 3, 5, dtype=torch.float16), sp, m, kpt_2d=_meta(9, 9))   # (the dtype comes before the shape)
        with pytest.raises(RuntimeError, match="seg_pred must be float32"):
            train.pvnet_loss(vp, sp.half(), m, kpt_2d=kp)
        with pytest.raises(RuntimeError, match="vertex must be float32"):
            train.pvnet_loss(vp, sp, m, vertex=tg.double())
        with pytest.raises(RuntimeError, match="mask must be uint8, bool, int32 or int64"):
            train.pvnet_loss(vp, sp, _meta(2, 3, 5), kpt_2d=kp)
        with pytest.raises(RuntimeError, match="kpt_2d must be float32 or float64"):
            train.pvnet_loss(vp, sp, m, kpt_2d=_meta(2, 2, 2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="vertex requires grad"):
            train.pvnet_loss(vp, sp, m, vertex=_meta(2, 4, 3, 5, requires_grad=True))
        with pytest.raises(RuntimeError, match="kpt_2d requires grad"):
            train.pvnet_loss(vp, sp, m, kpt_2d=_meta(2, 2, 2, requires_grad=True))
        with pytest.raises(ValueError, match="vertex_pred must be"):
            train.pvnet_loss(_meta(2, 4, 3, 6), sp, m, kpt_2d=kp)
        with pytest.raises(ValueError, match="vertex_pred must be"):
            train.pvnet_loss(_meta(2, 5, 3, 5), sp, m, kpt_2d=kp)                  # an odd number of channels
        with pytest.raises(ValueError, match="seg_pred must be"):
            train.pvnet_loss(vp, _meta(1, 2, 3, 5), m, kpt_2d=kp)
        with pytest.raises(ValueError, match="kpt_2d has 3 keypoints, vertex_pred 2"):
            train.pvnet_loss(vp, sp, m, kpt_2d=_meta(2, 3, 2))
        with pytest.raises(ValueError, match="kpt_2d must be"):
            train.pvnet_loss(vp, sp, m, kpt_2d=_meta(2, 2, 3))
        with pytest.raises(ValueError, match="vertex must be"):
            train.pvnet_loss(vp, sp, m, vertex=_meta(2, 4, 5, 3))
        with pytest.raises(ValueError, match="mask must be"):
            train.pvnet_loss(vp, sp, _meta(2, 1, 3, 5, dtype=torch.uint8), kpt_2d=kp)
        with pytest.raises(ValueError, match="C in \\[1, 16\\]"):
            train.pvnet_loss(vp, _meta(2, 17, 3, 5), m, kpt_2d=kp)
        with pytest.raises(ValueError, match="kpt_2d must be"):
            train.compute_vertex(m, _meta(3, 2, 2))
    finally:
        train._native.need_cuda = real_need


def test_network_wrapper_has_the_references_contract(pkg):
    import torch
    from torch import nn
    from clean_pvnet_amd import train

    class Net(nn.Module):
        def forward(self, inp):
            return {"seg": inp[:, :2], "vertex": inp[:, 2:]}

    w = train.NetworkWrapper(Net())
    assert isinstance(w.net, Net) and list(w.state_dict()) == []
    inp = torch.zeros(1, 6, 3, 5)
    output, loss, scalar_stats, image_stats = w({"inp": inp, "meta": {"pose_test": 1}})     # no mask and no target are touched
    assert set(output) == {"seg", "vertex"} and loss.dim() == 0 and int(loss) == 0 and scalar_stats == {} and image_stats == {}
    seen = {}
    real = train.pvnet_loss

    def fake(vertex_pred, seg_pred, mask, *, kpt_2d=None, vertex=None):
        seen.update(kpt_2d=kpt_2d, vertex=vertex, K=vertex_pred.shape[1] // 2, C=seg_pred.shape[1])
        return torch.tensor(0.25), torch.tensor(0.5)

    train.pvnet_loss = fake
    try:
        batch = {"inp": inp, "mask": torch.zeros(1, 3, 5, dtype=torch.uint8), "kpt_2d": torch.zeros(1, 2, 2), "meta": {}}
        output, loss, scalar_stats, image_stats = w(batch)
        assert list(scalar_stats) == ["vote_loss", "seg_loss", "loss"] and image_stats == {}
        assert float(loss) == 0.75 and scalar_stats["loss"] is loss and float(scalar_stats["vote_loss"]) == 0.25
        assert seen["kpt_2d"] is batch["kpt_2d"] and seen["vertex"] is None and (seen["K"], seen["C"]) == (2, 2)
        batch["vertex"] = torch.zeros(1, 4, 3, 5)                                  # a loader that still ships the field: it wins
        w(batch)
        assert seen["vertex"] is batch["vertex"] and seen["kpt_2d"] is None
    finally:
        train.pvnet_loss = real
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        w(batch)
