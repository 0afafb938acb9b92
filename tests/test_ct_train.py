"""The detector's heat-map targets and training loss (include/pvnet_vote.h, "Detector training", clean_pvnet_amd.ct_train) without
a GPU: the numpy twin of the contract (tests/ct_train_twin.py) reproduces what the reference's own ``prepare_detection``,
``ct_collator`` and ``NetworkWrapper`` gave on the CPU (tests/golden/ct_train_*.npz, made by tests/golden/make_ct_train_golden.py)
-- indices, boxes, classes, weights, counts, radii, the whole heat map and the wh gradient bit for bit, both losses and the logit
gradient within one float32 ulp of the reference's float64 run, and within that ulp plus the reference's own measured
float32-float64 distance of its float32 run; the header, the symbols, the host-side refusals and the wrapper's checks are there.
The GPU tests (tests/test_gpu_ct_train.py) then hold the device to the twin.

The clamp: the reference's float64 run clamps the sigmoid to 1e-4 and 0.9999 in binary64, its float32 run (and the contract) to
the float32 values of the two.  log(1 - hi) differs by 1.66e-4 between them at every element clamped from above, so against the
float64 run the twin is evaluated with that run's own two constants, and against the float32 run with the contract's.  With the
contract's constants the distance to the float64 run was 0 ulps (c3_37x53), 2 (c30_34x45_int, no_pos), 145 (clamp12) and
149 (clamp30): the constants, not the arithmetic."""
import os

import numpy as np
import pytest

from tests import capi
from tests import ct_train_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
SYMBOLS = {"pvv_ct_targets", "pvv_ct_loss_workspace_bytes", "pvv_ct_loss_forward", "pvv_ct_loss_backward"}
TITLE = "Detector training: heat-map targets and the detector loss"
LO64, HI64 = 1e-4, 1 - 1e-4                                      # what torch.clamp compares a float64 tensor with


def _ulp(x):
    """The distance from |x| to the next float32 above it."""
    x = np.abs(np.float32(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


@pytest.fixture(scope="module", params=list(twin.GOLDEN_CASES))
def case(request):
    """(name, the stored results, the regenerated inputs)."""
    g, d = twin.load_golden(request.param), twin.golden_inputs(request.param)
    for k in ("boxes", "cls", "num"):
        assert g[k].dtype == d[k].dtype and g[k].tobytes() == d[k].tobytes()
    assert d["ct_hm_pred"].astype(np.float64).sum() == g["ct_hm_pred_sum"] and d["wh_pred"].astype(np.float64).sum() == g["wh_pred_sum"]
    return request.param, g, d


# ------------------------------------------------------------------------------------------------ 1. the twin against the reference
def test_golden_cases_hold_what_the_issue_asks():
    d = twin.golden_inputs("c3_37x53")
    r, ind, n = d["radius"][0], d["ct_ind"][0], int(d["ct_num"][0])
    assert d["boxes"].dtype == np.float32 and twin.golden_inputs("c30_34x45_int")["boxes"].dtype == np.int64
    assert (r[:n] == 0).any() and n < int(d["num"][0])                                       # a radius-0 object; some were dropped
    assert len(set(ind[:n].tolist())) < n                                                    # two objects with one centre
    cx, cy = ind[:n] % 53, ind[:n] // 53
    assert (cx - r[:n] < 0).any() and (cy - r[:n] < 0).any() and (cx + r[:n] >= 53).any() and (cy + r[:n] >= 37).any()
    assert ((cx + r[:n] >= 53) & (cy + r[:n] >= 37)).any()                                   # a corner
    assert (d["boxes"][0, 5, 0] == d["boxes"][0, 5, 2]) and int(d["num"][0]) > 6             # a degenerate box in the middle
    assert twin.one_object((1.0, 25.0, 6.0, 30.0), 0, 3, 37, 53)[0] == 4 and twin.one_object((2.0, 26.0, 7.0, 31.0), 0, 3, 37, 53)[0] == 4
    assert (d["ct_hm"][0] == 1).sum() == len(set(zip(d["ct_cls"][0, :n].tolist(), ind[:n].tolist())))
    assert (d["ct_hm"][0].reshape(3, -1).max(1) == 1).all() and ((d["ct_hm"] > 0) & (d["ct_hm"] < 1)).any()
    e = twin.golden_inputs("c30_34x45_int")
    assert e["num"].tolist() == [17, 130, 0] and e["ct_num"][2] == 0 and not e["ct_hm"][2].any() and e["cls"].shape == (3, 130)
    z = np.abs(d["ct_hm_pred"].astype(np.float64))
    assert (np.abs(z - twin.LN9999) >= 0.01).all() and (z > twin.LN9999).any()               # outside the band; some are clamped
    for name, v in (("clamp12", 12), ("clamp30", 30)):
        c = twin.golden_inputs(name)
        assert (c["ct_hm_pred"] == v).any() and (c["ct_hm_pred"] == -v).any()
        at = c["ct_hm_pred"][c["ct_hm"] == 1]
        assert (np.abs(at) == v).all() and len(at) >= 1                                      # positives are clamped too
    assert twin.golden_inputs("clamp30")["ct_hm_pred"].shape == (1, 4, 8, 12)
    assert not (twin.golden_inputs("no_pos")["ct_hm"] == 1).any()


def test_rows_and_radii_equal_the_references_bit_for_bit(case):
    name, g, d = case
    w = int(g["width"])
    assert w == max(1, int(g["ct_num"].max())) and d["ct_num"].tobytes() == g["ct_num"].tobytes()
    for k in ("ct_ind", "wh", "ct_cls", "ct_01", "radius"):
        got = np.ascontiguousarray(d[k][:, :w])
        assert got.dtype == g[k].dtype and got.tobytes() == g[k].tobytes(), k
        assert not d[k][:, w:].any(), k                                                      # the padding to N is zeros


def test_heat_map_equals_the_references_bit_for_bit(case):
    name, g, d = case
    assert d["ct_hm"].dtype == np.float32 and d["ct_hm"].shape == g["ct_hm"].shape
    centres = g["ct_hm"] == 1
    assert np.array_equal(d["ct_hm"] == 1, centres)
    diff = d["ct_hm"].view(np.uint32) != g["ct_hm"].view(np.uint32)
    print("%s: %d of %d heat-map elements differ, %d centres" % (name, diff.sum(), diff.size, centres.sum()))
    assert not diff.any()


def test_the_rule_that_is_left_out_never_fires():
    r = np.arange(0, 2001, dtype=np.float64)
    sigma = (2 * r + 1) / 6
    corner = np.exp(-((r * r) / (sigma * sigma) + (r * r) / (sigma * sigma)) / 2)
    assert corner.min() > 1.2e-4 > np.finfo(np.float64).eps


def test_losses_are_within_one_ulp_of_the_float64_run(case):
    name, g, d = case
    ct = twin.focal_loss(d["ct_hm_pred"], d["ct_hm"], lo=LO64, hi=HI64)
    wh = twin.wh_loss(d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"])
    e_ct, e_wh = abs(float(ct) - float(g["ct_loss64"])), abs(float(wh) - float(g["wh_loss64"]))
    print("%s: ct_loss %.9g (float64 run %.12g, |diff| %.3g, ulp %.3g); wh_loss %.9g (float64 run %.12g, |diff| %.3g, ulp %.3g)"
          % (name, ct, g["ct_loss64"], e_ct, _ulp(g["ct_loss64"]), wh, g["wh_loss64"], e_wh, _ulp(g["wh_loss64"])))
    assert ct.dtype == np.float32 and wh.dtype == np.float32
    assert e_ct <= _ulp(g["ct_loss64"]) and e_wh <= _ulp(g["wh_loss64"])


def test_losses_are_within_the_measured_distance_of_the_float32_run(case):
    name, g, d = case
    ct = twin.focal_loss(d["ct_hm_pred"], d["ct_hm"])
    wh = twin.wh_loss(d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"])
    e_ct, e_wh = abs(float(ct) - float(g["ct_loss"])), abs(float(wh) - float(g["wh_loss"]))
    b_ct, b_wh = _ulp(g["ct_loss"]) + float(g["ct_loss_f32_dist"]), _ulp(g["wh_loss"]) + float(g["wh_loss_f32_dist"])
    print("%s: ct_loss |diff| to the float32 run %.3g (bound %.3g); wh_loss %.3g (bound %.3g)" % (name, e_ct, b_ct, e_wh, b_wh))
    assert e_ct <= b_ct and e_wh <= b_wh


def test_logit_gradient_is_within_one_ulp_of_the_float64_run(case):
    name, g, d = case
    got32, got64 = twin.focal_grad(d["ct_hm_pred"], d["ct_hm"], lo=LO64, hi=HI64)
    apart = twin.ulp_apart(got32, g["hm_grad64"].astype(np.float32))
    print("%s: logit gradient at most %d float32 from the float64 run, %d of %d elements differ (the reference's float32 run: %d)"
          % (name, apart.max(), (apart > 0).sum(), apart.size, g["hm_grad_f32_ulps"]))
    assert apart.max() <= 1 and got32.tobytes() == got64.astype(np.float32).tobytes()
    mine = twin.focal_grad(d["ct_hm_pred"], d["ct_hm"])[0]                                   # the contract's constants: the same but in the band
    assert twin.ulp_apart(mine, got32).max() == 0
    s = 1 / (1 + np.exp(-d["ct_hm_pred"].astype(np.float64)))
    assert not mine[(s < twin.LO) | (s > twin.HI)].any() and mine[(s > twin.LO) & (s < twin.HI) & (d["ct_hm"] <= 1)].all()


def test_wh_gradient_equals_autograd_bit_for_bit(case):
    name, g, d = case
    assert int(g["wh_grad_ulps"]) == 0                                                       # what the script found
    got = twin.wh_grad(d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"], go=0.1)               # loss = ct_loss + 0.1 * wh_loss
    assert got.dtype == np.float32 and got.tobytes() == g["wh_grad"].tobytes()


def test_an_upstream_gradient_scales_as_the_contract_says():
    d = twin.golden_inputs("c3_37x53")
    g1, g2 = twin.focal_grad(d["ct_hm_pred"], d["ct_hm"], 1.0)[1], twin.focal_grad(d["ct_hm_pred"], d["ct_hm"], 2.0)[1]
    assert np.array_equal(g2, 2 * g1)                              # a power of two scales every operation exactly
    assert not twin.focal_grad(d["ct_hm_pred"], d["ct_hm"], 0.0)[0].any()
    a = (d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"])
    assert np.array_equal(twin.wh_grad(*a, go=2.0), 2 * twin.wh_grad(*a, go=1.0)) and not twin.wh_grad(*a, go=0.0).any()


def test_zero_weight_padding_changes_neither_loss():
    d = twin.golden_inputs("c3_37x53")
    w = int(d["ct_num"].max())
    cut = [d[k][:, :w] for k in ("wh", "ct_ind", "ct_01")]
    assert twin.wh_loss(d["wh_pred"], *cut).tobytes() == twin.wh_loss(d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"]).tobytes()
    assert twin.wh_grad(d["wh_pred"], *cut).tobytes() == twin.wh_grad(d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"]).tobytes()


# ------------------------------------------------------------------------------------------------ 2. the header and the symbols
def test_header_declares_and_library_exports_the_entry_points(pkg):
    raw = open(HEADER).read()
    declared = list(capi.native.declarations("pvnet_vote.h"))                                # in the header's order
    assert SYMBOLS <= set(declared) and set(declared[-8:-4]) == SYMBOLS                      # directly before the last section
    assert TITLE in raw and raw.index("Model metadata (ABI v8") < raw.index(TITLE) < raw.index("Training: vote targets and the PVNet loss")
    section = raw[raw.index(TITLE):raw.index("Training: vote targets and the PVNet loss")]
    for cite in ("lib/datasets/tless_train/ct.py:46-66", "lib/utils/data_utils.py:10-65", "lib/datasets/collate_batch.py:6-32",
                 "lib/train/trainers/ct.py:14-31", "lib/utils/net_utils.py:9-49", ":195-246"):
        assert cite in section
    for symbol, cite in (("pvv_ct_targets", "P:46-66"), ("pvv_ct_loss_forward", "T:20-26"), ("pvv_ct_loss_backward", "T:20-26")):
        before = section[:section.index("int %s(" % symbol)]
        assert cite in before[before.rindex("/*"):]                                          # each entry point cites what it replaces
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in raw                                                # additive: the version did not move
    import lib
    table = lib.load_build().HIP_LIBS
    assert len(table) == 7 and list(table)[-1] == "icp"
    assert "#define PVV_CT_TRAIN_MAX_N %d" % twin.MAX_N in raw
    for name, value in (("F32", 0), ("I32", 1), ("I64", 2)):
        assert "#define PVV_BOX_%s %d" % (name, value) in raw


def test_module_imports(pkg):
    import torch
    from clean_pvnet_amd import ct_train
    assert all(callable(getattr(ct_train, f)) for f in ("ct_targets", "ct_loss", "CtLoss", "NetworkWrapper"))
    assert ct_train.MAX_N == twin.MAX_N
    assert ct_train.BOX_KINDS == {torch.float32: 0, torch.int32: 1, torch.int64: 2}


# ------------------------------------------------------------------------------------------------ 3. the host-only checks
def _workspace(B, C, H, W):
    """What the layout of the header gives: per (image, tile) two binary64 and one int64, per image four binary64 and two int64,
    each of the four parts rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256                                                    # noqa: E731
    tiles = -(-C * H * W // twin.TILE)
    return up(B * tiles * 16) + up(B * tiles * 8) + up(B * 32) + up(B * 16)


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 37, 53), (1, 4, 8, 12), (1, 30, 135, 180), (32, 30, 135, 180)])
def test_workspace_sizes(B, C, H, W):
    got = capi.load().pvv_ct_loss_workspace_bytes(B, C, H, W)
    assert got == _workspace(B, C, H, W) and got % 256 == 0
    assert got < 1 << 20                                                                     # partials, not maps


def test_host_side_refusals():
    L = capi.load()
    x = 256                                                                                  # a pointer that is not NULL: never dereferenced

    def fwd(B=1, N=4, C=3, H=8, W=8, hp=x, wh=x, ind=x, strides=None, ws=x, nbytes=1 << 20, losses=x, state=x):
        hs, wsr, ms = strides or (C * H * W, 2 * H * W, C * H * W)
        return L.pvv_ct_loss_forward(hp, hs, x, wsr, x, ms, wh, ind, 1, x, B, N, C, H, W, ws, nbytes, losses, state, None)

    def bwd(B=1, N=4, C=3, H=8, W=8, hp=x, wh=x, ind=x, strides=None, state=x, go=x, gh=x):
        hs, wsr, ms = strides or (C * H * W, 2 * H * W, C * H * W)
        return L.pvv_ct_loss_backward(hp, hs, x, wsr, x, ms, wh, ind, 1, x, B, N, C, H, W, state, go, gh, x, None)

    def tgt(B=1, N=4, C=3, H=8, W=8, boxes=x, kind=0, hm=x, num=x):
        return L.pvv_ct_targets(boxes, kind, x, 1, num, 1, B, N, C, H, W, hm, x, x, x, x, x, None)

    for f in (fwd, bwd, tgt):
        assert f(B=0) == -1 and f(C=0) == -1 and f(H=0) == -1 and f(W=-1) == -1 and b"positive" in L.pvv_last_error()
        assert f(B=65536) == -1 and b"65535" in L.pvv_last_error()
        assert f(N=0) == -1 and f(N=513) == -1 and b"N must lie in [1, 512]" in L.pvv_last_error()
        assert f(C=1, H=46341, W=46341) == -1 and b"2^31" in L.pvv_last_error()              # 2*H*W
        assert f(C=30, H=8462, W=8462) == -1 and b"2^31" in L.pvv_last_error()               # C*H*W
    for f in (fwd, bwd):
        assert f(hp=None) == -1 and b"NULL" in L.pvv_last_error()
        assert f(wh=None) == -1 and f(ind=None) == -1 and b"NULL" in L.pvv_last_error()
        assert f(B=2, strides=(3 * 64 - 1, 2 * 64, 3 * 64)) == -1 and b"image stride" in L.pvv_last_error()
        assert f(B=2, strides=(3 * 64, 2 * 64 - 1, 3 * 64)) == -1 and b"image stride" in L.pvv_last_error()
        assert f(B=2, strides=(3 * 64, 2 * 64, 3 * 64 - 1)) == -1 and b"image stride" in L.pvv_last_error()
        assert f(state=None) == -1 and b"NULL" in L.pvv_last_error()
        assert f(state=260) == -1 and b"8-byte aligned" in L.pvv_last_error()
    assert fwd(losses=None) == -1 and b"NULL" in L.pvv_last_error()
    assert fwd(ws=None) == -1 and b"NULL workspace" in L.pvv_last_error()
    assert fwd(ws=264) == -1 and b"256-byte aligned" in L.pvv_last_error()
    assert fwd(nbytes=255) == -2 and b"too small" in L.pvv_last_error()
    assert bwd(go=None) == -1 and bwd(gh=None) == -1 and b"NULL" in L.pvv_last_error()
    assert tgt(boxes=None) == -1 and tgt(hm=None) == -1 and tgt(num=None) == -1 and b"NULL" in L.pvv_last_error()
    assert tgt(kind=3) == -1 and tgt(kind=-1) == -1 and b"box_kind" in L.pvv_last_error()
    assert L.pvv_ct_loss_workspace_bytes(1, 30, 8462, 8462) == 0 and b"2^31" in L.pvv_last_error()
    assert L.pvv_ct_loss_workspace_bytes(0, 3, 8, 8) == 0 and b"positive" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 4. the wrapper's checks
def _meta(*shape, **kw):
    import torch
    return torch.empty(*shape, device="meta", **kw)


def _loss_args():
    import torch
    return [_meta(2, 3, 4, 5), _meta(2, 2, 4, 5), _meta(2, 3, 4, 5), _meta(2, 6, 2), _meta(2, 6, dtype=torch.int64), _meta(2, 6)]


def test_cpu_tensors_are_refused(pkg):
    import torch
    from clean_pvnet_amd import ct_train
    hp, wp, hm = torch.zeros(1, 3, 4, 5), torch.zeros(1, 2, 4, 5), torch.zeros(1, 3, 4, 5)
    wh, ind, w01 = torch.zeros(1, 6, 2), torch.zeros(1, 6, dtype=torch.int64), torch.zeros(1, 6)
    with pytest.raises(RuntimeError, match="ct_hm_pred must be a CUDA tensor; there is no CPU fallback"):
        ct_train.ct_loss(hp, wp, hm, wh, ind, w01)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ct_train.CtLoss()(hp, wp, hm, wh, ind, w01)
    with pytest.raises(RuntimeError, match="boxes must be a CUDA tensor"):
        ct_train.ct_targets(torch.zeros(1, 6, 4), ind, torch.zeros(1, dtype=torch.int64), 3, 4, 5)


def test_dtypes_grads_and_shapes_are_refused_in_that_order(pkg):
    import torch
    from clean_pvnet_amd import ct_train
    real_need = ct_train._native.need_cuda
    ct_train._native.need_cuda = lambda *a: None                                             # past the device check: dtype, grad, then shapes
    names = ["ct_hm_pred", "wh_pred", "ct_hm", "wh", "ct_ind", "ct_01"]
    try:
        for i, name in enumerate(names):
            a = _loss_args()
            a[i] = _meta(9, 9, dtype=torch.float16)                                          # (the dtype comes before the shape)
            want = "ct_ind must be int32 or int64, got torch.float16" if name == "ct_ind" else "%s must be float32, got torch.float16" % name
            with pytest.raises(RuntimeError, match=want):
                ct_train.ct_loss(*a)
        for i, name in enumerate(names):
            if i < 2 or name == "ct_ind":
                continue
            a = _loss_args()
            a[i] = _meta(*a[i].shape, requires_grad=True)
            with pytest.raises(RuntimeError, match="%s requires grad; gradients go to ct_hm_pred and wh_pred only" % name):
                ct_train.ct_loss(*a)
        bad = {"ct_hm_pred": _meta(2, 3, 4), "wh_pred": _meta(2, 3, 4, 5), "ct_hm": _meta(2, 3, 5, 4), "wh": _meta(2, 6, 3),
               "ct_ind": _meta(2, 7, dtype=torch.int64), "ct_01": _meta(3, 6)}
        for i, name in enumerate(names):
            a = _loss_args()
            a[i] = bad[name]
            with pytest.raises(ValueError, match="%s must be" % name):
                ct_train.ct_loss(*a)
        a = _loss_args()
        a[3], a[4], a[5] = _meta(2, 513, 2), _meta(2, 513, dtype=torch.int64), _meta(2, 513)
        with pytest.raises(ValueError, match="N must lie in \\[1, 512\\]"):
            ct_train.ct_loss(*a)
        boxes, cls, num = _meta(2, 6, 4), _meta(2, 6, dtype=torch.int64), _meta(2, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="boxes must be float32 or int32 or int64, got torch.float64"):
            ct_train.ct_targets(boxes.double(), cls, num, 3, 4, 5)
        with pytest.raises(RuntimeError, match="cls must be int32 or int64"):
            ct_train.ct_targets(boxes, _meta(2, 6), num, 3, 4, 5)
        with pytest.raises(RuntimeError, match="num must be int32 or int64"):
            ct_train.ct_targets(boxes, cls, _meta(2), 3, 4, 5)
        with pytest.raises(ValueError, match="boxes must be \\[B, N, 4\\]"):
            ct_train.ct_targets(_meta(2, 6, 5), cls, num, 3, 4, 5)
        with pytest.raises(ValueError, match="cls must be"):
            ct_train.ct_targets(boxes, _meta(2, 5, dtype=torch.int64), num, 3, 4, 5)
        with pytest.raises(ValueError, match="num must be"):
            ct_train.ct_targets(boxes, cls, _meta(3, dtype=torch.int64), 3, 4, 5)
        with pytest.raises(ValueError, match="must be positive and N in \\[1, 512\\]"):
            ct_train.ct_targets(boxes, cls, num, 0, 4, 5)
        with pytest.raises(ValueError, match="must be positive and N in \\[1, 512\\]"):
            ct_train.ct_targets(_meta(2, 513, 4), _meta(2, 513, dtype=torch.int64), num, 3, 4, 5)
    finally:
        ct_train._native.need_cuda = real_need


def test_network_wrapper_has_the_references_contract(pkg):
    import torch
    from torch import nn
    from clean_pvnet_amd import ct_train

    class Net(nn.Module):
        def forward(self, inp):
            return {"ct_hm": inp[:, :3], "wh": inp[:, 3:]}

    w = ct_train.NetworkWrapper(Net())
    assert isinstance(w.net, Net) and list(w.state_dict()) == []
    inp = torch.zeros(1, 5, 4, 6)
    seen = {}
    real_loss, real_targets = ct_train.ct_loss, ct_train.ct_targets

    def fake_loss(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01):
        seen.update(ct_hm=ct_hm, wh=wh, ct_ind=ct_ind, ct_01=ct_01, C=ct_hm_pred.shape[1], wh_channels=wh_pred.shape[1])
        return torch.tensor(0.25), torch.tensor(0.5)

    def fake_targets(boxes, cls, num, num_classes, height, width):
        seen.update(boxes=boxes, sizes=(num_classes, height, width))
        return "hm", "wh", "cls", "ind", "01", "num"

    ct_train.ct_loss, ct_train.ct_targets = fake_loss, fake_targets
    try:
        batch = {"inp": inp, "ct_hm": torch.zeros(1, 3, 4, 6), "wh": torch.zeros(1, 2, 2), "ct_ind": torch.zeros(1, 2, dtype=torch.int64),
                 "ct_01": torch.zeros(1, 2), "boxes": torch.zeros(1, 2, 4)}
        output, loss, scalar_stats, image_stats = w(batch)
        assert set(output) == {"ct_hm", "wh"} and list(scalar_stats) == ["ct_loss", "wh_loss", "loss"] and image_stats == {}
        assert float(loss) == np.float32(0.25) + np.float32(0.1) * np.float32(0.5) and scalar_stats["loss"] is loss
        assert seen["ct_hm"] is batch["ct_hm"] and seen["ct_ind"] is batch["ct_ind"] and "boxes" not in seen       # shipped targets win
        assert (seen["C"], seen["wh_channels"]) == (3, 2)
        batch = {"inp": inp, "boxes": torch.zeros(1, 2, 4), "cls": torch.zeros(1, 2, dtype=torch.int64), "num": torch.zeros(1, dtype=torch.int64)}
        w(batch)
        assert seen["boxes"] is batch["boxes"] and seen["sizes"] == (3, 4, 6) and (seen["ct_hm"], seen["ct_ind"], seen["ct_01"]) == ("hm", "ind", "01")
    finally:
        ct_train.ct_loss, ct_train.ct_targets = real_loss, real_targets
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        w(batch)
