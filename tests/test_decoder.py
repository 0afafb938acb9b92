"""PVNet's decoder stages (include/pvnet_vote.h, "PVNet decoder stage"; ``pvnet_stage`` and ``PVNetDecoder`` of clean_pvnet_amd.head)
without a GPU: the stage twin (tests/decoder_twin.py) is the head's twin stopped after the activation; it stays within its bound
of torch's own modules in float64 and leaves it when a rule is stated wrongly; the module has the reference's names; and the
library takes the stage flags of ``out_kind`` -- with pointers that are never dereferenced, every call ends in a refusal before
any launch.  The GPU tests (tests/test_gpu_decoder.py) then hold the device to the twin bit for bit."""
import json
import os
import re

import numpy as np
import pytest

from tests import decoder_twin as twin
from tests import head_twin as ht
from tests.test_head import _within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
STAGE, SAME_RES = 0x400, 0x800


# ------------------------------------------------------------------------------------------------ 1. the twin
@pytest.mark.parametrize("name", list(ht.CASES))
def test_the_stage_twin_is_the_head_twins_activation(name):
    d = ht.reference(name)
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(d["t"] > 0, d["t"], d["t"] * F32(0.1)).astype(F32)
    got = twin.stage(d["fm"], d["x"], d["weight1"], d["scale"], d["shift"])
    assert got.dtype == F32 and got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def torch64():
    """name -> (torch's own modules on the case's inputs in float64, eval mode, CPU; stage64's value; its bound), once per case."""
    import torch
    from torch import nn
    cache = {}

    def run(name):
        if name not in cache:
            d = twin.reference(name)
            conv = nn.Sequential(nn.Conv2d(d["C2"] + d["C0"], d["M"], 3, 1, 1, bias=False), nn.BatchNorm2d(d["M"]),
                                 nn.LeakyReLU(0.1, True)).double().eval()
            t = lambda a: torch.tensor(a).double()                                   # noqa: E731
            with torch.no_grad():
                conv[0].weight.copy_(t(d["weight"]))
                for p, k in ((conv[1].weight, "gamma"), (conv[1].bias, "beta"), (conv[1].running_mean, "mean"), (conv[1].running_var, "var")):
                    p.copy_(t(d[k]))
                assert conv[1].eps == d["eps"]
                fm = nn.UpsamplingBilinear2d(scale_factor=2)(t(d["a"])) if d["up"] else t(d["a"])
                want = conv(torch.cat([fm, t(d["skip"])], 1)).numpy()
            bn = (d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
            cache[name] = (want,) + twin.stage64(d["a"], d["skip"], d["weight"], bn, d["slope"], up=d["up"])
        return cache[name]
    return run


@pytest.mark.parametrize("name", list(twin.CASES))
def test_the_stage_twin_is_within_stage64s_bound_of_torchs_modules(torch64, name):
    d = twin.reference(name)
    want, a64, bound = torch64(name)
    worst = _within(d["out"], want, bound)                                          # equal NaN sets, equal infinities
    f = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(d["out"].astype(np.float64) - want)[f]
    print("%s: max |stage - torch64| = %.3g, worst err / bound = %.3g, stage64 against torch64: %.3g of the bound"
          % (name, err.max(), worst, _within(a64, want, bound)))
    assert d["out"].shape == (d["B"], d["M"], d["H"], d["W"]) and worst <= 1 and err.max() > 0
    assert f.any() and np.isnan(want).any()                                         # the NaN reached some outputs and spared others
    assert _within(a64, want, bound) < 1e-3                                         # the binary64 twin is torch's function


def test_cases_are_the_issues_and_hold_the_plants():
    c = twin.CASES
    assert [(n, c[n]["B"], c[n]["C2"], c[n]["C0"], c[n]["h"], c[n]["w"], c[n]["M"], c[n]["up"]) for n in twin.ISSUE_CASES] == [
        ("one_by_one", 2, 3, 1, 1, 1, 2, True), ("odd_chunks", 1, 70, 59, 5, 9, 5, True), ("no_skip_same_res", 2, 5, 0, 9, 35, 97, False),
        ("stage_4s", 1, 128, 64, 5, 17, 64, True), ("stage_8s", 1, 256, 128, 9, 33, 128, False), ("stage_2s", 1, 64, 64, 4, 16, 32, True)]
    assert c["split_rows"]["M"] > 64 and c["split_rows"]["up"]
    for name in c:
        d = twin.reference(name)
        assert np.isnan(d["a"]).sum() == 1 and np.isposinf(d["a"]).sum() == 1 and np.isfinite(d["skip"]).all()
        assert d["gamma"][0] == 0 and d["var"][1] == 0 and d["shift"][0] == 0 and np.signbit(d["shift"][0])
        assert (np.signbit(d["out"]) & (d["out"] == 0)).any(), name                # an activation that is exactly -0
        if d["M"] >= 3:
            assert d["mean"][2] == 1e6
    dec = twin.decoder_reference()
    assert dec["out"].shape == (1, 20, 16, 24) and np.isnan(dec["out"]).any() and np.isfinite(dec["out"]).sum() > dec["out"].size // 2


# ------------------------------------------------------------------------------------------------ 2. mutations
MUTATIONS = {
    "skip_channels_first": (dict(order="skip_a"), ("odd_chunks", "split_rows", "stage_2s")),
    "align_corners_false": (dict(coords="half_pixel"), ("odd_chunks", "split_rows", "stage_2s")),
    "replicated_ring": (dict(ring="edge"), ("odd_chunks", "no_skip_same_res", "split_rows")),
    "slope_0.01": (dict(slope=0.01), ("one_by_one", "odd_chunks", "no_skip_same_res")),
    "upsample_where_same_res_was_meant": (dict(crop=True), ("no_skip_same_res",)),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_rule_stated_wrongly_leaves_the_bound(torch64, mutation):
    kw, names = MUTATIONS[mutation]
    kw = dict(kw)
    slope = kw.pop("slope", 0.1)
    worst = {}
    for name in names:
        d = twin.reference(name)
        want, _, bound = torch64(name)
        assert _within(d["out"], want, bound) <= 1                                  # the rule stated rightly does not
        out = twin.stage(d["a"], d["skip"], d["weight"], d["scale"], d["shift"], slope, up=d["up"], **kw)
        worst[name] = _within(out, want, bound)
    print(mutation, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1


# ------------------------------------------------------------------------------------------------ 3. the module
def test_module_imports_and_leaves_the_head_as_it_was(pkg):
    from clean_pvnet_amd import head
    assert all(callable(getattr(head, f)) for f in ("pvnet_stage", "PVNetDecoder", "cached_fold", "pvnet_head", "PVNetHead"))
    assert head.MAX_M == 64 and head.MAX_STAGE_M == 128 and (head.STAGE, head.SAME_RES) == (STAGE, SAME_RES)


def test_state_dict_keys_are_the_references(pkg):
    import torch
    from clean_pvnet_amd import head
    with open(os.path.join(ROOT, "tests", "golden", "pvnet_decoder_keys.json")) as f:
        keys = json.load(f)
    m = head.PVNetDecoder(ver_dim=18, seg_dim=2)
    sd = m.state_dict()
    assert list(sd) == keys
    shapes = {"conv8s.0.weight": (128, 384, 3, 3), "conv4s.0.weight": (64, 192, 3, 3), "conv2s.0.weight": (32, 128, 3, 3),
              "convraw.0.weight": (32, 35, 3, 3), "convraw.3.weight": (20, 32, 1, 1)}
    assert all(tuple(sd[k].shape) == v for k, v in shapes.items())
    with torch.no_grad():
        for bn in (m.conv8s[1], m.conv2s[1]):
            bn.running_mean.normal_()
    whole = {"resnet18_8s.conv1.weight": torch.zeros(1), **{k: v.clone() for k, v in sd.items()}}   # a network's checkpoint
    again = head.PVNetDecoder.from_state_dict(whole)
    assert not again.training and (again.ver_dim, again.seg_dim) == (18, 2) and list(again.state_dict()) == keys
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), m.state_dict().values()))
    small = head.PVNetDecoder.from_state_dict(head.PVNetDecoder(4, 3, fcdim=7, s8dim=6, s4dim=5, s2dim=4, raw_dim=9).state_dict(), seg_dim=3)
    assert (small.ver_dim, small.seg_dim) == (4, 3) and tuple(small.conv8s[0].weight.shape) == (6, 135, 3, 3)
    assert tuple(small.conv4s[0].weight.shape) == (5, 70, 3, 3) and tuple(small.convraw[0].weight.shape) == (9, 7, 3, 3)


def test_from_module_shares_storage_and_the_fold_is_cached_per_stage(pkg):
    import torch
    from torch import nn
    from clean_pvnet_amd import head

    class Net(nn.Module):                                                           # the four Sequentials of a reference network
        def __init__(self):
            super().__init__()
            src = head.PVNetDecoder(4, 2, fcdim=8, s8dim=6, s4dim=5, s2dim=4, raw_dim=7)
            self.ver_dim, self.seg_dim = 4, 2
            self.conv8s, self.conv4s, self.conv2s, self.convraw = src.conv8s, src.conv4s, src.conv2s, src.convraw
    net = Net().eval()
    m = head.PVNetDecoder.from_module(net)
    assert not m.training and (m.ver_dim, m.seg_dim) == (4, 2)
    for name in ("conv8s", "conv4s", "conv2s", "convraw"):
        assert getattr(m, name) is getattr(net, name)
    assert {p.data_ptr() for p in m.parameters()} == {p.data_ptr() for p in net.parameters()}
    a = m.folded("conv4s")
    assert m.folded("conv4s")[0] is a[0] and m.folded("conv2s")[0] is not a[0]       # folded once, per stage
    with torch.no_grad():
        net.conv4s[1].running_var.mul_(4)                                           # the network's buffer is the decoder's
    b = m.folded("conv4s")
    assert b[0] is not a[0] and torch.equal(b[0], head.fold_bn(net.conv4s[1])[0]) and not torch.equal(b[0], a[0])
    h = head.PVNetHead(4, 2, s2dim=3, raw_dim=5).eval()                            # PVNetHead goes through the same helper
    assert h.folded()[0] is h.folded()[0] and torch.equal(h.folded()[1], head.fold_bn(h.convraw[1])[1])


def test_training_mode_cpu_tensors_and_the_136_row_shape_are_refused(pkg):
    import torch
    from clean_pvnet_amd import head
    m = head.PVNetDecoder(4, 2, fcdim=8, s8dim=6, s4dim=5, s2dim=4, raw_dim=7)
    x, x2s, x4s, x8s, xfc = (torch.zeros(1, c, s, s) for c, s in ((3, 16), (64, 8), (64, 4), (128, 2), (8, 2)))
    with pytest.raises(RuntimeError, match="forward only.*eval"):                  # a new module is in training mode
        m(x, x2s, x4s, x8s, xfc)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"), torch.no_grad():
        m.eval()(x, x2s, x4s, x8s, xfc)
    w, s = torch.zeros(5, 6, 3, 3), torch.zeros(5)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        head.pvnet_stage(xfc, x8s, w, s, s)
    meta = lambda *shape, **k: torch.empty(*shape, device="meta", **k)              # noqa: E731
    real_need = head._native.need_cuda
    head._native.need_cuda = lambda *a: None                                        # past the device check: dtype, grad, shapes
    try:
        with pytest.raises(RuntimeError, match="forward only"):                    # its parameters require grad
            m.eval().to("meta")(*(t.to("meta") for t in (x, x2s, x4s, x8s, xfc)))
        with pytest.raises(RuntimeError, match="136.*not supported"):             # up8sto4s gives 136 rows, x4s has 135
            head.pvnet_stage(meta(1, 4, 68, 90), meta(1, 2, 135, 180), meta(5, 6, 3, 3), meta(5), meta(5))
        with pytest.raises(RuntimeError, match="not supported"):
            head.pvnet_stage(meta(1, 4, 9, 9), meta(1, 2, 18, 18), meta(5, 6, 3, 3), meta(5), meta(5), upsample=False)
        with pytest.raises(ValueError, match="128"):
            head.pvnet_stage(meta(1, 4, 9, 9), meta(1, 2, 18, 18), meta(129, 6, 3, 3), meta(129), meta(129))
        with pytest.raises(RuntimeError, match="float32"):
            head.pvnet_stage(meta(1, 4, 9, 9, dtype=torch.float16), meta(1, 2, 18, 18), meta(5, 6, 3, 3), meta(5), meta(5))
        with pytest.raises(RuntimeError, match="forward only"):
            head.pvnet_stage(meta(1, 4, 9, 9), meta(1, 2, 18, 18), meta(5, 6, 3, 3, requires_grad=True), meta(5), meta(5))
        with pytest.raises(RuntimeError, match="out_dtype"):
            head.pvnet_stage(meta(1, 4, 9, 9), meta(1, 2, 18, 18), meta(5, 6, 3, 3), meta(5), meta(5), out_dtype=torch.float64)
    finally:
        head._native.need_cuda = real_need


# ------------------------------------------------------------------------------------------------ 4. the flags of out_kind
def test_the_header_states_the_stage_flags_and_adds_no_symbol():
    from tests import capi
    with open(os.path.join(ROOT, "include", "pvnet_vote.h")) as f:
        text = f.read()
    assert re.search(r"^#define PVV_HEAD_STAGE\s+0x400\b", text, re.M)
    assert re.search(r"^#define PVV_HEAD_SAME_RES\s+0x800\b", text, re.M)
    assert re.search(r"^#define PVV_HEAD_STAGE_MAX_M\s+128$", text, re.M)
    assert re.search(r"^#define PVV_ABI_VERSION 8$", text, re.M)
    heads = {sym for sym in capi.declared() if sym.startswith("pvv_head_")}
    assert heads == {"pvv_head_forward", "pvv_head_upsample"} and heads <= capi.exported()


def test_the_stage_flags_are_accepted_and_checked_before_any_launch():
    """Fails on the parent commit, where PVV_HEAD_OUT_F32 | 0x400 is an unknown dtype code.  No call here reaches a launch: a
    call that passes the pointer check is given an H of more tiles than one launch takes, the check that follows it."""
    from tests import capi
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    up = dict(B=2, C2=4, C0=3, h=5, w=6, H=10, W=12, M1=8, M2=6)
    same = dict(up, H=5, W=6)
    tall = dict(h=262144, w=1, H=524288, W=2)                                        # 65536 tiles along H: refused after the pointers
    tall_same = dict(h=524288, w=2, H=524288, W=2)

    def fwd(shape, ptrs=(x,) * 8, kind=STAGE, **over):
        s = {**shape, **over}
        fm_stride, x_stride = s["C2"] * s["h"] * s["w"], s["C0"] * s["H"] * s["W"]
        return L.pvv_head_forward(ptrs[0], fm_stride, ptrs[1], x_stride, *ptrs[2:7], s["B"], s["C2"], s["C0"], s["h"], s["w"], s["H"],
                                  s["W"], s["M1"], s["M2"], 0.1, kind, ptrs[7], None)

    def refused(rc, word):
        msg = L.pvv_last_error()
        assert rc == -1 and word in msg, (rc, msg)
        return True

    for shape, tall_shape, flags in ((up, tall, STAGE), (same, tall_same, STAGE | SAME_RES)):
        for code in (0, 1, 2):                                                      # the flags with each dtype code pass the kind check
            assert refused(fwd(shape, (None,) * 8, kind=flags | code), b"NULL") and b"dtype code" not in L.pvv_last_error()
        for i in (0, 1, 2, 3, 4, 7):                                                # each of the six pointers a stage reads, alone
            assert refused(fwd(shape, tuple(None if j == i else x for j in range(8)), kind=flags), b"NULL")
        no_conv2 = (x, x, x, x, x, None, None, x)                                   # d_weight2 and d_bias2 are not read
        assert refused(fwd(shape, no_conv2, kind=flags, **tall_shape), b"too large for one launch")
        assert refused(fwd(shape, no_conv2, kind=flags, M2=0, **tall_shape), b"too large for one launch")     # nor is M2
        assert refused(fwd(shape, (x, None, x, x, x, None, None, x), kind=flags, C0=0, **tall_shape), b"too large")   # d_x with C0 = 0
        assert refused(fwd(shape, kind=flags | 3), b"dtype code")
        assert refused(fwd(shape, kind=flags, B=0), b"positive") and refused(fwd(shape, kind=flags, B=65536), b"65535")
        assert refused(fwd(shape, kind=flags, M1=128, **tall_shape), b"too large for one launch")             # past the M check
        assert refused(fwd(shape, kind=flags, M1=129), b"<= 128")
        assert refused(fwd(shape, kind=flags, C2=400, **tall_shape), b"too large for one launch") and b"LDS" not in L.pvv_last_error()
    assert refused(fwd(up, kind=STAGE | SAME_RES), b"PVV_HEAD_SAME_RES")            # H = 2h under SAME_RES
    assert refused(fwd(same, kind=STAGE), b"2*h")                                   # and H = h without it
    big = dict(C2=1, C0=0, h=23171, w=23171, H=46342, W=46342)                      # H * W > 2^31
    assert refused(fwd(up, kind=STAGE, **big), b"2^31")
    assert refused(fwd(up, kind=STAGE, C2=1, C0=0, h=2048, w=2048, H=4096, W=4096, M1=128), b"2^31")       # the output's M1 * H * W
    for kind in (SAME_RES, STAGE | 0x100, STAGE | SAME_RES | 0x100, STAGE | 0x200, STAGE | 0x1000, SAME_RES | 0x100):
        assert refused(fwd(up, kind=kind), b"dtype code"), kind
    assert refused(fwd(up, kind=0, M1=65), b"<= 64")                                # without the flag the head is what it was
    assert refused(fwd(up, kind=0, C2=120), b"LDS")
