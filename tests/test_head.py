"""PVNet's output head (include/pvnet_vote.h, "PVNet output head", clean_pvnet_amd.head) without a GPU: the module, the two entry points
and their argument checks exist; the numpy twin of the contract (tests/head_twin.py) stays within its derived bound of the
reference's own expression -- torch's modules as lib/networks/pvnet/resnet18.py:53-59, 90-92 state it, eval mode, float64 -- and
leaves that bound as soon as one of the contract's rules is stated wrongly.  The GPU tests (tests/test_gpu_head.py) then hold the
device to the twin bit for bit."""
import os

import numpy as np
import pytest

from tests import capi
from tests import head_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
SYMBOLS = {"pvv_head_forward", "pvv_head_upsample"}
F32 = np.float32


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import head
    assert all(callable(getattr(head, f)) for f in ("pvnet_head", "upsample2x", "fold_bn", "PVNetHead"))
    assert head.MAX_UPSAMPLE == 1 << 28 and head.MAX_M == 64


def test_header_declares_and_library_exports_the_two_entry_points():
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in open(HEADER).read()                      # additive: the version did not move


def test_host_side_argument_checks():
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    ok = dict(B=2, C2=4, C0=3, h=5, w=6, H=10, W=12, M1=8, M2=6)

    def fwd(ptrs=(x,) * 8, fm_stride=4 * 30, x_stride=3 * 120, kind=0, **over):
        s = {**ok, **over}
        return L.pvv_head_forward(ptrs[0], fm_stride, ptrs[1], x_stride, *ptrs[2:7], s["B"], s["C2"], s["C0"], s["h"], s["w"], s["H"],
                                  s["W"], s["M1"], s["M2"], 0.1, kind, ptrs[7], None)

    assert fwd((None,) * 8) == -1 and b"NULL" in L.pvv_last_error()
    for i in range(8):                                                              # every pointer alone
        assert fwd(tuple(None if j == i else x for j in range(8))) == -1 and b"NULL" in L.pvv_last_error()
    for name in ("B", "C2", "M1", "M2"):
        assert fwd(**{name: 0}) == -1 and b"positive" in L.pvv_last_error()
    assert fwd(h=0, H=0) == -1 and b"positive" in L.pvv_last_error()
    assert fwd(C0=-1) == -1 and b"not negative" in L.pvv_last_error()
    assert fwd(H=11) == -1 and b"2*h" in L.pvv_last_error()
    assert fwd(W=11) == -1 and b"2*w" in L.pvv_last_error()
    assert fwd(M1=65) == -1 and b"<= 64" in L.pvv_last_error()
    assert fwd(M2=65) == -1 and b"<= 64" in L.pvv_last_error()
    assert fwd(fm_stride=4 * 30 - 1) == -1 and b"image stride" in L.pvv_last_error()
    assert fwd(x_stride=3 * 120 - 1) == -1 and b"image stride" in L.pvv_last_error()
    big = dict(C2=1, C0=0, h=23171, w=23171, H=46342, W=46342)                      # H * W > 2^31
    assert fwd(fm_stride=23171 * 23171, **big) == -1 and b"2^31" in L.pvv_last_error()
    assert fwd(kind=3) == -1 and b"dtype code" in L.pvv_last_error()
    assert fwd(kind=-1) == -1 and b"dtype code" in L.pvv_last_error()
    assert fwd(C2=120, fm_stride=120 * 30) == -1 and b"LDS" in L.pvv_last_error()  # the halo of 123 channels does not fit
    up = lambda ptrs, stride, shape: L.pvv_head_upsample(ptrs[0], stride, *shape, ptrs[1], None)   # noqa: E731
    assert up((None, None), 120, (2, 4, 5, 6, 10, 12)) == -1 and b"NULL" in L.pvv_last_error()
    assert up((x, x), 120, (2, 4, 5, 6, 10, 13)) == -1 and b"2*w" in L.pvv_last_error()
    assert up((x, x), 119, (2, 4, 5, 6, 10, 12)) == -1 and b"image stride" in L.pvv_last_error()
    assert up((x, x), 120, (0, 4, 5, 6, 10, 12)) == -1 and b"positive" in L.pvv_last_error()
    assert up((x, x), 64 * 512 * 512, (5, 64, 512, 512, 1024, 1024)) == -1 and b"2^28" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 1. the upsample
def _torch_upsample64(fm):
    import torch
    with torch.no_grad():
        return torch.nn.UpsamplingBilinear2d(scale_factor=2)(torch.tensor(fm).double()).numpy()


def _within(got, want, bound):
    """NaN sets equal, infinities equal, and every finite value within its bound; returns the largest error / bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]):
        return np.inf
    f = np.isfinite(want)
    if not np.isfinite(got[f]).all() or not np.isfinite(bound[f]).all():
        return np.inf
    err = np.abs(got[f] - want[f])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound[f])
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize("name", list(twin.CASES))
def test_twin_upsample_is_within_its_bound_of_torch_float64(name):
    d = twin.reference(name)
    want = _torch_upsample64(d["fm"])
    u64, bound = twin.upsample64(d["fm"])
    worst = _within(d["u"], want, bound)
    f = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err, err64 = np.abs(d["u"].astype(np.float64) - want)[f], np.abs(u64 - want)[f]
    print("%s: max |u - torch64| = %.3g, worst err / bound = %.3g, |u64 - torch64| = %.3g" % (name, err.max(), worst, err64.max()))
    assert worst <= 1
    if d["h"] == 1:
        assert twin.same_bits(d["u"][1], np.broadcast_to(d["fm"][1], d["u"][1].shape))      # r = 0: every output is the one input
        assert np.isnan(d["u"][0, 0]).all() and np.isnan(d["u"][0, 1]).all()                  # Inf * 0 is NaN: the zero weight multiplies
    else:
        assert err.max() > 0                                                                  # (float32 does round here)


def test_twin_upsample_axis_is_the_float32_formula():
    i0, i1, l0, l1, src = twin.axis(240, 480)
    r = F32(239) / F32(479)
    assert src.dtype == F32 and np.array_equal(src, r * np.arange(480, dtype=F32))
    assert i0[0] == 0 and l1[0] == 0 and i0.max() <= 239 and (i1 <= 239).all() and ((i1 == i0 + 1) | (i0 == 239)).all()
    assert np.array_equal(l0, F32(1) - l1) and (twin.axis(1, 2)[4] == 0).all() and (twin.axis(1, 2)[1] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the whole function
@pytest.fixture(scope="module")
def torch64():
    """name -> the reference's expression on the case's inputs, float64, eval mode, CPU: computed once per case."""
    import torch
    from torch import nn
    cache = {}

    def run(name):
        if name not in cache:
            d = twin.reference(name)
            convraw = nn.Sequential(nn.Conv2d(d["C2"] + d["C0"], d["M1"], 3, 1, 1, bias=False), nn.BatchNorm2d(d["M1"]),
                                    nn.LeakyReLU(0.1, True), nn.Conv2d(d["M1"], d["M2"], 1, 1)).double().eval()
            up2storaw = nn.UpsamplingBilinear2d(scale_factor=2)
            t = lambda a: torch.tensor(a).double()                                   # noqa: E731
            with torch.no_grad():
                convraw[0].weight.copy_(t(d["weight1"]))
                for p, k in ((convraw[1].weight, "gamma"), (convraw[1].bias, "beta"), (convraw[1].running_mean, "mean"),
                             (convraw[1].running_var, "var"), (convraw[3].weight, "weight2"), (convraw[3].bias, "bias2")):
                    p.copy_(t(d[k]))
                assert convraw[1].eps == d["eps"]
                fm = up2storaw(t(d["fm"]))
                out = convraw(torch.cat([fm, t(d["x"])], 1)).numpy()
            bn = (d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
            cache[name] = (out,) + twin.forward64(d["fm"], d["x"], d["weight1"], bn, d["weight2"], d["bias2"])
        return cache[name]
    return run


@pytest.mark.parametrize("name", list(twin.CASES))
def test_twin_is_within_the_bound_of_the_references_expression(torch64, name):
    d = twin.reference(name)
    want, out64, bound = torch64(name)
    worst = _within(d["out"], want, bound)
    f = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(d["out"].astype(np.float64) - want)[f]
    print("%s: max |out - torch64| = %.3g, worst err / bound = %.3g (slack %.3g), forward64 against torch64: %.3g of the bound"
          % (name, err.max(), worst, 1 - worst, _within(out64, want, bound)))
    assert d["out"].shape == (d["B"], d["M2"], 2 * d["h"], 2 * d["w"]) and worst <= 1 and err.max() > 0
    assert f.any() and np.isnan(want).any()                                         # the NaN reached some outputs and spared others
    assert _within(out64, want, bound) < 1e-3                                       # the binary64 twin is the reference's function
    for kind, rounded in (("float16", twin.to_f16(d["out"]).astype(np.float64)),
                          ("bfloat16", (twin.to_bf16(d["out"]).astype(np.uint32) << 16).view(F32).astype(np.float64))):
        hb = bound + twin.half_ulp(np.abs(want) + bound, kind)
        keep = np.isfinite(rounded) | ~f                                            # an overflow to Inf is the format's, not an error
        assert _within(np.where(keep, rounded, want), want, hb) <= 1


def test_cases_hold_what_the_gpu_tests_need():
    for name in twin.CASES:
        d = twin.reference(name)
        assert np.isnan(d["fm"]).sum() == 1 and np.isposinf(d["fm"]).sum() == 1 and np.isfinite(d["x"]).all()
        assert d["gamma"][0] == 0 and d["var"][1] == 0 and np.isfinite(d["scale"]).all() and np.isfinite(d["shift"]).all()
        assert d["shift"][0] == 0 and np.signbit(d["shift"][0])
        assert (np.signbit(d["t"]) & (d["t"] == 0)).any(), name                    # a pre-activation that is exactly -0
        out = d["out"]
        assert np.isinf(twin.to_f16(out[np.isfinite(out)])).any() and not np.isinf(out).any()   # float16 overflows, float32 does not
    assert any((c["C2"] + c["C0"]) % 2 for c in twin.CASES.values()) and any(c["M1"] % 2 for c in twin.CASES.values())
    assert any(c["M1"] > 32 and c["M2"] > 32 for c in twin.CASES.values()) and any(c["C0"] == 0 for c in twin.CASES.values())
    r = twin.CASES["reference_channels"]                                            # more than one 8 x 32 tile, partial last ones
    assert 2 * r["h"] > 8 and (2 * r["h"]) % 8 and 2 * r["w"] > 32 and (2 * r["w"]) % 32


def test_half_rounding():
    import torch
    a = np.array([1.0, 1.00390625, 1.01171875, 65504.0, 65520.0, -70000.0, 3.0e38, 3.4e38, np.inf, -0.0, 1e-41], F32)
    assert twin.to_bf16(a)[:5].tolist() == [0x3F80, 0x3F80, 0x3F82, 0x4780, 0x4780]           # ties go to the even pattern
    assert twin.to_bf16(a)[7:10].tolist() == [0x7F80, 0x7F80, 0x8000]                          # overflow to Inf; -0 stays
    rng = np.random.default_rng(11)
    b = np.concatenate([a, (rng.standard_normal(4000) * 10.0 ** rng.integers(-30, 30, 4000)).astype(F32)])
    assert twin.to_bf16(b).tobytes() == torch.tensor(b).bfloat16().view(torch.int16).numpy().tobytes()
    assert twin.to_f16(b).tobytes() == torch.tensor(b).half().numpy().tobytes()
    assert twin.to_f16(a)[3] == 65504 and np.isposinf(twin.to_f16(a)[4]) and np.isneginf(twin.to_f16(a)[5])
    nan = np.array([0x7FC00000, 0xFF800001], np.uint32).view(F32)
    assert twin.to_bf16(nan).tolist() == [0x7FC0, 0xFFC0]


# ------------------------------------------------------------------------------------------------ 3. mutations
MUTATIONS = {
    "align_corners_false": dict(coords="half_pixel"),
    "replicated_ring": dict(ring="edge"),
    "channel_order_x_fm": dict(order="x_fm"),
    "slope_0.01": dict(slope=0.01),
    "eps_omitted": dict(fold=dict(use_eps=False)),
    "shift_from_rounded_scale": dict(fold=dict(from_rounded_scale=True)),
    "bias_after_the_chain": dict(bias_first=False),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_rule_stated_wrongly_leaves_the_bound(torch64, mutation):
    kw = dict(MUTATIONS[mutation])
    fold = kw.pop("fold", {})
    worst = {}
    for name in twin.CASES:
        d = twin.reference(name)
        want, _, bound = torch64(name)
        scale, shift = twin.fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"], **fold)
        out = twin.forward(d["fm"], d["x"], d["weight1"], scale, shift, d["weight2"], d["bias2"], **kw)
        worst[name] = _within(out, want, bound)
    print(mutation, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1
    if mutation == "shift_from_rounded_scale":                                     # the planted channel 2 is what shows it
        assert worst["one_by_one"] <= 1 < min(worst["two_blocks"], worst["no_image"])


def test_zero_ring():
    """All-ones fm, x and weight1: conv1 counts the cells of its window that lie inside the image."""
    C2, C0, h, w = 3, 2, 3, 4
    C = C2 + C0
    one = lambda *s: np.ones(s, F32)                                                # noqa: E731
    _, t = twin.forward(one(1, C2, h, w), one(1, C0, 2 * h, 2 * w), one(1, C, 3, 3), one(1), np.zeros(1, F32), one(1, 1), np.zeros(1, F32), parts=True)
    t = t[0, 0]
    assert t[0, 0] == t[0, -1] == t[-1, 0] == t[-1, -1] == 4 * C
    assert (t[0, 1:-1] == 6 * C).all() and (t[-1, 1:-1] == 6 * C).all() and (t[1:-1, 0] == 6 * C).all() and (t[1:-1, -1] == 6 * C).all()
    assert (t[1:-1, 1:-1] == 9 * C).all()


# ------------------------------------------------------------------------------------------------ 4. the fold and the module
def _bn(d, **kw):
    import torch
    bn = torch.nn.BatchNorm2d(d["M1"], **kw)
    with torch.no_grad():
        for p, k in ((bn.weight, "gamma"), (bn.bias, "beta"), (bn.running_mean, "mean"), (bn.running_var, "var")):
            if p is not None:
                p.copy_(torch.tensor(d[k]))
    return bn


def test_fold_bn_is_the_binary64_expression_and_refuses_what_it_cannot_fold(pkg):
    from clean_pvnet_amd import head
    d = twin.reference("two_blocks")
    scale, shift = head.fold_bn(_bn(d))
    g, b, m, v = (d[k].astype(np.float64) for k in ("gamma", "beta", "mean", "var"))
    s64 = g / np.sqrt(v + 1e-5)
    assert scale.numpy().tobytes() == s64.astype(F32).tobytes() == d["scale"].tobytes()
    assert shift.numpy().tobytes() == (b - m * s64).astype(F32).tobytes() == d["shift"].tobytes()
    assert shift.numpy()[2] != (b - m * s64.astype(F32).astype(np.float64)).astype(F32)[2]       # not from the rounded scale
    with pytest.raises(ValueError, match="affine"):
        head.fold_bn(_bn(d, affine=False))
    with pytest.raises(ValueError, match="running statistics"):
        head.fold_bn(_bn(d, track_running_stats=False))


STATE_KEYS = ["convraw.0.weight", "convraw.1.weight", "convraw.1.bias", "convraw.1.running_mean", "convraw.1.running_var",
              "convraw.1.num_batches_tracked", "convraw.3.weight", "convraw.3.bias"]


def test_state_dict_names_and_round_trip(pkg):
    import torch
    from clean_pvnet_amd import head
    m = head.PVNetHead(ver_dim=18, seg_dim=2)
    sd = m.state_dict()
    assert list(sd) == STATE_KEYS
    assert tuple(sd["convraw.0.weight"].shape) == (32, 35, 3, 3) and tuple(sd["convraw.3.weight"].shape) == (20, 32, 1, 1)
    with torch.no_grad():
        m.convraw[1].running_mean.normal_()
        m.convraw[1].running_var.uniform_(0.5, 2)
    whole = {"resnet18_8s.conv1.weight": torch.zeros(1), **{k: v.clone() for k, v in m.state_dict().items()}}   # a network's checkpoint
    again = head.PVNetHead.from_state_dict(whole)
    assert not again.training and (again.ver_dim, again.seg_dim) == (18, 2)
    assert list(again.state_dict()) == STATE_KEYS
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), m.state_dict().values()))
    small = head.PVNetHead.from_state_dict({"head." + k[len("convraw."):]: v for k, v in head.PVNetHead(4, 3, s2dim=5, raw_dim=7).state_dict().items()},
                                           seg_dim=3, prefix="head.")
    assert (small.ver_dim, small.seg_dim) == (4, 3) and tuple(small.convraw[0].weight.shape) == (7, 8, 3, 3)


def test_the_fold_is_cached_and_follows_the_buffers(pkg):
    import torch
    from clean_pvnet_amd import head
    m = head.PVNetHead(4, 2, s2dim=3, raw_dim=5).eval()
    a = m.folded()
    assert m.folded()[0] is a[0]                                                    # folded once
    with torch.no_grad():
        m.convraw[1].running_var.mul_(4)
    b = m.folded()
    assert b[0] is not a[0] and not torch.equal(b[0], a[0])
    m.load_state_dict(head.PVNetHead(4, 2, s2dim=3, raw_dim=5).state_dict())
    c = m.folded()
    assert c[0] is not b[0] and torch.equal(c[0], head.fold_bn(m.convraw[1])[0])


def test_cpu_tensors_and_training_mode_are_refused(pkg):
    import torch
    from clean_pvnet_amd import head
    fm, x = torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 4, 4)
    w1, s, w2, b2 = torch.zeros(5, 6, 3, 3), torch.zeros(5), torch.zeros(2, 5), torch.zeros(2)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        head.pvnet_head(fm, x, w1, s, s, w2, b2)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        head.upsample2x(fm)
    m = head.PVNetHead(1, 1, s2dim=3, raw_dim=5)
    with pytest.raises(RuntimeError, match="forward only"):                        # a new module is in training mode
        m(fm, x)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"), torch.no_grad():
        m.eval()(fm, x)


def test_requires_grad_and_other_dtypes_are_refused_not_dropped(pkg):
    import torch
    from clean_pvnet_amd import head
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)                      # noqa: E731
    named = [("fm", meta(1, 3, 2, 2)), ("weight1", meta(5, 6, 3, 3, requires_grad=True))]
    real_need = head._native.need_cuda
    head._native.need_cuda = lambda *a: None                                        # the order of the checks: device, dtype, grad
    try:
        with pytest.raises(RuntimeError, match="forward only"):
            head._check(named)
        with torch.no_grad():
            head._check(named)
        head._check([(n, t.detach()) for n, t in named])
        with pytest.raises(RuntimeError, match="float32"):
            head._check([("fm", meta(1, 3, 2, 2, dtype=torch.float16))])
        with pytest.raises(RuntimeError, match="float32"):
            head.upsample2x(meta(1, 3, 2, 2, dtype=torch.bfloat16))
        m = head.PVNetHead(1, 1, s2dim=3, raw_dim=5).eval().to("meta")             # its parameters require grad
        with pytest.raises(RuntimeError, match="forward only"):
            m(meta(1, 3, 2, 2), meta(1, 3, 4, 4))
        with pytest.raises(RuntimeError, match="out_dtype"), torch.no_grad():
            head.pvnet_head(meta(1, 3, 2, 2), meta(1, 3, 4, 4), meta(5, 6, 3, 3), meta(5), meta(5), meta(2, 5), meta(2), out_dtype=torch.float64)
    finally:
        head._native.need_cuda = real_need
