"""DCNv2 modulated deformable convolution on the MI355X (clean_pvnet_amd.dcn): every output equals the numpy twin
(tests/dcn_twin.py, itself held to torch's ``unfold`` / ``conv2d`` and to binary64 in tests/test_dcn.py) bit for bit with -0 as
+0, on a side stream as on the default stream; the columns alone do too; the modules pass their strided views correctly and the
extension surface the reference's own module calls gives the same bits."""
import numpy as np
import pytest

from tests import dcn_twin as twin

pytestmark = pytest.mark.gpu


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in ("input", "offset", "mask", "weight", "bias")}


def _conv(t, d, bias=True):
    from clean_pvnet_amd.dcn import dcn_v2_conv
    return dcn_v2_conv(t["input"], t["offset"], t["mask"], t["weight"], t["bias"] if bias else None, d["stride"], d["padding"],
                       d["dilation"], d["dg"])


def on_both_streams(f):
    """f() on a side stream and on the default stream: the two results are the same bits; returns them as numpy."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = f()
    side.synchronize()
    a, b = a.cpu().numpy(), f().cpu().numpy()
    assert a.tobytes() == b.tobytes(), "the side stream's result differs from the default stream's"
    return a


def _report(name, got, want):
    diff = twin.canon(got) != twin.canon(want)
    if diff.any():
        w = np.argwhere(diff)
        print("%s: %d of %d outputs differ; first at %s: device %r, twin %r; max |diff| = %.3g"
              % (name, diff.sum(), diff.size, tuple(w[0]), got[tuple(w[0])], want[tuple(w[0])], np.nanmax(np.abs(got - want))))
    return not diff.any()


# ------------------------------------------------------------------------------------------------------------ 1. the output
@pytest.mark.parametrize("name", list(twin.CASES))
def test_forward_equals_the_twin_bit_for_bit(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: _conv(t, d))
    assert got.shape == d["out"].shape and np.isfinite(got).all()
    assert _report(name, got, d["out"])


def test_no_bias_is_a_bias_of_zeros(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "two_groups_m33")
    got = _conv(t, d, bias=False).cpu().numpy()
    want = _conv({**t, "bias": torch.zeros_like(t["bias"])}, d).cpu().numpy()
    assert twin.same_bits(got, want) and not twin.same_bits(got, d["out"])


# ------------------------------------------------------------------------------------------------------------ 2. the columns
@pytest.mark.parametrize("name", twin.COLUMN_CASES)
def test_columns_equal_the_twin_bit_for_bit(pkg, gpu, name):
    from clean_pvnet_amd.dcn import columns
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: columns(t["input"], t["offset"], t["mask"], d["kernel"], d["stride"], d["padding"], d["dilation"],
                                          d["dg"]))
    assert np.isfinite(got).all()                                                   # the NaN offset gave a zero, not a NaN
    assert _report(name, got, d["col"])
    for b, g, tap, y, x, axis, target in d["planted"]:                              # the planted samples that lie outside: zero columns
        if not np.isfinite(target) or target in (-1.0, float(d["H"] if axis == "h" else d["W"])) or abs(target) > 1e6:
            KK, Cg = d["kernel"][0] * d["kernel"][1], d["C"] // d["dg"]
            rows = [(g * Cg + c) * KK + tap for c in range(Cg)]
            assert not got[b, rows, y * d["Wo"] + x].any()


def test_columns_refuse_more_than_2_28_elements(pkg, gpu):
    import torch
    from clean_pvnet_amd.dcn import columns
    x = torch.zeros(1, 1, 1, 1, device=gpu).expand(1, 64, 700, 700)                 # 64 * 9 * 490000 > 2^28; no memory behind it
    off, msk = torch.zeros(1, 1, 1, 1, device=gpu).expand(1, 18, 700, 700), torch.zeros(1, 1, 1, 1, device=gpu).expand(1, 9, 700, 700)
    with pytest.raises(ValueError, match="2\\^28"):
        columns(x, off, msk, (3, 3), 1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------ 3. the modules
def _module(gpu, name="odd_k_small_m", zero_offsets=False):
    import torch
    from clean_pvnet_amd.dcn import DCN
    d = twin.reference(name)
    # dilation 1 whatever the case's: the offset convolution takes none, as in the reference, and the two sizes must agree
    m = DCN(d["C"], d["M"], d["kernel"], d["stride"], d["padding"], 1, d["dg"]).to(gpu).requires_grad_(False)
    with torch.no_grad():
        m.weight.copy_(_t(gpu, d["weight"]))
        m.bias.copy_(_t(gpu, d["bias"]))
        if not zero_offsets:
            g = torch.Generator(device="cpu").manual_seed(3)
            m.conv_offset_mask.weight.copy_(torch.randn(m.conv_offset_mask.weight.shape, generator=g) * 0.3)
            m.conv_offset_mask.bias.copy_(torch.randn(m.conv_offset_mask.bias.shape, generator=g))
    return d, m, _t(gpu, d["input"])


@pytest.mark.parametrize("name", ["odd_k_small_m", "uncached_odd_group"])
def test_dcn_module_passes_views_that_equal_the_copies(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.dcn import dcn_v2_conv
    from lib.csrc.dcn_v2 import _ext
    d, m, x = _module(gpu, name)
    got = m(x)
    out = m.conv_offset_mask(x)
    o1, o2, mask = torch.chunk(out, 3, dim=1)
    offset, mask = torch.cat((o1, o2), dim=1).contiguous(), torch.sigmoid(mask).contiguous()
    assert float(offset.abs().max()) > 1                                            # real offsets
    want = dcn_v2_conv(x, offset, mask, m.weight, m.bias, m.stride, m.padding, m.dilation, m.deformable_groups)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # the call the reference's own DCN.forward makes (dcn_v2.py:25-31, 119-128), built by hand
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = m.kernel_size, m.stride, m.padding, m.dilation
    theirs = _ext.dcn_v2_forward(x, m.weight, m.bias, offset, mask, kh, kw, sh, sw, ph, pw, dh, dw, m.deformable_groups)
    assert theirs.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    # and the twin on the same offsets
    tw = twin.forward(d["input"], offset.cpu().numpy(), mask.cpu().numpy(), d["weight"], d["bias"], m.stride, m.padding, m.dilation, d["dg"])
    assert _report(name, got.cpu().numpy(), tw)


def test_dcn_module_at_its_initial_offsets_is_half_a_convolution(pkg, gpu):
    import torch
    import torch.nn.functional as F
    d, m, x = _module(gpu, "odd_k_small_m", zero_offsets=True)
    got = m(x).cpu().numpy().astype(np.float64)
    xd, wd = torch.from_numpy(d["input"]).double(), torch.from_numpy(d["weight"]).double()
    conv = F.conv2d(xd, wd, None, d["stride"], d["padding"], 1).numpy()
    want = 0.5 * conv + d["bias"].astype(np.float64)[None, :, None, None]           # sigmoid(0) = 0.5 exactly
    colabs = F.unfold(xd.abs(), d["kernel"], 1, d["padding"], d["stride"]).numpy() * 0.5
    bound = twin.gemm_bound(d["weight"], d["bias"], colabs).reshape(want.shape)
    err = np.abs(got - want)
    print("max err %.3g, max bound %.3g" % (err.max(), bound.max()))
    assert (err <= bound).all()


def test_grad_is_refused_on_the_device(pkg, gpu):
    import torch
    from clean_pvnet_amd.dcn import DCN
    m = DCN(2, 3, (3, 3), 1, 1).to(gpu)
    x = torch.zeros(1, 2, 5, 5, device=gpu)
    with pytest.raises(RuntimeError, match="forward only"):
        m(x)
    with torch.no_grad():
        assert tuple(m(x).shape) == (1, 3, 5, 5)
    from clean_pvnet_amd.dcn import dcn_v2_conv
    off, msk = torch.zeros(1, 18, 5, 5, device=gpu), torch.ones(1, 9, 5, 5, device=gpu)
    with pytest.raises(RuntimeError, match="float32"):                             # no half-precision path, and no silent cast
        dcn_v2_conv(x.half(), off, msk, m.weight.detach(), None, 1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------ 4. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    from clean_pvnet_amd.dcn import columns
    cases = [_device_case(gpu, name) for name in twin.ISSUE_CASES]
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            runs.append([_conv(t, d) for d, t in cases])
        d, t = cases[0]
        col = columns(t["input"], t["offset"], t["mask"], d["kernel"], d["stride"], d["padding"], d["dilation"], d["dg"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(col.shape) == d["col"].shape
    for (d, _), a, b in zip(cases, *runs):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a.tobytes() == b.tobytes() and twin.same_bits(a, d["out"])
