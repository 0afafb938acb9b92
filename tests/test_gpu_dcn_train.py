"""The DCNv2 backward pass on the MI355X (clean_pvnet_amd.dcn_train): all five gradients equal the numpy twin
(tests/dcn_train_twin.py, itself held to a binary64 autograd evaluation in tests/test_dcn_train.py) bit for bit with -0 as +0,
through the functional entry and through autograd; reruns, chunked batches, views and subsets of the gradients give the same
bytes; the ``DCN`` module trains end to end within the derived bound; a non-finite upstream gradient poisons its own image
only; and ``dcn`` still refuses."""
import numpy as np
import pytest

from tests import dcn_train_twin as twin
from tests import dcn_twin

pytestmark = pytest.mark.gpu
NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
KEYS = ("input", "offset", "mask", "weight", "bias", "gout")


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in KEYS}


def _geo(d):
    return d["stride"], d["padding"], d["dilation"], d["dg"]


def _backward(t, d, **kw):
    from clean_pvnet_amd.dcn_train import dcn_v2_backward
    return dcn_v2_backward(t["input"], t["offset"], t["mask"], t["weight"], t["bias"], t["gout"], *_geo(d), **kw)


def _np(grads):
    return [None if g is None else g.cpu().numpy() for g in grads]


def _autograd(t, d, requires=(True,) * 5):
    """The five ``.grad`` of the leaves after ``dcn_v2_conv(...).backward(gout)``, and the output."""
    from clean_pvnet_amd.dcn_train import dcn_v2_conv
    leaves = [t[k].clone().requires_grad_(r) for k, r in zip(KEYS[:5], requires)]
    out = dcn_v2_conv(*leaves, *_geo(d))
    out.backward(t["gout"])
    return [leaf.grad for leaf in leaves], out.detach()


def _report(what, got, want):
    diff = dcn_twin.canon(got) != dcn_twin.canon(want)
    if diff.any():
        w = np.argwhere(diff)
        print("%s: %d of %d differ; first at %s: device %r, twin %r; max |diff| = %.3g"
              % (what, diff.sum(), diff.size, tuple(w[0]), got[tuple(w[0])], want[tuple(w[0])], np.nanmax(np.abs(got - want))))
    return not diff.any()


# ------------------------------------------------------------------------------------------------ 5. the device against the twin
@pytest.mark.parametrize("name", list(dcn_twin.CASES))
def test_backward_equals_the_twin_bit_for_bit(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = _np(_backward(t, d))
    ok = [_report("%s %s" % (name, what), g, w) for what, g, w in zip(NAMES, got, d["grads"])]
    assert all(ok), dict(zip(NAMES, ok))
    assert got[3].tobytes() == d["grads"][3].tobytes() and got[4].tobytes() == d["grads"][4].tobytes()    # (not even a zero's sign)
    through, _ = _autograd(t, d)
    for what, a, b in zip(NAMES, _np(through), got):
        assert a.tobytes() == b.tobytes(), what
    KK = d["kernel"][0] * d["kernel"][1]
    goff = got[1].reshape(d["B"], d["dg"], KK, 2, d["Ho"], d["Wo"])
    gmask = got[2].reshape(d["B"], d["dg"], KK, d["Ho"], d["Wo"])
    for b, g, tap, y, x, axis, target in d["planted"]:                              # outside the window, a NaN offset too: exactly +0
        if not np.isfinite(target) or target in (-1.0, float(d["H"] if axis == "h" else d["W"])) or abs(target) > 1e6:
            assert not goff[b, g, tap, :, y, x].view(np.uint32).any() and not gmask[b, g, tap, y, x].view(np.uint32)
    assert all(np.isfinite(g).all() for g in got)


# ------------------------------------------------------------------------------------------------ 6. reruns, no host sync
def test_two_runs_give_identical_bytes_and_nothing_synchronises(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "k_chunks_pixel_tiles")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first, second = _backward(t, d), _backward(t, d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for what, a, b in zip(NAMES, _np(first), _np(second)):
        assert a.tobytes() == b.tobytes(), what


# ------------------------------------------------------------------------------------------------ 7. the forward's bytes
@pytest.mark.parametrize("name", ["odd_k_small_m", "two_groups_m33"])
def test_forward_bytes_equal_dcn(pkg, gpu, name):
    import torch
    from clean_pvnet_amd import dcn, dcn_train
    d, t = _device_case(gpu, name)
    args = [t[k] for k in KEYS[:5]]
    with torch.no_grad():
        want = dcn.dcn_v2_conv(*args, *_geo(d))
        plain = dcn_train.dcn_v2_conv(*args, *_geo(d))
    _, tracked = _autograd(t, d)
    assert plain.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() == tracked.cpu().numpy().tobytes()
    assert dcn_twin.same_bits(want.cpu().numpy(), d["out"])


# ------------------------------------------------------------------------------------------------ 8. subsets of the gradients
@pytest.mark.parametrize("requires", [(False, False, False, True, True), (True, False, False, False, False)],
                         ids=["weight_and_bias", "input"])
def test_needs_input_grad_subsets(pkg, gpu, requires):
    d, t = _device_case(gpu, "odd_k_small_m")
    full = _np(_autograd(t, d)[0])
    got = _autograd(t, d, requires)[0]
    functional = _backward(t, d, need=requires)
    for what, r, g, f, w in zip(NAMES, requires, got, functional, full):
        if r:
            assert g.cpu().numpy().tobytes() == f.cpu().numpy().tobytes() == w.tobytes(), what
        else:
            assert g is None and f is None, what


# ------------------------------------------------------------------------------------------------ 9. views
def test_channel_slices_of_one_tensor_equal_the_copies(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "uncached_odd_group")
    taps = d["dg"] * d["kernel"][0] * d["kernel"][1]
    both = torch.cat([t["offset"], t["mask"]], dim=1)
    views = dict(t, offset=both[:, :2 * taps], mask=both[:, 2 * taps:])
    assert not views["mask"].is_contiguous() and views["offset"].data_ptr() == both.data_ptr()
    want = _np(_backward(t, d))
    for what, a, b in zip(NAMES, _np(_backward(views, d)), want):
        assert a.tobytes() == b.tobytes(), what
    strided = dict(views, gout=t["gout"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))      # grad_output: made contiguous
    assert not strided["gout"].is_contiguous()
    for what, a, b in zip(NAMES, _np(_backward(strided, d)), want):
        assert a.tobytes() == b.tobytes(), what


# ------------------------------------------------------------------------------------------------ 10. chunks
def test_chunks_of_two_images_equal_one_chunk(pkg, gpu):
    c = dict(dcn_twin.CASES["odd_k_small_m"], B=5)
    rng = np.random.default_rng(5)
    Ho, Wo = dcn_twin.out_size(c["H"], c["W"], c["kernel"], c["stride"], c["padding"], c["dilation"])
    t = dict(input=rng.standard_normal((5, c["C"], c["H"], c["W"])), offset=2 * rng.standard_normal((5, 18, Ho, Wo)),
             mask=rng.random((5, 9, Ho, Wo)), weight=rng.standard_normal((c["M"], c["C"], 3, 3)), bias=rng.standard_normal(c["M"]),
             gout=rng.standard_normal((5, c["M"], Ho, Wo)) * 10.0 ** rng.integers(-3, 4, (5, 1, 1, 1)))
    host = {k: v.astype(np.float32) for k, v in t.items()}
    t = {k: _t(gpu, v) for k, v in host.items()}
    whole = _np(_backward(t, c))
    for chunk in (2, 1):
        for what, a, b in zip(NAMES, _np(_backward(t, c, _chunk_images=chunk)), whole):
            assert a.tobytes() == b.tobytes(), (what, chunk)
    want = twin.backward(host["input"], host["offset"], host["mask"], host["weight"], host["gout"], *_geo(c))
    assert all(_report("B=5 %s" % what, g, w) for what, g, w in zip(NAMES, whole, want))


def test_a_footprint_too_large_for_lds_takes_the_plain_scatter(pkg, gpu):
    """Dilation 40: the tile's footprint does not fit the scatter's LDS windows, so every addition goes to memory -- the same
    integers, the same bytes as the twin."""
    c = dict(C=2, M=3, H=20, W=20, kernel=(3, 3), stride=1, padding=40, dilation=40, dg=1)
    rng = np.random.default_rng(9)
    Ho, Wo = dcn_twin.out_size(c["H"], c["W"], c["kernel"], c["stride"], c["padding"], c["dilation"])
    assert (Ho, Wo) == (20, 20)
    host = dict(input=rng.standard_normal((2, 2, 20, 20)), offset=6 * rng.standard_normal((2, 18, Ho, Wo)), mask=rng.random((2, 9, Ho, Wo)),
                weight=rng.standard_normal((3, 2, 3, 3)), bias=rng.standard_normal(3), gout=rng.standard_normal((2, 3, Ho, Wo)))
    host = {k: v.astype(np.float32) for k, v in host.items()}
    got = _np(_backward({k: _t(gpu, v) for k, v in host.items()}, c))
    want = twin.backward(host["input"], host["offset"], host["mask"], host["weight"], host["gout"], *_geo(c))
    assert np.count_nonzero(want[0]) > 400
    assert all(_report("dilation 40 %s" % what, g, w) for what, g, w in zip(NAMES, got, want))


# ------------------------------------------------------------------------------------------------ 11. the module, end to end
def test_dcn_module_trains_within_the_bound_of_binary64(pkg, gpu):
    """``DCN(4, 6, 3, 1, 1)`` with a non-zero ``conv_offset_mask``, ``out.square().sum().backward()``, against the same module
    graph on the CPU in binary64 (``dcn64``), evaluated at the device's float32 intermediates (the offset convolution's output,
    the sigmoid, the DCN's output: each binary64 value is moved onto the float32 one by a constant, so the comparison is of
    the backward passes).  Bounds: ``weight`` and ``bias`` the twin's derived bounds as they are.  The gradient reaching the
    offset convolution's output is grad_offset (its bound) and grad_mask * sigmoid' (grad_mask's bound * sigmoid' + 8u |grad_mask|:
    the float32 sigmoid is within 4u of the binary64 one, the backward's three operations within 3u); a convolution gradient
    of n terms summed in any order in float32 is within gamma_n * sum |terms| (n = B*P for conv_offset_mask.weight and .bias,
    n = 27 * 9 for the input) plus the same sum of the incoming bound; the input adds the twin's grad_input bound and one
    rounding for the sum of the two paths."""
    import torch
    import torch.nn.functional as F
    from clean_pvnet_amd.dcn_train import DCN
    g = torch.Generator(device="cpu").manual_seed(17)
    m = DCN(4, 6, 3, 1, 1)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / 6)
        m.bias.copy_(torch.randn(m.bias.shape, generator=g))
        m.conv_offset_mask.weight.copy_(torch.randn(m.conv_offset_mask.weight.shape, generator=g) * 0.3)
        m.conv_offset_mask.bias.copy_(torch.randn(m.conv_offset_mask.bias.shape, generator=g))
    x_host = torch.randn(2, 4, 9, 11, generator=g)
    host = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(gpu)
    x = x_host.to(gpu).requires_grad_(True)
    out = m(x)
    out.square().sum().backward()
    with torch.no_grad():
        z32 = m.conv_offset_mask(x)
        mask32 = torch.sigmoid(z32[:, 18:])
    assert float(z32[:, :18].abs().max()) > 1                                       # real offsets
    got = {"input": x.grad, **{k: p.grad for k, p in m.named_parameters()}}
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}

    leaf = {k: v.double().requires_grad_(True) for k, v in host.items()}
    x64 = x_host.double().requires_grad_(True)
    pin = lambda v64, v32: v64 + (v32.detach().cpu().double() - v64).detach()       # noqa: E731
    z = pin(F.conv2d(x64, leaf["conv_offset_mask.weight"], leaf["conv_offset_mask.bias"], padding=1), z32)
    z.retain_grad()
    mask = pin(torch.sigmoid(z[:, 18:]), mask32)
    o = pin(twin.dcn64(x64, z[:, :18], mask, leaf["weight"], leaf["bias"], 1, 1, 1, 1), out)
    o.square().sum().backward()
    want = {"input": x64.grad.numpy(), **{k: v.grad.numpy() for k, v in leaf.items()}}

    go32 = (2 * out.detach()).cpu().numpy()
    b_in, b_off, b_mask, b_w, b_b = twin.bounds(x_host.numpy(), z32[:, :18].cpu().numpy(), mask32.cpu().numpy(), host["weight"].numpy(),
                                                go32, 1, 1, 1, 1)
    u = dcn_twin.U
    s64 = torch.sigmoid(z32[:, 18:].cpu().double()).numpy()
    gm64 = np.abs(z.grad[:, 18:].numpy()) / np.maximum(s64 * (1 - s64), 1e-300)     # |grad_mask| of the binary64 graph
    bz = torch.from_numpy(np.concatenate([b_off, b_mask * s64 * (1 - s64) + 8 * u * gm64], axis=1))
    az = z.grad.abs()
    ax, aw = x_host.double().abs(), host["conv_offset_mask.weight"].double().abs()
    n_par, n_in = 2 * 9 * 11, 27 * 9
    bound = {
        "weight": b_w, "bias": b_b,
        "conv_offset_mask.weight": (torch.nn.grad.conv2d_weight(ax, aw.shape, bz, padding=1)
                                    + twin.gamma(n_par + 1) * torch.nn.grad.conv2d_weight(ax, aw.shape, az, padding=1)).numpy(),
        "conv_offset_mask.bias": (bz.sum(dim=(0, 2, 3)) + twin.gamma(n_par + 1) * az.sum(dim=(0, 2, 3))).numpy(),
    }
    conv_in = torch.nn.grad.conv2d_input(ax.shape, aw, bz, padding=1) + twin.gamma(n_in + 1) * torch.nn.grad.conv2d_input(ax.shape, aw, az, padding=1)
    bound["input"] = b_in + conv_in.numpy() + 2 * u * (np.abs(want["input"]) + b_in + conv_in.numpy())
    for k in ("input", "weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"):
        err = np.abs(got[k] - want[k])
        print("%s: max err %.3g, max bound %.3g, worst err / bound %.3g" % (k, err.max(), bound[k].max(), (err / np.maximum(bound[k], 1e-300)).max()))
    for k in bound:
        assert np.isfinite(got[k]).all() and (np.abs(got[k] - want[k]) <= bound[k]).all(), k
        assert np.abs(got[k] - want[k]).max() > 0, k


# ------------------------------------------------------------------------------------------------ 12. a non-finite upstream gradient
def test_an_inf_upstream_poisons_its_own_image_only(pkg, gpu):
    d, t = _device_case(gpu, "odd_k_small_m")
    clean = _np(_backward(t, d))
    gout = t["gout"].clone()
    gout[0, 2, 3, 4] = float("inf")
    got = _np(_backward(dict(t, gout=gout), d))
    assert np.isnan(got[0][0]).all()                                                # image 0: all NaN, so that a gradient scaler sees it
    for i in range(3):                                                              # image 1: input, offset and mask gradients as before
        assert got[i][1].tobytes() == clean[i][1].tobytes(), NAMES[i]
    assert np.isfinite(got[0][1]).all() and not np.isfinite(got[3]).all() and not np.isfinite(got[4]).all()
    again = _np(_backward(t, d))                                                    # and nothing faulted: the next call is as clean as the first
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, clean))


# ------------------------------------------------------------------------------------------------ 13. dcn still refuses
def test_dcn_still_refuses_a_tensor_that_requires_grad(pkg, gpu):
    import torch
    from clean_pvnet_amd import dcn
    from lib.csrc.dcn_v2 import _ext
    d, t = _device_case(gpu, "odd_k_small_m")
    with pytest.raises(RuntimeError, match="forward only"):
        dcn.dcn_v2_conv(t["input"], t["offset"], t["mask"], t["weight"].clone().requires_grad_(True), t["bias"], *_geo(d))
    with pytest.raises(RuntimeError, match="forward only"):
        dcn.DCN(3, 5, 3, 1, 1).to(gpu)(t["input"])
    with pytest.raises(NotImplementedError, match="forward pass"):
        _ext.dcn_v2_backward(None, None)
    with torch.no_grad():
        assert tuple(dcn.DCN(3, 5, 3, 1, 1).to(gpu)(t["input"]).shape) == (2, 5, 7, 9)
