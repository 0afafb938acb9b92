"""PVNet's output head on the MI355X (clean_pvnet_amd.head): every output equals the numpy twin (tests/head_twin.py, itself held to
the reference's expression in float64 in tests/test_head.py) bit for bit with -0 as +0, on a side stream as on the default
stream; the upsample alone does too, and lies within twice the twin's bound of torch's own device kernel; the half-precision
outputs are the float32 ones rounded; views are read by their strides; the module feeds ``decode_keypoint`` without a copy."""
import numpy as np
import pytest

from tests import head_twin as twin
from tests.test_gpu_dcn import on_both_streams

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("fm", "x", "weight1", "scale", "shift", "weight2", "bias2")


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in KEYS}


def _head(t, **kw):
    from clean_pvnet_amd.head import pvnet_head
    return pvnet_head(*(t[k] for k in KEYS), **kw)


def _report(name, got, want):
    diff = twin.canon(got) != twin.canon(want)
    if diff.any():
        w = np.argwhere(diff)
        with np.errstate(invalid="ignore"):
            print("%s: %d of %d outputs differ; first at %s: device %r, twin %r; max |diff| = %.3g"
                  % (name, diff.sum(), diff.size, tuple(w[0]), got[tuple(w[0])], want[tuple(w[0])], np.nanmax(np.abs(got - want))))
    return not diff.any()


# ------------------------------------------------------------------------------------------------------------ 1. the output
@pytest.mark.parametrize("name", list(twin.CASES))
def test_forward_equals_the_twin_bit_for_bit(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: _head(t))
    assert got.shape == d["out"].shape and got.dtype == F32
    assert _report(name, got, d["out"])
    assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("name", list(twin.CASES))
def test_half_outputs_are_the_float32_result_rounded(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    full = _head(t).cpu().numpy()
    f16 = _head(t, out_dtype=torch.float16)
    bf16 = _head(t, out_dtype=torch.bfloat16)
    assert f16.dtype == torch.float16 and bf16.dtype == torch.bfloat16 and f16.shape == bf16.shape == tuple(full.shape)
    f16 = f16.cpu().numpy()
    assert f16.tobytes() == twin.to_f16(full).tobytes()
    assert bf16.view(torch.int16).cpu().numpy().tobytes() == twin.to_bf16(full).tobytes()
    assert np.isinf(f16).any() and not np.isinf(full).any()                        # the overflow to Inf is there


# ------------------------------------------------------------------------------------------------------------ 2. the upsample
@pytest.mark.parametrize("name", list(twin.CASES))
def test_upsample_equals_the_twin_bit_for_bit(pkg, gpu, name):
    from clean_pvnet_amd.head import upsample2x
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: upsample2x(t["fm"]))
    assert _report(name, got, d["u"])


@pytest.mark.parametrize("name", list(twin.CASES))
def test_upsample_is_within_twice_the_bound_of_torchs_device_kernel(pkg, gpu, name):
    """Both are float32 evaluations of one function, each within the twin's bound of the exact one.  What the reference network
    computes on this card is torch's kernel; bit parity with it is not claimed (it is free to contract), the share is printed."""
    import torch
    from clean_pvnet_amd.head import upsample2x
    d, t = _device_case(gpu, name)
    ours = upsample2x(t["fm"]).cpu().numpy()
    theirs = torch.nn.UpsamplingBilinear2d(scale_factor=2)(t["fm"]).cpu().numpy()
    _, bound = twin.upsample64(d["fm"])
    assert np.array_equal(np.isnan(ours), np.isnan(theirs))
    f = np.isfinite(theirs)
    err = np.abs(ours[f].astype(np.float64) - theirs[f].astype(np.float64))
    print("%s: %.1f%% of the finite outputs have torch's bits; max |ours - torch| = %.3g, worst err / (2 bound) = %.3g"
          % (name, 100 * (twin.canon(ours)[f] == twin.canon(theirs)[f]).mean(), err.max(), (err / np.maximum(2 * bound[f], 1e-300)).max()))
    assert np.isfinite(ours[f]).all() and (err <= 2 * bound[f]).all()


def test_upsample_refuses_more_than_2_28_elements(pkg, gpu):
    import torch
    from clean_pvnet_amd.head import upsample2x
    fm = torch.zeros(1, 1, 1, 1, device=gpu).expand(1, 64, 1100, 1100)            # 64 * 4 * 1210000 > 2^28; no memory behind it
    with pytest.raises(ValueError, match="2\\^28"):
        upsample2x(fm)


# ------------------------------------------------------------------------------------------------------------ 3. views and the module
@pytest.mark.parametrize("name", ["one_by_one", "reference_channels", "no_image"])
def test_channel_slices_give_the_bytes_of_contiguous_copies(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    B, C2, C0 = d["B"], d["C2"], d["C0"]
    wide_fm = torch.full((B + 1, C2 + 5, d["h"], d["w"]), float("nan"), device=gpu)
    wide_x = torch.full((B + 1, C0 + 4, 2 * d["h"], 2 * d["w"]), float("nan"), device=gpu)
    wide_fm[:B, 2:2 + C2], wide_x[:B, 1:1 + C0] = t["fm"], t["x"]
    fm, x = wide_fm[:B, 2:2 + C2], wide_x[:B, 1:1 + C0]
    assert fm.stride(0) > C2 * d["h"] * d["w"] and fm.data_ptr() != wide_fm.data_ptr() and (B == 1 or not fm.is_contiguous())
    got = _head({**t, "fm": fm, "x": x}).cpu().numpy()
    want = _head(t).cpu().numpy()
    assert got.tobytes() == want.tobytes() and _report(name, got, d["out"])


def _module(gpu, d):
    import torch
    from clean_pvnet_amd.head import PVNetHead
    m = PVNetHead(d["M2"] - 1, 1, s2dim=d["C2"], raw_dim=d["M1"], image_dim=d["C0"]).to(gpu).eval().requires_grad_(False)
    with torch.no_grad():
        m.convraw[0].weight.copy_(_t(gpu, d["weight1"]))
        for p, k in ((m.convraw[1].weight, "gamma"), (m.convraw[1].bias, "beta"), (m.convraw[1].running_mean, "mean"),
                     (m.convraw[1].running_var, "var"), (m.convraw[3].weight, "weight2"), (m.convraw[3].bias, "bias2")):
            p.copy_(_t(gpu, d[k]))
    return m


@pytest.mark.parametrize("name", ["two_blocks", "reference_channels"])
def test_module_equals_the_function_on_its_folded_parameters(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    m = _module(gpu, d)
    out = m(t["fm"], t["x"])
    assert set(out) == {"seg", "vertex"} and out["seg"].shape[1] == 1 and out["vertex"].shape[1] == d["M2"] - 1
    assert out["seg"].untyped_storage().data_ptr() == out["vertex"].untyped_storage().data_ptr()     # views of one tensor
    scale, shift = m.folded()
    assert scale.cpu().numpy().tobytes() == d["scale"].tobytes() and shift.cpu().numpy().tobytes() == d["shift"].tobytes()
    got = torch.cat([out["seg"], out["vertex"]], 1).cpu().numpy()
    assert got.tobytes() == _head(t).cpu().numpy().tobytes() and _report(name, got, d["out"])
    with torch.no_grad():
        m.convraw[1].running_mean.add_(1)                                           # the fold follows the buffers
    assert not np.array_equal(m.folded()[1].cpu().numpy(), d["shift"])
    with pytest.raises(RuntimeError, match="forward only"):
        m.train()(t["fm"], t["x"])
    with pytest.raises(RuntimeError, match="forward only"):
        m.eval().requires_grad_(True)(t["fm"], t["x"])


def test_module_output_feeds_decode_keypoint_without_a_copy(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.head import PVNetHead
    g = torch.Generator(device="cpu").manual_seed(7)
    m = PVNetHead(ver_dim=8, seg_dim=2, s2dim=6, raw_dim=8).eval().requires_grad_(False)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    m = m.to(gpu)
    fm, x = torch.randn(2, 6, 24, 32, generator=g).to(gpu), torch.randn(2, 3, 48, 64, generator=g).to(gpu)
    out = m(fm, x)
    assert not out["vertex"].is_contiguous() and bool(torch.isfinite(out["vertex"]).all())
    assert 0.05 < float((out["seg"][:, 1] > out["seg"][:, 0]).float().mean()) < 0.95              # a mask with both classes
    views = decode_keypoint(dict(out), seed=5)
    copies = decode_keypoint({"seg": out["seg"].float().contiguous(), "vertex": out["vertex"].float().contiguous()}, seed=5)
    for k in ("mask", "kpt_2d"):
        assert views[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    assert tuple(views["kpt_2d"].shape) == (2, 4, 2) and tuple(views["mask"].shape) == (2, 48, 64)


def test_an_empty_batch_gives_an_empty_tensor(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "odd_k")
    out = _head({**t, "fm": t["fm"][:0], "x": t["x"][:0]}, out_dtype=torch.bfloat16)
    assert tuple(out.shape) == (0, d["M2"], 2 * d["h"], 2 * d["w"]) and out.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ 4. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    from clean_pvnet_amd.head import upsample2x
    cases = [_device_case(gpu, name) for name in twin.CASES]
    m = _module(gpu, cases[2][0])
    m.folded()
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            runs.append([_head(t) for d, t in cases] + [_head(cases[1][1], out_dtype=torch.float16).view(torch.int16),
                                                        upsample2x(cases[1][1]["fm"]), m(cases[2][1]["fm"], cases[2][1]["x"])["vertex"]])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for (d, _), a in zip(cases, runs[0]):
        assert twin.same_bits(a.cpu().numpy(), d["out"])
