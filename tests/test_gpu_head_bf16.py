"""The bfloat16 compute mode of PVNet's output head on the MI355X (``pvnet_head(..., compute="bfloat16")``): every output lies within the
twin's ``bound_acc`` of its ``out64`` (tests/head_bf16_twin.py) and has its non-finite sets, on a side stream as on the default
stream; the exact-sum cases agree bit for bit in ``bfloat16`` mode; the half-precision outputs are the float32 ones rounded; views
are read by their strides; the module keeps the mode and feeds ``decode_keypoint`` without a copy; the limits and refusals are the
float32 mode's."""
import numpy as np
import pytest

from tests import head_bf16_twin as twin
from tests.test_gpu_dcn import on_both_streams

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = twin.KEYS
ALL = list(twin.CASES) + list(twin.EXACT_CASES)


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in KEYS}


def _head(d, t, mode, **kw):
    from clean_pvnet_amd.head import pvnet_head
    return pvnet_head(*(t[k] for k in KEYS), negative_slope=d["slope"], compute=mode, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. the output
@pytest.mark.parametrize("mode", twin.DEVICE_MODES)
@pytest.mark.parametrize("name", ALL)
def test_forward_lies_within_bound_acc_of_the_twin(pkg, gpu, name, mode):
    d, t = _device_case(gpu, name)
    ref = d[mode]
    got = on_both_streams(lambda: _head(d, t, mode))
    assert got.shape == ref["out64"].shape and got.dtype == F32
    f = np.isfinite(ref["out64"])
    bits = np.mean(twin.canon(got)[f] == twin.canon(ref["out64"].astype(F32))[f])
    print("%s %s: worst |device - out64| / bound_acc = %.3g; %.1f%% of the finite outputs have out64's float32 bits"
          % (name, mode, twin.worst(got, ref), 100 * bits))
    assert twin.within(got, ref, mode)
    if name in twin.EXACT_CASES:
        if mode == "bfloat16":
            assert twin.same_bits(got, ref["out64"].astype(F32))
    else:
        assert not f.all() and f.any()                                              # the planted NaN and Inf are there


@pytest.mark.parametrize("mode", twin.DEVICE_MODES)
@pytest.mark.parametrize("name", list(twin.CASES))
def test_half_outputs_are_the_float32_result_rounded(pkg, gpu, name, mode):
    import torch
    d, t = _device_case(gpu, name)
    full = _head(d, t, mode).cpu().numpy()
    f16 = _head(d, t, mode, out_dtype=torch.float16)
    bf16 = _head(d, t, mode, out_dtype=torch.bfloat16)
    assert f16.dtype == torch.float16 and bf16.dtype == torch.bfloat16 and f16.shape == bf16.shape == tuple(full.shape)
    f16 = f16.cpu().numpy()
    assert f16.tobytes() == twin.to_f16(full).tobytes()
    assert bf16.view(torch.int16).cpu().numpy().tobytes() == twin.to_bf16(full).tobytes()
    assert np.isinf(f16).any() and not np.isinf(full).any()                        # the overflow to Inf is there


def test_float32_through_the_new_argument_is_the_call_without_it(pkg, gpu):
    from clean_pvnet_amd.head import pvnet_head
    d, t = _device_case(gpu, "reference_channels")
    a = pvnet_head(*(t[k] for k in KEYS), compute="float32").cpu().numpy()
    b = pvnet_head(*(t[k] for k in KEYS)).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != _head(d, t, "bfloat16").cpu().numpy().tobytes()           # and the modes are other kernels


# ------------------------------------------------------------------------------------------------------------ 2. views and the module
@pytest.mark.parametrize("mode", twin.DEVICE_MODES)
@pytest.mark.parametrize("name", ["one_by_one", "reference_channels", "no_image"])
def test_channel_slices_give_the_bytes_of_contiguous_copies(pkg, gpu, name, mode):
    import torch
    d, t = _device_case(gpu, name)
    B, C2, C0 = d["B"], d["C2"], d["C0"]
    wide_fm = torch.full((B + 1, C2 + 5, d["h"], d["w"]), float("nan"), device=gpu)
    wide_x = torch.full((B + 1, C0 + 4, 2 * d["h"], 2 * d["w"]), float("nan"), device=gpu)
    wide_fm[:B, 2:2 + C2], wide_x[:B, 1:1 + C0] = t["fm"], t["x"]
    fm, x = wide_fm[:B, 2:2 + C2], wide_x[:B, 1:1 + C0]
    assert fm.stride(0) > C2 * d["h"] * d["w"] and fm.data_ptr() != wide_fm.data_ptr() and (B == 1 or not fm.is_contiguous())
    got = _head(d, {**t, "fm": fm, "x": x}, mode).cpu().numpy()
    assert got.tobytes() == _head(d, t, mode).cpu().numpy().tobytes() and twin.within(got, d[mode], mode)


def _module(gpu, d, mode):
    import torch
    from clean_pvnet_amd.head import PVNetHead
    m = PVNetHead(d["M2"] - 1, 1, s2dim=d["C2"], raw_dim=d["M1"], image_dim=d["C0"], compute=mode).to(gpu).eval().requires_grad_(False)
    with torch.no_grad():
        m.convraw[0].weight.copy_(_t(gpu, d["weight1"]))
        for p, k in ((m.convraw[1].weight, "gamma"), (m.convraw[1].bias, "beta"), (m.convraw[1].running_mean, "mean"),
                     (m.convraw[1].running_var, "var"), (m.convraw[3].weight, "weight2"), (m.convraw[3].bias, "bias2")):
            p.copy_(_t(gpu, d[k]))
    return m


@pytest.mark.parametrize("name", ["two_blocks", "reference_channels"])
def test_module_equals_the_function_on_its_folded_parameters(pkg, gpu, name):
    import torch
    from clean_pvnet_amd.head import PVNetHead
    d, t = _device_case(gpu, name)
    m = _module(gpu, d, "bfloat16")
    assert m.compute == "bfloat16" and all(p.dtype == torch.float32 for p in m.parameters())
    for mode in twin.DEVICE_MODES + ("float32",):
        m.compute = mode                                                            # an attribute, changed between calls
        out = m(t["fm"], t["x"])
        assert out["seg"].untyped_storage().data_ptr() == out["vertex"].untyped_storage().data_ptr()     # views of one tensor
        got = torch.cat([out["seg"], out["vertex"]], 1).cpu().numpy()
        from clean_pvnet_amd.head import pvnet_head
        want = pvnet_head(*(t[k] for k in KEYS), compute=mode).cpu().numpy()
        assert got.tobytes() == want.tobytes(), mode
        if mode != "float32":
            assert twin.within(got, d[mode], mode)
    sd = {k: v for k, v in m.state_dict().items()}
    m2 = PVNetHead.from_state_dict(sd, seg_dim=1, image_dim=d["C0"], compute="bfloat16")
    assert m2.compute == "bfloat16" and set(sd) == set(m2.state_dict())
    with pytest.raises(ValueError, match="compute"):
        PVNetHead(2, 1, compute="float16")
    m2.compute = "bfloat16x3"                                                        # the twin's split mode is not offered
    with pytest.raises(ValueError, match="compute"):
        m2.to(gpu).requires_grad_(False)(t["fm"], t["x"])
    m.compute = "bfloat16"
    with pytest.raises(RuntimeError, match="forward only"):
        m.train()(t["fm"], t["x"])
    with pytest.raises(RuntimeError, match="forward only"):
        m.eval().requires_grad_(True)(t["fm"], t["x"])


@pytest.mark.parametrize("mode", twin.DEVICE_MODES)
def test_module_output_feeds_decode_keypoint_without_a_copy(pkg, gpu, mode):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.head import PVNetHead
    g = torch.Generator(device="cpu").manual_seed(7)
    m = PVNetHead(ver_dim=8, seg_dim=2, s2dim=6, raw_dim=8, compute=mode).eval().requires_grad_(False)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    m = m.to(gpu)
    fm, x = torch.randn(2, 6, 24, 32, generator=g).to(gpu), torch.randn(2, 3, 48, 64, generator=g).to(gpu)
    out = m(fm, x)
    assert not out["vertex"].is_contiguous() and bool(torch.isfinite(out["vertex"]).all())
    views = decode_keypoint(dict(out), seed=5)
    copies = decode_keypoint({"seg": out["seg"].float().contiguous(), "vertex": out["vertex"].float().contiguous()}, seed=5)
    for k in ("mask", "kpt_2d"):
        assert views[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    assert tuple(views["kpt_2d"].shape) == (2, 4, 2) and tuple(views["mask"].shape) == (2, 48, 64)


# ------------------------------------------------------------------------------------------------------------ 3. limits and refusals
def test_limits_and_refusals_are_the_float32_modes(pkg, gpu):
    import torch
    from clean_pvnet_amd.head import pvnet_head
    d, t = _device_case(gpu, "odd_k")
    with pytest.raises(ValueError, match="compute"):
        _head(d, t, "float16")
    with pytest.raises(ValueError, match="compute"):
        _head(d, t, None)
    with pytest.raises(ValueError, match="compute"):
        _head(d, t, "bfloat16x3")
    z = lambda *s: torch.zeros(*s, device=gpu)                                      # noqa: E731
    for mode in ("float32",) + twin.DEVICE_MODES:
        with pytest.raises(ValueError, match=r"\[1, 64\]"):                          # M1 = 65
            pvnet_head(z(1, 2, 4, 4), z(1, 1, 8, 8), z(65, 3, 3, 3), z(65), z(65), z(2, 65), z(2), compute=mode)
        with pytest.raises(RuntimeError, match="do not fit"):                        # a halo that does not fit a CU's LDS
            pvnet_head(z(1, 400, 4, 4), z(1, 0, 8, 8), z(4, 400, 3, 3), z(4), z(4), z(2, 4), z(2), compute=mode)
        out = _head(d, {**t, "fm": t["fm"][:0], "x": t["x"][:0]}, mode, out_dtype=torch.bfloat16)    # B = 0
        assert tuple(out.shape) == (0, d["M2"], 2 * d["h"], 2 * d["w"]) and out.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ 4. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    cases = [_device_case(gpu, name) for name in twin.CASES]
    m = _module(gpu, cases[2][0], "bfloat16")
    m.folded()
    for mode in twin.DEVICE_MODES:                                                  # the first launches (the LDS limit is raised) are not timed paths
        _head(cases[2][0], cases[2][1], mode)
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            runs.append([_head(d, t, mode) for d, t in cases for mode in twin.DEVICE_MODES]
                        + [_head(cases[1][0], cases[1][1], "bfloat16", out_dtype=torch.float16).view(torch.int16),
                           m(cases[2][1]["fm"], cases[2][1]["x"])["vertex"]])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    refs = [(d[mode], mode) for d, _ in cases for mode in twin.DEVICE_MODES]
    for (ref, mode), a in zip(refs, runs[0]):
        assert twin.within(a.cpu().numpy(), ref, mode)
