"""PVNet's decoder stages on the MI355X (``pvnet_stage`` and ``PVNetDecoder`` of clean_pvnet_amd.head): every output equals the numpy
twin (tests/decoder_twin.py, itself held to torch's modules in float64 in tests/test_decoder.py) bit for bit with -0 as +0, on a
side stream as on the default stream; the half-precision stores are the float32 bytes rounded; views are read by their strides;
the decoder equals its twin, its own four function calls, and feeds ``decode_keypoint`` without a copy."""
import numpy as np
import pytest

from tests import decoder_twin as twin
from tests.test_gpu_dcn import on_both_streams
from tests.test_gpu_head import _report

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in twin.KEYS}


def _stage(d, t, **kw):
    from clean_pvnet_amd.head import pvnet_stage
    return pvnet_stage(*(t[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"], **kw)


# ------------------------------------------------------------------------------------------------------------ 1. a stage
@pytest.mark.parametrize("name", list(twin.CASES))
def test_stage_equals_the_twin_bit_for_bit(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: _stage(d, t))
    assert got.shape == d["out"].shape and got.dtype == F32
    assert _report(name, got, d["out"])
    assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("name", list(twin.CASES))
def test_half_stores_are_the_float32_bytes_rounded(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    full = _stage(d, t).cpu().numpy()
    f16, bf16 = _stage(d, t, out_dtype=torch.float16), _stage(d, t, out_dtype=torch.bfloat16)
    assert f16.dtype == torch.float16 and bf16.dtype == torch.bfloat16 and f16.shape == bf16.shape == tuple(full.shape)
    assert f16.cpu().numpy().tobytes() == twin.to_f16(full).tobytes()
    assert bf16.view(torch.int16).cpu().numpy().tobytes() == twin.to_bf16(full).tobytes()


@pytest.mark.parametrize("name", ["one_by_one", "odd_chunks", "stage_2s"])
def test_channel_slices_give_the_bytes_of_contiguous_copies(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    B, C2, C0 = d["B"], d["C2"], d["C0"]
    wide_a = torch.full((B + 1, C2 + 5, d["h"], d["w"]), float("nan"), device=gpu)
    wide_skip = torch.full((B + 1, C0 + 4, d["H"], d["W"]), float("nan"), device=gpu)
    wide_a[:B, 2:2 + C2], wide_skip[:B, 1:1 + C0] = t["a"], t["skip"]
    a, skip = wide_a[:B, 2:2 + C2], wide_skip[:B, 1:1 + C0]
    assert a.stride(0) > C2 * d["h"] * d["w"] and a.data_ptr() != wide_a.data_ptr() and (B == 1 or not a.is_contiguous())
    got = _stage(d, {**t, "a": a, "skip": skip}).cpu().numpy()
    want = _stage(d, t).cpu().numpy()
    assert got.tobytes() == want.tobytes() and _report(name, got, d["out"])


def test_an_empty_batch_gives_an_empty_tensor(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "odd_chunks")
    out = _stage(d, {**t, "a": t["a"][:0], "skip": t["skip"][:0]}, out_dtype=torch.bfloat16)
    assert tuple(out.shape) == (0, d["M"], d["H"], d["W"]) and out.dtype == torch.bfloat16


def test_m_129_is_refused_from_python(pkg, gpu):
    import torch
    from clean_pvnet_amd.head import pvnet_stage
    z = lambda *s: torch.zeros(*s, device=gpu)                                      # noqa: E731
    with pytest.raises(ValueError, match="128"):
        pvnet_stage(z(1, 2, 3, 3), z(1, 1, 6, 6), z(129, 3, 3, 3), z(129), z(129))
    with pytest.raises(RuntimeError, match="136.*not supported"):
        pvnet_stage(z(1, 2, 68, 90), z(1, 1, 135, 180), z(4, 3, 3, 3), z(4), z(4))


# ------------------------------------------------------------------------------------------------------------ 2. the decoder
FEATURES = ("x", "x2s", "x4s", "x8s", "xfc")


def _decoder(gpu):
    import torch
    from clean_pvnet_amd.head import PVNetDecoder
    d = twin.decoder_reference()
    m = PVNetDecoder.from_state_dict({k: torch.tensor(np.asarray(v)) for k, v in d["state"].items()}, seg_dim=d["seg_dim"])
    return d, m.to(gpu).requires_grad_(False), [_t(gpu, d[k]) for k in FEATURES]


def test_decoder_equals_the_twin_and_its_own_four_calls(pkg, gpu):
    import torch
    from clean_pvnet_amd.head import pvnet_head, pvnet_stage
    d, m, feats = _decoder(gpu)
    out = m(*feats)
    assert set(out) == {"seg", "vertex"} and out["seg"].shape[1] == 2 and out["vertex"].shape[1] == 18
    assert out["seg"].untyped_storage().data_ptr() == out["vertex"].untyped_storage().data_ptr()     # views of one tensor
    got = torch.cat([out["seg"], out["vertex"]], 1).cpu().numpy()
    assert _report("decoder_16x24", got, d["out"])
    x, x2s, x4s, x8s, xfc = feats
    fm = pvnet_stage(xfc, x8s, m.conv8s[0].weight, *m.folded("conv8s"), upsample=False)
    fm = pvnet_stage(fm, x4s, m.conv4s[0].weight, *m.folded("conv4s"))
    fm = pvnet_stage(fm, x2s, m.conv2s[0].weight, *m.folded("conv2s"))
    own = pvnet_head(fm, x, m.convraw[0].weight, *m.folded("convraw"), m.convraw[3].weight, m.convraw[3].bias)
    assert got.tobytes() == own.cpu().numpy().tobytes()
    for name in ("conv8s", "conv4s", "conv2s", "convraw"):
        assert m.folded(name)[0].cpu().numpy().tobytes() == d["params"][name + ".scale"].tobytes()
    with pytest.raises(RuntimeError, match="forward only"):
        m.train()(*feats)


def test_decoder_output_feeds_decode_keypoint_without_a_copy(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    d, m, feats = _decoder(gpu)
    feats[0] = torch.nan_to_num(feats[0], nan=0.25, posinf=-0.5)                     # the planted NaN and Inf would reach the votes
    out = m(*feats)
    assert out["vertex"].storage_offset() == 2 * 16 * 24 and bool(torch.isfinite(out["vertex"]).all())   # a view behind seg's channels
    views = decode_keypoint(dict(out), seed=5)
    copies = decode_keypoint({"seg": out["seg"].float().contiguous(), "vertex": out["vertex"].float().contiguous()}, seed=5)
    for k in ("mask", "kpt_2d"):
        assert views[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    assert tuple(views["kpt_2d"].shape) == (1, 9, 2) and tuple(views["mask"].shape) == (1, 16, 24)


# ------------------------------------------------------------------------------------------------------------ 3. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    cases = [_device_case(gpu, name) for name in twin.CASES]
    d, m, feats = _decoder(gpu)
    for name in ("conv8s", "conv4s", "conv2s", "convraw"):
        m.folded(name)
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            runs.append([_stage(c, t) for c, t in cases] + [_stage(cases[1][0], cases[1][1], out_dtype=torch.float16).view(torch.int16),
                                                            m(*feats)["vertex"]])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for (c, _), a in zip(cases, runs[0]):
        assert twin.same_bits(a.cpu().numpy(), c["out"])
