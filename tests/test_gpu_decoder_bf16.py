"""The bfloat16 matrix-core mode of PVNet's decoder stages on the MI355X (``pvnet_stage(compute="bfloat16")`` and
``PVNetDecoder(stage_compute="bfloat16")`` of clean_pvnet_amd.head): every output lies within the twin's ``bound_acc``
(tests/decoder_bf16_twin.py, itself held to the float32 stage's function in tests/test_decoder_bf16.py) with the twin's
non-finite sets, on a side stream as on the default stream; the exact-sum cases equal the twin bit for bit; the half-precision
stores are the float32 bytes rounded; views are read by their strides; the decoder equals its own four calls, each stage within
the twin's bound of the device's own output of the stage before, and feeds ``decode_keypoint`` without a copy."""
import numpy as np
import pytest

from tests import decoder_bf16_twin as twin
from tests import decoder_twin as dt
from tests import head_bf16_twin as hb
from tests import head_twin as ht
from tests.test_gpu_dcn import on_both_streams

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _device_case(gpu, name):
    d = twin.reference(name)
    return d, {k: _t(gpu, d[k]) for k in twin.KEYS}


def _stage(d, t, compute="bfloat16", **kw):
    from clean_pvnet_amd.head import pvnet_stage
    return pvnet_stage(*(t[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"], compute=compute, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. a stage
@pytest.mark.parametrize("name", list(twin.CASES))
def test_stage_lies_within_bound_acc_with_the_twins_non_finite_sets(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: _stage(d, t))
    assert got.shape == d["a64"].shape and got.dtype == F32
    with np.errstate(invalid="ignore"):
        print("%s: worst share of bound_acc %.3g; max |device - a64| = %.3g" % (
            name, twin.worst(got, d), np.nanmax(np.where(np.isfinite(d["a64"]), np.abs(got - d["a64"]), 0))))
    assert twin.within(got, d)
    assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("name", list(twin.EXACT_CASES))
def test_exact_sum_cases_equal_the_twin_bit_for_bit(pkg, gpu, name):
    d, t = _device_case(gpu, name)
    got = on_both_streams(lambda: _stage(d, t))
    diff = ht.canon(got) != ht.canon(d["a32"])
    if diff.any():
        w = tuple(np.argwhere(diff)[0])
        print("%s: %d of %d outputs differ; first at %s: device %r, twin %r" % (name, diff.sum(), diff.size, w, got[w], d["a32"][w]))
    assert not diff.any()


@pytest.mark.parametrize("name", ["odd_chunks", "no_skip_same_res", "straddle", "wide_c16_up", "exact_same"])
def test_half_stores_are_the_float32_bytes_rounded(pkg, gpu, name):
    import torch
    d, t = _device_case(gpu, name)
    full = _stage(d, t).cpu().numpy()
    f16, bf16 = _stage(d, t, out_dtype=torch.float16), _stage(d, t, out_dtype=torch.bfloat16)
    assert f16.dtype == torch.float16 and bf16.dtype == torch.bfloat16 and f16.shape == bf16.shape == tuple(full.shape)
    assert f16.cpu().numpy().tobytes() == twin.to_f16(full).tobytes()
    assert bf16.view(torch.int16).cpu().numpy().tobytes() == twin.to_bf16(full).tobytes()
    assert twin.within(f16.float().cpu().numpy(), d, "float16") and twin.within(bf16.float().cpu().numpy(), d, "bfloat16")


@pytest.mark.parametrize("name", ["one_by_one", "straddle", "c33"])
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
    assert got.tobytes() == _stage(d, t).cpu().numpy().tobytes() and twin.within(got, d)


def test_an_empty_batch_gives_an_empty_tensor(pkg, gpu):
    import torch
    d, t = _device_case(gpu, "odd_chunks")
    out = _stage(d, {**t, "a": t["a"][:0], "skip": t["skip"][:0]}, out_dtype=torch.bfloat16)
    assert tuple(out.shape) == (0, d["M"], d["H"], d["W"]) and out.dtype == torch.bfloat16


@pytest.mark.parametrize("name", ["odd_chunks", "no_skip_same_res", "split_rows"])
def test_float32_through_the_keyword_gives_the_bytes_of_the_call_without_it(pkg, gpu, name):
    from clean_pvnet_amd.head import pvnet_stage
    d, t = _device_case(gpu, name)
    without = pvnet_stage(*(t[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"]).cpu().numpy()
    assert _stage(d, t, compute="float32").cpu().numpy().tobytes() == without.tobytes()
    assert dt.same_bits(without, dt.reference(name)["out"])
    assert _stage(d, t).cpu().numpy().tobytes() != without.tobytes()                # and the mode is another function


# ------------------------------------------------------------------------------------------------------------ 2. the decoder
FEATURES = ("x", "x2s", "x4s", "x8s", "xfc")


def _decoder(gpu, **kw):
    import torch
    from clean_pvnet_amd.head import PVNetDecoder
    d = dt.decoder_reference()
    m = PVNetDecoder.from_state_dict({k: torch.tensor(np.asarray(v)) for k, v in d["state"].items()}, seg_dim=d["seg_dim"], **kw)
    return d, m.to(gpu).requires_grad_(False), [_t(gpu, d[k]) for k in FEATURES]


@pytest.mark.parametrize("compute", ["float32", "bfloat16"])
def test_decoder_equals_its_own_four_calls_and_each_stage_lies_within_the_twins_bound(pkg, gpu, compute):
    import torch
    from clean_pvnet_amd.head import pvnet_head, pvnet_stage
    d, m, feats = _decoder(gpu, stage_compute="bfloat16", compute=compute)
    p = d["params"]
    out = m(*feats)
    got = torch.cat([out["seg"], out["vertex"]], 1).cpu().numpy()
    x, x2s, x4s, x8s, xfc = feats
    fm, own = xfc, {}
    for name, skip in (("conv8s", x8s), ("conv4s", x4s), ("conv2s", x2s)):
        before = fm.cpu().numpy()
        fm = pvnet_stage(fm, skip, getattr(m, name)[0].weight, *m.folded(name), upsample=name != "conv8s", compute="bfloat16")
        own[name] = fm.cpu().numpy()
        ref = twin.stage(before, skip.cpu().numpy(), p[name + ".weight"], p[name + ".scale"], p[name + ".shift"], up=name != "conv8s")
        print("decoder %s: worst share of bound_acc %.3g" % (name, twin.worst(own[name], ref)))
        assert twin.within(own[name], ref) and np.isfinite(own[name]).all(), name   # fed the device's own output of the stage before
    head = pvnet_head(fm, x, m.convraw[0].weight, *m.folded("convraw"), m.convraw[3].weight, m.convraw[3].bias, compute=compute)
    assert got.tobytes() == head.cpu().numpy().tobytes()                           # the decoder is its own four calls
    args = (own["conv2s"], d["x"], p["convraw.weight1"], p["convraw.scale"], p["convraw.shift"], p["convraw.weight2"], p["convraw.bias2"])
    if compute == "float32":                                                       # the head as its own tests hold it
        assert ht.same_bits(got, ht.forward(*args))
    else:
        assert hb.within(got, hb.forward(*args, 0.1, "bfloat16"), "bfloat16")
    m.stage_compute = "float32"                                                    # set between calls: the parent's decoder again
    plain = m(*feats)
    if compute == "float32":
        assert ht.same_bits(torch.cat([plain["seg"], plain["vertex"]], 1).cpu().numpy(), d["out"])
    assert torch.cat([plain["seg"], plain["vertex"]], 1).cpu().numpy().tobytes() != got.tobytes()


def test_decoder_output_feeds_decode_keypoint_without_a_copy(pkg, gpu):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    d, m, feats = _decoder(gpu, stage_compute="bfloat16", compute="bfloat16")
    feats[0] = torch.nan_to_num(feats[0], nan=0.25, posinf=-0.5)                     # the planted NaN and Inf would reach the votes
    out = m(*feats)
    assert out["vertex"].storage_offset() == 2 * 16 * 24 and bool(torch.isfinite(out["vertex"]).all())
    views = decode_keypoint(dict(out), seed=5)
    copies = decode_keypoint({"seg": out["seg"].float().contiguous(), "vertex": out["vertex"].float().contiguous()}, seed=5)
    for k in ("mask", "kpt_2d"):
        assert views[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k


# ------------------------------------------------------------------------------------------------------------ 3. no host sync
def test_nothing_synchronises_and_reruns_give_the_same_bits(pkg, gpu):
    import torch
    cases = [_device_case(gpu, name) for name in list(twin.CASES) + list(twin.EXACT_CASES)]
    d, m, feats = _decoder(gpu, stage_compute="bfloat16")
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
        assert twin.within(a.cpu().numpy(), c)
