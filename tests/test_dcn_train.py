"""The DCNv2 backward pass (include/pvnet_vote.h "Modulated deformable convolution, backward", clean_pvnet_amd.dcn_train) without
a GPU: the numpy twin of the contract (tests/dcn_train_twin.py) stays within its derived bound of ``backward64`` -- the same
function in torch ops in binary64, differentiated by autograd --, its fixed-point scatter is exact up to the quantum and does
not depend on the order of arrival, the module refuses what ``dcn`` refuses, keeps the reference's parameter names and swaps
into a model, and the library exports what the header declares.  The GPU tests (tests/test_gpu_dcn_train.py) then hold the
device to the twin bit for bit."""
import os

import numpy as np
import pytest

from tests import capi
from tests import dcn_train_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
F32 = np.float32
NAMES = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")
CPU_CASES = ("odd_k_small_m", "two_groups_m33", "one_by_one", "uncached_odd_group")


def _args(d):
    return d["input"], d["offset"], d["mask"], d["weight"]


def _geo(d):
    return d["stride"], d["padding"], d["dilation"], d["dg"]


# ------------------------------------------------------------------------------------------------ 1. the twin against backward64
@pytest.mark.parametrize("name", CPU_CASES)
def test_twin_is_within_the_bound_of_backward64(name):
    """Every one of the five gradients lies within gamma_n * sum |terms| of the binary64 autograd result, with (one added to
    each for the binary64 arithmetic): grad_input n = M + 8 plus half a quantum per contribution, grad_offset and grad_mask
    n = M + Cg + 10, grad_weight n = SLAB + 11, grad_bias n = 3 (the counts are derived in dcn_train_twin.bounds).  The largest
    error is not zero, and the planted samples far outside and on a NaN offset have gradients of exactly +0."""
    d = twin.reference(name)
    want = twin.backward64(*_args(d), d["bias"], d["gout"], *_geo(d))
    bound = twin.bounds(*_args(d), d["gout"], *_geo(d))
    KK = d["kernel"][0] * d["kernel"][1]
    far = np.zeros((d["B"], d["dg"], KK, d["Ho"], d["Wo"]), bool)
    for b, g, t, y, x, axis, target in d["planted"]:
        if not np.isfinite(target) or abs(target) > 1e6:
            far[b, g, t, y, x] = True
    assert far.sum() == 3
    for what, got, ref, bnd in zip(NAMES, d["grads"], want, bound):
        assert got.dtype == F32 and got.shape == ref.shape == bnd.shape, what
        assert np.isfinite(got).all(), what
        ref = np.nan_to_num(ref, nan=0.0) if what in ("grad_offset",) else ref     # (autograd gives the NaN offset no gradient: 0)
        err = np.abs(got.astype(np.float64) - ref)
        print("%s %s: max err %.3g, max bound %.3g, worst err / bound %.3g" % (name, what, err.max(), bnd.max(), (err / np.maximum(bnd, 1e-300)).max()))
        assert (err <= bnd).all(), what
        assert err.max() > 0, what
    goff = d["grads"][1].reshape(d["B"], d["dg"], KK, 2, d["Ho"], d["Wo"])
    gmask = d["grads"][2].reshape(d["B"], d["dg"], KK, d["Ho"], d["Wo"])
    for arr in (goff[:, :, :, 0][far], goff[:, :, :, 1][far], gmask[far]):
        assert arr.size == 3 and not arr.view(np.uint32).any()                     # +0, by its bits
    assert goff[:, :, :, 0][~far].any() and gmask[~far].any()


def test_planted_sites_outside_the_window_contribute_nothing():
    """-1 and H (W) are outside the forward's window: exactly +0 for both offset gradients and the mask gradient there."""
    d = twin.reference("odd_k_small_m")
    KK = 9
    goff = d["grads"][1].reshape(d["B"], d["dg"], KK, 2, d["Ho"], d["Wo"])
    gmask = d["grads"][2].reshape(d["B"], d["dg"], KK, d["Ho"], d["Wo"])
    seen = 0
    for b, g, t, y, x, axis, target in d["planted"]:
        if target in (-1.0, float(d["H"] if axis == "h" else d["W"])):
            seen += 1
            assert not goff[b, g, t, :, y, x].view(np.uint32).any() and not gmask[b, g, t, y, x].view(np.uint32)
    assert seen == 4


# ------------------------------------------------------------------------------------------------ 2. the fixed-point scatter
@pytest.mark.parametrize("name", ["odd_k_small_m", "uncached_odd_group"])
def test_fixed_point_scatter_is_exact_to_the_quantum_and_order_independent(name):
    """Against the same float32 contributions added in binary64: each is rounded to a multiple of q = 2^(e - 40) (at most q/2
    off), the int64 sum is exact, and the result is rounded to binary64 and float32 once each:
    |twin - sum64| <= count * q/2 + (2^-24 + 2^-52) * (|sum64| + count * q/2)."""
    d = twin.reference(name)
    x = d["input"]
    B, C = d["B"], d["C"]
    tp = twin.taps(x.shape, d["offset"], d["kernel"], *_geo(d))
    gc5 = twin.gcol(d["weight"], d["gout"]).reshape(B, d["dg"], C // d["dg"], tp["KK"], tp["P"])
    _, _, maxbits = twin.coord(x, d["mask"], gc5, tp, d["dg"])
    img, elem, vals = twin.contributions(d["mask"], gc5, tp, d["dg"], x.shape)
    got = twin.fixed_point_scatter(img, elem, vals, maxbits, x.shape)
    assert got.tobytes() == d["grads"][0].tobytes()
    total, count = twin.float64_scatter(img, elem, vals, x.shape)
    half_q = np.array([2.0 ** (twin.pow2_exp(int(m)) - twin.FIX - 1) for m in maxbits])[:, None, None, None]
    bound = count * half_q + (2.0 ** -24 + 2.0 ** -52) * (np.abs(total) + count * half_q)
    err = np.abs(got.astype(np.float64) - total)
    print("%s: max err %.3g, max bound %.3g, largest count %d" % (name, err.max(), bound.max(), count.max()))
    assert (err <= bound).all() and err.max() > 0 and count.max() > 4
    for b in range(B):                                                             # the maximum bounds every contribution
        assert np.abs(vals[img == b]).max() <= 2.0 ** twin.pow2_exp(int(maxbits[b]))
    rng = np.random.default_rng(11)
    for _ in range(2):
        again = twin.fixed_point_scatter(img, elem, vals, maxbits, x.shape, order=rng.permutation(vals.size))
        assert again.tobytes() == got.tobytes()
    plain = np.zeros((B, x[0].size), F32)                                          # float32 additions do depend on the order
    np.add.at(plain, (img, elem), vals)
    order = rng.permutation(vals.size)
    shuffled = np.zeros_like(plain)
    np.add.at(shuffled, (img[order], elem[order]), vals[order])
    assert plain.tobytes() != shuffled.tobytes()


def test_pow2_exp_and_a_maximum_that_is_not_finite():
    for value, e in ((1.0, 0), (1.5, 1), (2.0, 1), (0.75, 0), (0.5, -1), (2.0 ** -149, -149), (3 * 2.0 ** -149, -147), (2.0 ** -126, -126),
                     (3.4e38, 128)):
        assert twin.pow2_exp(F32(value).view(np.uint32)) == e, value
    img, elem, vals = np.array([0, 1]), np.array([2, 3]), np.array([1.0, 1.0], F32)
    out = twin.fixed_point_scatter(img, elem, vals, np.array([0x7F800000, 0x3F800000], np.uint32), (2, 1, 2, 2))
    assert np.isnan(out[0]).all() and out[1].ravel().tolist() == [0, 0, 0, 1]
    out = twin.fixed_point_scatter(img, elem, vals * 0, np.array([0, 0], np.uint32), (2, 1, 2, 2))
    assert not out.view(np.uint32).any()


def test_grad_bias_and_grad_weight_orders():
    """The two binary64 reductions against exact rational sums on integers, where every order gives the same value, and the
    slab boundary of grad_weight: a chain that restarts at pixel SLAB."""
    rng = np.random.default_rng(3)
    go = rng.integers(-8, 9, (2, 3, 20, 30)).astype(F32)
    assert np.array_equal(twin.grad_bias(go), go.sum(axis=(0, 2, 3)))
    P = twin.SLAB + 3
    col, g = np.ones((1, 1, P), F32), np.ones((1, 1, P), F32)
    col[0, 0, 0], g[0, 0, 1:twin.SLAB] = F32(2.0 ** 24), 0                          # 2^24 + 1 + 1 + 1: a float32 chain over all pixels loses them
    got = twin.grad_weight(col, g, (1, 1, 1, 1))
    assert got[0, 0, 0, 0] == F32(2.0 ** 24 + 4) and got[0, 0, 0, 0] != F32(2.0 ** 24)


# ------------------------------------------------------------------------------------------------ 3. refusals and the modules
def test_cpu_tensors_and_float16_are_refused(pkg):
    import torch
    from clean_pvnet_amd import dcn_train
    x, off, msk = torch.zeros(1, 2, 4, 4), torch.zeros(1, 18, 4, 4), torch.ones(1, 9, 4, 4)
    wt = torch.zeros(3, 2, 3, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn_train.dcn_v2_conv(x, off, msk, wt, None, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn_train.dcn_v2_backward(x, off, msk, wt, None, torch.zeros(1, 3, 4, 4), 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn_train.DCN(2, 3, (3, 3), 1, 1)(x)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn_train.DCNv2(2, 3, (3, 3), 1, 1)(x, off, msk)
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)                      # noqa: E731
    real_need = dcn_train._native.need_cuda
    dcn_train._native.need_cuda = lambda *a: None                                   # past the device check: the dtype check is next
    try:
        with pytest.raises(RuntimeError, match="float32"):
            dcn_train.dcn_v2_conv(meta(1, 2, 4, 4, dtype=torch.float16), meta(1, 18, 4, 4), meta(1, 9, 4, 4), meta(3, 2, 3, 3), None, 1, 1, 1, 1)
        with pytest.raises(RuntimeError, match="float32"):
            dcn_train.dcn_v2_backward(meta(1, 2, 4, 4), meta(1, 18, 4, 4), meta(1, 9, 4, 4), meta(3, 2, 3, 3), None,
                                      meta(1, 3, 4, 4, dtype=torch.float16), 1, 1, 1, 1)
    finally:
        dcn_train._native.need_cuda = real_need


def test_state_dict_names_equal_dcn(pkg):
    from clean_pvnet_amd import dcn, dcn_train
    ours, theirs = dcn_train.DCN(4, 6, (3, 3), 1, 1, deformable_groups=2), dcn.DCN(4, 6, (3, 3), 1, 1, deformable_groups=2)
    assert isinstance(ours, dcn.DCN) and isinstance(dcn_train.DCNv2(4, 6, 3, 1, 1), dcn.DCNv2)
    assert list(ours.state_dict()) == list(theirs.state_dict()) == ["weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"]
    assert [tuple(v.shape) for v in ours.state_dict().values()] == [tuple(v.shape) for v in theirs.state_dict().values()]
    ours.load_state_dict(theirs.state_dict())
    assert list(dcn_train.DCNv2(4, 6, 3, 1, 1).state_dict()) == ["weight", "bias"]


def test_convert_swaps_the_classes_and_keeps_the_parameters(pkg):
    from torch import nn
    from clean_pvnet_amd import dcn, dcn_train
    a, b = dcn.DCN(4, 6, 3, 1, 1), dcn.DCNv2(6, 2, 3, 1, 1)
    model = nn.Sequential(a, nn.ReLU(), nn.Sequential(b))
    before = list(model.parameters())
    names = list(model.state_dict())
    got = dcn_train.convert(model)
    assert got is model and type(model[0]) is dcn_train.DCN and type(model[2][0]) is dcn_train.DCNv2 and type(model[1]) is nn.ReLU
    assert all(p is q for p, q in zip(before, model.parameters())) and len(before) == len(list(model.parameters())) == 6
    assert list(model.state_dict()) == names
    assert model[0].conv_offset_mask is a.conv_offset_mask and model[0].stride == a.stride
    assert type(a) is dcn.DCN                                                       # the layer that was replaced is as it was
    alone = dcn_train.convert(a)
    assert type(alone) is dcn_train.DCN and alone.weight is a.weight
    assert dcn_train.convert(alone) is alone


# ------------------------------------------------------------------------------------------------ 4. header and library
def test_header_declares_and_library_exports_the_backward_entry_points():
    declared = {s for s in capi.declared() if s.startswith("pvv_dcn_backward")}
    assert declared == {"pvv_dcn_backward", "pvv_dcn_backward_workspace_bytes"}
    assert declared <= capi.exported()
    assert capi.load().pvv_abi_version() == 8 and "#define PVV_ABI_VERSION 8" in open(HEADER).read()
    assert "#define PVV_DCN_SLAB %d" % twin.SLAB in open(HEADER).read()


def test_workspace_is_bounded_whatever_the_batch_and_the_host_checks():
    L = capi.load()
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    ws = lambda B, chunk=0, shape=(64, 135, 180, 64): L.pvv_dcn_backward_workspace_bytes(B, *shape, *geo, chunk)   # noqa: E731
    one = ws(1)
    assert 0 < one and ws(32) == ws(4096) <= one + (256 << 20)                       # the default chunk: what fits 256 MiB
    assert ws(5, 2, (3, 7, 9, 5)) < ws(5, 5, (3, 7, 9, 5)) == ws(5, 0, (3, 7, 9, 5)) == ws(5, 99, (3, 7, 9, 5))
    assert ws(0) == -1 and b"positive" in L.pvv_last_error()
    assert ws(1, 0, (1, 2000, 2000, 1)) == -1 and b"2^22" in L.pvv_last_error()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    bwd = lambda ptrs, wsp, nbytes, B=1: L.pvv_dcn_backward(ptrs[0], ptrs[1], ptrs[2], 18 * 63, ptrs[3], 9 * 63, ptrs[4], B, 3, 7, 9, 5, *geo,  # noqa: E731
                                                            x, x, x, x, x, wsp, nbytes, None)
    assert bwd((x, x, None, x, x), x, 1 << 30) == -1 and b"NULL" in L.pvv_last_error()
    assert bwd((x,) * 5, None, 1 << 30) == -1 and b"aligned" in L.pvv_last_error()
    assert bwd((x,) * 5, 264, 1 << 30) == -1 and b"aligned" in L.pvv_last_error()
    assert bwd((x,) * 5, x, ws(1, 1, (3, 7, 9, 5)) - 1) == -2 and b"smaller" in L.pvv_last_error()
