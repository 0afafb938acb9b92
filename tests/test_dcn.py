"""DCNv2 modulated deformable convolution (include/pvnet_vote.h's last section, clean_pvnet_amd.dcn, lib.csrc.dcn_v2._ext)
without a GPU: the module, the two entry points and their argument checks exist; the numpy twin of the contract
(tests/dcn_twin.py) emulates ``fmaf`` exactly, reduces to ``unfold`` / ``conv2d`` at zero and integer offsets and stays within
its derived bound of a binary64 evaluation; the reference's own ``lib/networks/dcn_v2.py`` arrives at our entry point with its
own call convention.  The GPU tests (tests/test_gpu_dcn.py) then hold the device to the twin bit for bit."""
import ctypes
import ctypes.util
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import capi
from tests import dcn_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
REFERENCE_DCN = "/root/reference/lib/networks/dcn_v2.py"
SYMBOLS = {"pvv_dcn_forward", "pvv_dcn_columns"}
F32 = np.float32


# ------------------------------------------------------------------------------------------------ 0. the module and the symbols
def test_module_imports(pkg):
    from clean_pvnet_amd import dcn
    assert all(callable(getattr(dcn, f)) for f in ("dcn_v2_conv", "columns", "DCNv2", "DCN"))
    assert dcn.MAX_COLUMNS == 1 << 28


def test_header_declares_and_library_exports_the_two_entry_points():
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in open(HEADER).read()                      # additive: the version did not move


def test_host_side_argument_checks():
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    geo = (3, 3, 1, 1, 1, 1, 1, 1)                                                  # kh, kw, stride, pad, dilation
    fwd = lambda ptrs, strides, shape, g=geo, dg=1: L.pvv_dcn_forward(ptrs[0], ptrs[1], ptrs[2], ptrs[3], strides[0], ptrs[4],  # noqa: E731
                                                                     strides[1], *shape, *g, dg, ptrs[5], None)
    ok_strides = (2 * 9 * 64, 9 * 64)
    assert fwd((None,) * 6, ok_strides, (1, 4, 8, 8, 4)) == -1 and b"NULL" in L.pvv_last_error()
    assert fwd((x, x, None, x, x, None), ok_strides, (1, 4, 8, 8, 4)) == -1 and b"NULL" in L.pvv_last_error()     # (bias may be NULL; out not)
    assert fwd((x,) * 6, ok_strides, (0, 4, 8, 8, 4)) == -1 and b"positive" in L.pvv_last_error()
    assert fwd((x,) * 6, ok_strides, (1, 4, 8, 8, 0)) == -1 and b"positive" in L.pvv_last_error()
    assert fwd((x,) * 6, ok_strides, (1, 4, 8, 8, 4), dg=3) == -1 and b"deformable_groups" in L.pvv_last_error()
    assert fwd((x,) * 6, ok_strides, (1, 4, 8, 8, 4), g=(0, 3, 1, 1, 1, 1, 1, 1)) == -1 and b"kh, kw" in L.pvv_last_error()
    assert fwd((x,) * 6, ok_strides, (1, 4, 8, 8, 4), g=(3, 3, 0, 1, 1, 1, 1, 1)) == -1 and b"stride" in L.pvv_last_error()
    assert fwd((x,) * 6, ok_strides, (1, 4, 2, 2, 4), g=(3, 3, 1, 1, 0, 0, 2, 2)) == -1 and b"larger than" in L.pvv_last_error()
    assert fwd((x,) * 6, (2 * 9 * 64 - 1, 9 * 64), (2, 4, 8, 8, 4)) == -1 and b"image stride" in L.pvv_last_error()
    assert fwd((x,) * 6, (2 * 9 * 64, 9 * 64 - 1), (2, 4, 8, 8, 4)) == -1 and b"image stride" in L.pvv_last_error()
    big = (2 * 9 * 46341 * 46341, 9 * 46341 * 46341)
    assert fwd((x,) * 6, big, (1, 1, 46341, 46341, 1)) == -1 and b"2^31" in L.pvv_last_error()
    col = lambda ptrs, shape: L.pvv_dcn_columns(ptrs[0], ptrs[1], ok_strides[0], ptrs[2], ok_strides[1], *shape, *geo, 1, ptrs[3], None)  # noqa: E731
    assert col((None,) * 4, (1, 4, 8, 8)) == -1 and b"NULL" in L.pvv_last_error()
    assert col((x,) * 4, (1, 4, 8, 0)) == -1 and b"positive" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 1. the emulated fmaf
def test_twin_fmaf_equals_libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    n = 1500
    a = (rng.standard_normal(4 * n) * 10.0 ** rng.integers(-6, 7, 4 * n)).astype(F32)
    b = (rng.standard_normal(4 * n) * 10.0 ** rng.integers(-6, 7, 4 * n)).astype(F32)
    c = (rng.standard_normal(4 * n) * 10.0 ** rng.integers(-6, 7, 4 * n)).astype(F32)
    c[n:2 * n] = -(a[n:2 * n] * b[n:2 * n])                                        # full cancellation of the leading bits
    c[2 * n:3 * n] = (a[2 * n:3 * n].astype(np.float64) * b[2 * n:3 * n] * (1 + 2.0 ** -23 * rng.integers(-3, 4, n))).astype(F32) * F32(-1)
    c[3 * n:] = (a[3 * n:] * b[3 * n:]) * F32(2.0 ** 24) * rng.choice([-1, 1], n).astype(F32)   # the product is half an ulp of c: ties
    a[:8], b[:8], c[:8] = 0, [0, 1, -1, 0, 5, -5, 0, 0], [0, 0, 0, -0.0, -0.0, 0, 1, -1]
    got = twin.fmaf(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[n:2 * n] != 0).any()                                               # the cancellation cases kept the product's tail


# ------------------------------------------------------------------------------------------------ 2. the twin against torch
def _plain(seed, B=2, C=3, M=4, H=7, W=6, kernel=(3, 3), dg=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, H, W)).astype(F32)
    wt = rng.standard_normal((M, C) + kernel).astype(F32)
    bs = rng.standard_normal(M).astype(F32)
    return x, wt, bs


@pytest.mark.parametrize("geo", [dict(stride=1, padding=1, dilation=1), dict(stride=2, padding=2, dilation=2),
                                 dict(stride=(1, 2), padding=(0, 1), dilation=(2, 1))])
def test_twin_at_zero_offsets_is_unfold_and_conv2d(geo):
    import torch
    import torch.nn.functional as F
    x, wt, bs = _plain(1)
    Ho, Wo = twin.out_size(7, 6, (3, 3), **geo)
    off, msk = np.zeros((2, 18, Ho, Wo), F32), np.ones((2, 9, Ho, Wo), F32)
    col = twin.columns(x, off, msk, (3, 3), dg=1, **geo)
    want = F.unfold(torch.from_numpy(x), (3, 3), dilation=geo["dilation"], padding=geo["padding"], stride=geo["stride"]).numpy()
    assert twin.same_bits(col, want)
    out = twin.forward(x, off, msk, wt, bs, **geo)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(bs).double(), **geo).numpy()
    bound = twin.gemm_bound(wt, bs, np.abs(want)).reshape(ref.shape)
    assert (np.abs(out.astype(np.float64) - ref) <= bound).all()
    assert np.abs(out - ref).max() > 0                                             # (float32 does round here)


def test_twin_at_integer_offsets_is_the_shifted_unfold():
    import torch
    import torch.nn.functional as F
    x, _, _ = _plain(2, H=8, W=9)
    dy, dx = 2, -3
    off = np.zeros((2, 9, 2, 8, 9), F32)
    off[:, :, 0], off[:, :, 1] = dy, dx
    col = twin.columns(x, off.reshape(2, 18, 8, 9), np.ones((2, 9, 8, 9), F32), (3, 3), 1, 1, 1)
    big = np.zeros((2, 3, 8 + 8, 9 + 8), F32)                                      # x in a frame of zeros, then unfold the shifted window
    big[:, :, 4:12, 4:13] = x
    shifted = big[:, :, 4 + dy - 1:4 + dy + 8 + 1, 4 + dx - 1:4 + dx + 9 + 1]
    want = F.unfold(torch.from_numpy(np.ascontiguousarray(shifted)), (3, 3)).numpy()
    assert twin.same_bits(col, want)


def test_twin_special_samples():
    """Exactly -1 and exactly H are outside; H - 1 is the last row with no row below; +-1e9 and NaN give a zero column."""
    x = np.arange(1, 13, dtype=F32).reshape(1, 1, 3, 4)
    one = np.ones((1, 1, 3, 4), F32)

    def at(h, w):                                                                   # 1 x 1 kernel: the sample of output pixel (0, 0)
        off = np.zeros((1, 2, 3, 4), F32)
        off[0, 0, 0, 0], off[0, 1, 0, 0] = h, w
        return twin.columns(x, off, one, (1, 1))[0, 0, 0]

    assert at(-1, 0) == 0 and at(0, -1) == 0 and at(3, 0) == 0 and at(0, 4) == 0
    assert at(2, 3) == 12 and at(2, 1) == 10 and at(-0.5, 0) == F32(0.5) and at(2.5, 3.5) == 3
    for v in (1e9, -1e9, np.nan, np.inf):
        assert at(v, 0) == 0 and at(0, v) == 0 and not np.signbit(at(v, 0))
    assert np.isnan(twin.columns(x, np.zeros((1, 2, 3, 4), F32), one * F32(np.nan), (1, 1))).all()   # a NaN mask does reach the column


@pytest.mark.parametrize("name", ["odd_k_small_m", "two_groups_m33", "one_by_one", "uncached_odd_group"])
def test_twin_is_within_the_bound_of_binary64(name):
    d = twin.reference(name)
    args = (d["input"], d["offset"], d["mask"], d["weight"], d["bias"], d["stride"], d["padding"], d["dilation"], d["dg"])
    out64, bound = twin.forward64(*args)
    out = d["out"]
    assert np.isfinite(out).all() and out.shape == (d["B"], d["M"], d["Ho"], d["Wo"])
    err = np.abs(out.astype(np.float64) - out64)
    print("%s: max |out - out64| = %.3g, min bound - err = %.3g" % (name, err.max(), (bound - err).min()))
    assert (err <= bound).all()
    assert err.max() > 0


def test_cases_hold_what_the_gpu_tests_need():
    for name in twin.CASES:
        d = twin.make_inputs(name)
        kinds = {(axis, target if np.isfinite(target) else "nan") for *_, axis, target in d["planted"]}
        H, W = d["H"], d["W"]
        assert {("h", -1.0), ("h", H - 1.0), ("h", float(H)), ("w", -1.0), ("w", W - 1.0), ("w", float(W)), ("h", 1e9), ("w", -1e9),
                ("h", "nan")} <= kinds
        assert np.isnan(d["offset"]).sum() == 1
        assert np.isfinite(twin.reference(name)["col"]).all()                       # the NaN offset gives a zero column, not NaN
        off = d["offset"][np.isfinite(d["offset"])]
        assert (off == np.rint(off)).mean() > 0.05 and (off != np.rint(off)).mean() > 0.5
    KK = lambda c: c["kernel"][0] * c["kernel"][1]                                  # noqa: E731
    assert any(KK(c) > 9 for c in twin.CASES.values()) and any((c["C"] // c["dg"]) * KK(c) % 2 for c in twin.CASES.values())


# ------------------------------------------------------------------------------------------------ 3. refusals and the drop-in surface
def test_cpu_tensors_and_other_dtypes_are_refused(pkg):
    import torch
    from clean_pvnet_amd import dcn
    x, off, msk, wt = torch.zeros(1, 2, 4, 4), torch.zeros(1, 18, 4, 4), torch.ones(1, 9, 4, 4), torch.zeros(3, 2, 3, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn.dcn_v2_conv(x, off, msk, wt, None, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn.columns(x, off, msk, (3, 3), 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        dcn.DCN(2, 3, (3, 3), 1, 1)(x)


def test_requires_grad_is_refused_not_dropped(pkg):
    import torch
    from clean_pvnet_amd import dcn
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)                      # noqa: E731
    named = [("input", meta(1, 2, 4, 4)), ("weight", meta(3, 2, 3, 3, requires_grad=True))]
    real_need = dcn._native.need_cuda
    dcn._native.need_cuda = lambda *a: None                                         # the order of the checks: device, dtype, grad
    try:
        with pytest.raises(RuntimeError, match="forward only"):
            dcn._check(named)
        with torch.no_grad():
            dcn._check(named)
        dcn._check([(n, t.detach()) for n, t in named])
        with pytest.raises(RuntimeError, match="float32"):
            dcn._check([("input", meta(1, 2, 4, 4, dtype=torch.float16))])
    finally:
        dcn._native.need_cuda = real_need


def test_the_three_stubs_raise():
    from lib.csrc.dcn_v2 import _ext
    for f in ("dcn_v2_backward", "dcn_v2_psroi_pooling_forward", "dcn_v2_psroi_pooling_backward"):
        with pytest.raises(NotImplementedError, match="forward pass"):
            getattr(_ext, f)(None, None)
    assert callable(_ext.dcn_v2_forward)


def test_state_dict_names(pkg):
    from clean_pvnet_amd import dcn
    m = dcn.DCN(4, 6, (3, 3), 1, 1, deformable_groups=2)
    sd = m.state_dict()
    assert list(sd) == ["weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"]
    assert tuple(sd["weight"].shape) == (6, 4, 3, 3) and tuple(sd["conv_offset_mask.weight"].shape) == (54, 4, 3, 3)
    assert not sd["conv_offset_mask.weight"].any() and not sd["conv_offset_mask.bias"].any() and not sd["bias"].any()
    assert list(dcn.DCNv2(4, 6, 3, 1, 1).state_dict()) == ["weight", "bias"]


@pytest.mark.skipif(not os.path.exists(REFERENCE_DCN), reason="the reference is not on this machine")
def test_the_references_own_module_runs_on_our_extension(pkg):
    import torch
    from clean_pvnet_amd import dcn
    from lib.csrc.dcn_v2 import _ext
    spec = importlib.util.spec_from_file_location("_reference_dcn_v2", REFERENCE_DCN)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)                                                    # its `from lib.csrc.dcn_v2 import _ext` is ours
    assert ref._backend is _ext and sys.modules["lib.csrc.dcn_v2._ext"] is _ext
    theirs = ref.DCN(4, 4, (3, 3), 1, 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                # its call convention reached our entry point
        theirs(torch.zeros(1, 4, 5, 5))
    ours = dcn.DCN(4, 4, (3, 3), 1, 1)
    assert list(ours.state_dict()) == list(theirs.state_dict())
    assert [tuple(v.shape) for v in ours.state_dict().values()] == [tuple(v.shape) for v in theirs.state_dict().values()]
    ours.load_state_dict(theirs.state_dict())
