"""The bfloat16 compute mode of the output head without a GPU: the header states the flag of ``pvv_head_forward``'s ``out_kind`` and
adds no symbol, the library accepts the flag and refuses what it refused; the twin (tests/head_bf16_twin.py) is order-independent on the exact-sum cases, lies within ``bound_mode`` of the
float32 contract's function and within ``bound_acc`` of its own float32 evaluation; and each rule of the contract, stated wrongly
in the twin, leaves the bound or the exact bits on a named case."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import head_bf16_twin as twin
from tests import head_twin as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_the_header_states_the_flag_and_adds_no_symbol():
    from tests import capi
    with open(os.path.join(ROOT, "include", "pvnet_vote.h")) as f:
        text = f.read()
    assert re.search(r"^#define PVV_HEAD_COMPUTE_BF16 0x100$", text, re.M)         # above the dtype code's low byte
    assert not re.search(r"^#define PVV_HEAD_COMPUTE_BF16X3", text, re.M)            # the split mode is the twin's only: not offered
    assert re.search(r"^#define PVV_ABI_VERSION 8$", text, re.M)
    heads = {sym for sym in capi.declared() if sym.startswith("pvv_head_")}
    assert heads == {"pvv_head_forward", "pvv_head_upsample"} and heads <= capi.exported()
    restype, argtypes = capi.native.declarations("pvnet_vote.h")["pvv_head_forward"]
    assert restype is ctypes.c_int and len(argtypes) == 22 and argtypes[-3] is ctypes.c_int    # out_kind carries the flag


def test_the_flag_is_accepted_and_everything_else_is_refused_as_before():
    """Fails on the parent commit, where PVV_HEAD_OUT_F32 | 0x100 is an unknown dtype code."""
    from tests import capi
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    ok = dict(B=2, C2=4, C0=3, h=5, w=6, H=10, W=12, M1=8, M2=6)
    BF16 = 0x100

    def fwd(ptrs=(x,) * 8, fm_stride=4 * 30, x_stride=3 * 120, kind=BF16, **over):
        s = {**ok, **over}
        return L.pvv_head_forward(ptrs[0], fm_stride, ptrs[1], x_stride, *ptrs[2:7], s["B"], s["C2"], s["C0"], s["h"], s["w"], s["H"],
                                  s["W"], s["M1"], s["M2"], 0.1, kind, ptrs[7], None)

    for kind in (BF16, BF16 | 1, BF16 | 2):                                         # the flag with each dtype code passes the kind check
        assert fwd((None,) * 8, kind=kind) == -1 and b"NULL" in L.pvv_last_error()
    for kind in (BF16 | 3, 0x200, 0x300, 0x10000 | BF16, -1, BF16 - (1 << 31)):     # 0x200 is kept free for the split mode
        assert fwd(kind=kind) == -1 and b"dtype code" in L.pvv_last_error(), kind
    for i in range(8):
        assert fwd(tuple(None if j == i else x for j in range(8))) == -1 and b"NULL" in L.pvv_last_error()
    assert fwd(B=0) == -1 and b"positive" in L.pvv_last_error()
    assert fwd(B=65536) == -1 and b"65535" in L.pvv_last_error()
    assert fwd(H=11) == -1 and b"2*h" in L.pvv_last_error()
    assert fwd(M1=65) == -1 and b"<= 64" in L.pvv_last_error()
    assert fwd(M2=65) == -1 and b"<= 64" in L.pvv_last_error()
    assert fwd(x_stride=3 * 120 - 1) == -1 and b"image stride" in L.pvv_last_error()
    big = dict(C2=1, C0=0, h=23171, w=23171, H=46342, W=46342)                      # H * W > 2^31
    assert fwd(fm_stride=23171 * 23171, **big) == -1 and b"2^31" in L.pvv_last_error()
    assert fwd(C2=120, fm_stride=120 * 30) == -1 and b"LDS" in L.pvv_last_error()  # the halo of 123 channels does not fit


# ------------------------------------------------------------------------------------------------------------ the exact cases
@pytest.mark.parametrize("name", list(twin.EXACT_CASES))
def test_exact_sum_cases_are_order_independent(name):
    d = twin.reference(name)
    ref = d["bfloat16"]
    want = ref["out64"].astype(F32)
    assert np.array_equal(want.astype(np.float64), ref["out64"]) and np.isfinite(want).all()
    assert len(np.unique(want)) > 50                                                # not a degenerate picture
    assert twin.same_bits(ref["out32"], want)
    for order in ("descending", "permuted"):
        got = twin.forward(*(d[k] for k in twin.KEYS), d["slope"], "bfloat16", order=order, seed=11)["out32"]
        assert twin.same_bits(got, want), order
    w2 = d["weight2"].reshape(d["M2"], d["M1"])
    assert ((w2 != 0).sum(1) == 1).all() and (np.diff(np.argmax(w2 != 0, axis=1)) != 0).all()


# ------------------------------------------------------------------------------------------------------------ the two bounds
def _bn(d):
    return (d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])


@pytest.mark.parametrize("mode", twin.MODES)
@pytest.mark.parametrize("name", list(twin.CASES))
def test_out64_lies_within_bound_mode_of_the_float32_contracts_function(name, mode):
    d = twin.reference(name)
    true64, bound = twin.bound_mode(d["fm"], d["x"], d["weight1"], _bn(d), d["weight2"], d["bias2"], d["slope"], mode)
    out64 = d[mode]["out64"]
    f = np.isfinite(true64)
    assert np.array_equal(f, np.isfinite(out64)) and f.any() and not f.all()
    err = np.abs(out64[f] - true64[f])
    print("%s %s: worst |out64 - forward64| / bound_mode = %.3g" % (name, mode, (err / bound[f]).max()))
    assert (err <= bound[f]).all()


@pytest.mark.parametrize("mode", twin.MODES)
@pytest.mark.parametrize("name", list(twin.CASES) + list(twin.EXACT_CASES))
def test_the_twins_float32_evaluation_lies_within_bound_acc(name, mode):
    ref = twin.reference(name)[mode]
    print("%s %s: worst |out32 - out64| / bound_acc = %.3g" % (name, mode, twin.worst(ref["out32"], ref)))
    assert twin.within(ref["out32"], ref, mode)


def test_bound_mode_of_x3_is_at_most_2_to_the_minus_6_of_bfloat16s():
    d = twin.reference("reference_channels")
    args = (d["fm"], d["x"], d["weight1"], _bn(d), d["weight2"], d["bias2"], d["slope"])
    _, b1 = twin.bound_mode(*args, "bfloat16")
    _, b3 = twin.bound_mode(*args, "bfloat16x3")
    f = np.isfinite(b1)
    assert f.any() and (b3[f] <= 2.0 ** -6 * b1[f]).all()


# ------------------------------------------------------------------------------------------------------------ the rules
def _leaves(name, mode, **wrong):
    """Whether the twin with one rule stated wrongly leaves the right twin's ``bound_acc`` (or, on an exact case, its bits)."""
    d = twin.reference(name)
    ref = d[mode]
    got = twin.forward(*(d[k] for k in twin.KEYS), d["slope"], mode, **wrong)["out64"]
    if name in twin.EXACT_CASES:
        return not twin.same_bits(got.astype(F32), ref["out64"].astype(F32))
    f = np.isfinite(ref["out64"]) & np.isfinite(got)
    return bool((np.abs(got[f] - ref["out64"][f]) > ref["bound_acc"][f]).any())


@pytest.mark.parametrize("name, mode, wrong", [
    ("exact_reference_channels", "bfloat16", dict(rounding="truncate")),           # truncation instead of nearest-even
    ("reference_channels", "bfloat16x3", dict(keep_lo=False)),                     # lo dropped
    ("reference_channels", "bfloat16x3", dict(drop=0)),                            # hi*hi dropped
    ("reference_channels", "bfloat16x3", dict(drop=1)),                            # hi*lo dropped
    ("reference_channels", "bfloat16x3", dict(drop=2)),                            # lo*hi dropped
    ("reference_channels", "bfloat16", dict(round_w1=False)),                      # weight1 left unrounded
    ("exact_two_blocks", "bfloat16", dict(round_a=False)),                         # a left unrounded before conv2
    ("odd_k", "bfloat16", dict(round_bias=True)),                                  # bias2 rounded: 70000 becomes 70144
    ("odd_k", "bfloat16x3", dict(round_bias=True)),
], ids=lambda v: v if isinstance(v, str) else "-".join("%s=%s" % kv for kv in v.items()))
def test_a_rule_stated_wrongly_leaves_the_bound_or_the_bits(name, mode, wrong):
    assert _leaves(name, mode, **wrong)
    assert not _leaves(name, mode)                                                  # and the rule stated rightly does not


def test_the_modes_and_the_cases_are_the_issues():
    assert set(ht.CASES) < set(twin.CASES) and twin.CASES["c16"]["C2"] + twin.CASES["c16"]["C0"] == 16
    assert twin.CASES["c17"]["C2"] + twin.CASES["c17"]["C0"] == 17
    for name in ht.CASES:                                                            # the plants are head_twin's, but for the last row
        a, b = ht.make_inputs(name), twin.make_inputs(name)
        for k in ("fm", "x", "weight1", "gamma", "beta", "mean", "var"):
            assert a[k].tobytes() == b[k].tobytes()
        assert np.array_equal(a["weight2"][:-1], b["weight2"][:-1]) and np.abs(b["weight2"]).max() < 10 and b["bias2"][0] == 70000
