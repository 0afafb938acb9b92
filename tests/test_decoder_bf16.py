"""The bfloat16 matrix-core mode of PVNet's decoder stages (include/pvnet_vote.h, "PVNet decoder stage", compute mode;
``pvnet_stage(compute=...)`` and ``PVNetDecoder(stage_compute=...)`` of clean_pvnet_amd.head) without a GPU: the header states the
flag; the library takes it beside ``PVV_HEAD_STAGE`` and nowhere else -- with pointers that are never dereferenced, every call
ends in a refusal before any launch --; the Python surface validates and keeps the keyword; the twin
(tests/decoder_bf16_twin.py) lies within ``bound_mode`` of the float32 stage's function, its own float32 evaluations lie within
``bound_acc`` in three orders, the exact-sum cases give one result in all of them, and a rule stated wrongly leaves the bound
or the bits; the built kernels spill nothing and ask for the LDS the host's expression states.  The GPU tests
(tests/test_gpu_decoder_bf16.py) then hold the device to the twin's bound."""
import os
import re

import numpy as np
import pytest

from tests import decoder_bf16_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
STAGE, SAME_RES, STAGE_BF16 = 0x400, 0x800, 0x2000


# ------------------------------------------------------------------------------------------------ 1. the flag of out_kind
def test_the_header_states_the_flag_and_adds_no_symbol():
    from tests import capi
    with open(os.path.join(ROOT, "include", "pvnet_vote.h")) as f:
        text = f.read()
    assert re.search(r"^#define PVV_HEAD_STAGE_BF16\s+0x2000\b", text, re.M)
    assert re.search(r"^#define PVV_ABI_VERSION 8$", text, re.M)
    heads = {sym for sym in capi.declared() if sym.startswith("pvv_head_")}
    assert heads == {"pvv_head_forward", "pvv_head_upsample"} and heads <= capi.exported()


def test_the_flag_is_accepted_beside_the_stage_flag_and_refused_everywhere_else():
    """Fails on the parent commit, where PVV_HEAD_STAGE | 0x2000 is an unknown dtype code.  No call here reaches a launch: a call
    that passes the pointer check is given an H of more tiles than one launch takes, the check that follows it."""
    from tests import capi
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    up = dict(B=2, C2=4, C0=3, h=5, w=6, H=10, W=12, M1=8, M2=6)
    same = dict(up, H=5, W=6)
    tall = dict(h=262144, w=1, H=524288, W=2)                                        # 65536 tiles along H: refused after the pointers
    tall_same = dict(h=524288, w=2, H=524288, W=2)

    def fwd(shape, ptrs=(x,) * 8, kind=STAGE | STAGE_BF16, **over):
        s = {**shape, **over}
        fm_stride, x_stride = s["C2"] * s["h"] * s["w"], s["C0"] * s["H"] * s["W"]
        return L.pvv_head_forward(ptrs[0], fm_stride, ptrs[1], x_stride, *ptrs[2:7], s["B"], s["C2"], s["C0"], s["h"], s["w"], s["H"],
                                  s["W"], s["M1"], s["M2"], 0.1, kind, ptrs[7], None)

    def refused(rc, word):
        msg = L.pvv_last_error()
        assert rc == -1 and word in msg, (rc, msg)
        return True

    for shape, tall_shape, flags in ((up, tall, STAGE | STAGE_BF16), (same, tall_same, STAGE | SAME_RES | STAGE_BF16)):
        for code in (0, 1, 2):                                                      # the flags with each dtype code pass the kind check
            assert refused(fwd(shape, (None,) * 8, kind=flags | code), b"NULL") and b"dtype code" not in L.pvv_last_error()
        for i in (0, 1, 2, 3, 4, 7):                                                # each of the six pointers a stage reads, alone
            assert refused(fwd(shape, tuple(None if j == i else x for j in range(8)), kind=flags), b"NULL")
        no_conv2 = (x, x, x, x, x, None, None, x)                                   # d_weight2 and d_bias2 are not read
        assert refused(fwd(shape, no_conv2, kind=flags, **tall_shape), b"too large for one launch")
        assert refused(fwd(shape, no_conv2, kind=flags, M2=0, **tall_shape), b"too large for one launch")     # nor is M2
        assert refused(fwd(shape, (x, None, x, x, x, None, None, x), kind=flags, C0=0, **tall_shape), b"too large")   # d_x with C0 = 0
        assert refused(fwd(shape, kind=flags | 3), b"dtype code")
        assert refused(fwd(shape, kind=flags, M1=128, **tall_shape), b"too large for one launch")             # past the M check
        assert refused(fwd(shape, kind=flags, M1=129), b"<= 128")
        assert refused(fwd(shape, kind=flags, C2=400, **tall_shape), b"too large for one launch") and b"LDS" not in L.pvv_last_error()
    assert refused(fwd(up, kind=STAGE | SAME_RES | STAGE_BF16), b"PVV_HEAD_SAME_RES")   # H = 2h under SAME_RES
    assert refused(fwd(same, kind=STAGE | STAGE_BF16), b"2*h")                      # and H = h without it
    assert refused(fwd(up, kind=STAGE | STAGE_BF16, C2=1, C0=0, h=23171, w=23171, H=46342, W=46342), b"2^31")
    for kind in (STAGE_BF16, STAGE_BF16 | 0x100, STAGE_BF16 | SAME_RES, STAGE | STAGE_BF16 | 0x100, STAGE | STAGE_BF16 | 3,
                 STAGE | STAGE_BF16 | 0x200, STAGE | STAGE_BF16 | 0x1000, STAGE | STAGE_BF16 | 0x4000, STAGE_BF16 | 1):
        assert refused(fwd(up, kind=kind), b"dtype code"), kind


# ------------------------------------------------------------------------------------------------ 2. the Python surface
def test_compute_values_are_validated_and_cpu_tensors_refused(pkg):
    import torch
    from clean_pvnet_amd import head
    assert head.STAGE_BF16 == STAGE_BF16
    xfc, x8s, w, s = torch.zeros(1, 8, 2, 2), torch.zeros(1, 128, 2, 2), torch.zeros(5, 136, 3, 3), torch.zeros(5)
    with pytest.raises(ValueError, match="compute must be one of 'float32', 'bfloat16'"):
        head.pvnet_stage(xfc, x8s, w, s, s, upsample=False, compute="bfloat16x3")
    with pytest.raises(ValueError, match="compute must be one of 'float32', 'bfloat16'"):
        head.PVNetDecoder(4, 2, stage_compute="half")
    with pytest.raises(ValueError, match="compute must be one of"):
        head.PVNetDecoder.from_state_dict(head.PVNetDecoder(4, 2, fcdim=8, s8dim=6, s4dim=5, s2dim=4, raw_dim=7).state_dict(),
                                          stage_compute=None)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        head.pvnet_stage(xfc, x8s, w, s, s, upsample=False, compute="bfloat16")
    m = head.PVNetDecoder(4, 2, fcdim=8, s8dim=6, s4dim=5, s2dim=4, raw_dim=7, stage_compute="bfloat16").eval()
    assert (m.compute, m.stage_compute) == ("float32", "bfloat16")                 # compute keeps meaning the head only
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"), torch.no_grad():
        m(torch.zeros(1, 3, 16, 16), torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 4, 4), torch.zeros(1, 128, 2, 2), xfc)
    assert head.PVNetDecoder(4, 2).stage_compute == "float32"


def test_stage_compute_survives_from_state_dict_and_from_module(pkg):
    from torch import nn
    from clean_pvnet_amd import head
    src = head.PVNetDecoder(4, 2, fcdim=8, s8dim=6, s4dim=5, s2dim=4, raw_dim=7)
    a = head.PVNetDecoder.from_state_dict(src.state_dict(), stage_compute="bfloat16")
    assert (a.compute, a.stage_compute) == ("float32", "bfloat16") and not a.training
    b = head.PVNetDecoder.from_state_dict(src.state_dict(), compute="bfloat16")
    assert (b.compute, b.stage_compute) == ("bfloat16", "float32")

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.ver_dim, self.seg_dim = 4, 2
            self.conv8s, self.conv4s, self.conv2s, self.convraw = src.conv8s, src.conv4s, src.conv2s, src.convraw
    c = head.PVNetDecoder.from_module(Net().eval(), stage_compute="bfloat16")
    assert (c.compute, c.stage_compute) == ("float32", "bfloat16") and c.conv8s is src.conv8s
    assert head.PVNetDecoder.from_module(Net().eval()).stage_compute == "float32"
    with pytest.raises(ValueError, match="compute must be one of"):
        head.PVNetDecoder.from_module(Net().eval(), stage_compute="half")
    c.stage_compute = "float32"                                                     # an attribute that may be set between calls
    assert c.stage_compute == "float32"


# ------------------------------------------------------------------------------------------------ 3. the twin
def test_the_cases_are_the_issues():
    from tests import decoder_twin as dt
    assert list(twin.CASES)[:9] == list(dt.CASES) and len(dt.CASES) == 9
    c = {n: (v["C2"] + v["C0"], v) for n, v in twin.CASES.items()}
    assert c["c16"][0] == 16 and c["c17"][0] == 17
    s = twin.CASES["straddle"]
    assert s["C2"] % 8 and s["C0"] > 0 and s["C2"] // 8 < (s["C2"] + s["C0"] - 1) // 8      # a group with channels of both
    assert c["c32"][0] == twin.CHUNK and c["c33"][0] == twin.CHUNK + 1
    for name in ("wide_c16_up", "wide_c17_same", "wide_two_up", "wide_two_same"):           # the launch keeps M in one workgroup
        v = twin.CASES[name]
        H, W = (2 * v["h"], 2 * v["w"]) if v["up"] else (v["h"], v["w"])
        assert v["B"] * ((H + 7) // 8) * ((W + 31) // 32) >= twin.FILL
    assert c["wide_c16_up"][0] == 16 and c["wide_c17_same"][0] == 17                        # the chunk of four row blocks, and + 1
    assert twin.CASES["wide_c16_up"]["M"] > 64 and 32 < twin.CASES["wide_two_up"]["M"] <= 64
    assert {v["up"] for v in twin.EXACT_CASES.values()} == {True, False}
    for name in twin.CASES:
        d = twin.reference(name)
        assert np.isnan(d["a"]).sum() == 1 and np.isposinf(d["a"]).sum() == 1
        assert np.isnan(d["a64"]).any() and np.isfinite(d["a64"]).any()


@pytest.mark.parametrize("name", list(twin.CASES))
def test_a64_lies_within_bound_mode_of_the_float32_stages_function(name):
    d = twin.reference(name)
    true64, bound = twin.bound_mode(d["a"], d["skip"], d["weight"], (d["gamma"], d["beta"], d["mean"], d["var"], d["eps"]), d["slope"],
                                    up=d["up"])
    f = np.isfinite(true64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(d["a64"] - true64)[f]
        print("%s: max |a64 - stage64| = %.3g, worst share of bound_mode %.3g" % (name, err.max(), np.nanmax(err / bound[f])))
    assert f.any() and twin.nonfinite_sets_match(d["a64"], true64) and (err <= bound[f]).all() and err.max() > 0


@pytest.mark.parametrize("name", list(twin.CASES) + list(twin.EXACT_CASES))
def test_the_twins_float32_evaluation_lies_within_bound_acc_in_three_orders(name):
    d = twin.reference(name)
    shares = {"ascending": twin.worst(d["a32"], d)}
    assert twin.within(d["a32"], d)
    for order in twin.ORDERS[1:]:
        a32 = twin.stage(*(d[k] for k in twin.KEYS), d["slope"], up=d["up"], order=order, seed=7)["a32"]
        assert twin.within(a32, d), order
        for kind in ("float16", "bfloat16"):                                        # the store's rounding on both ends of the interval
            assert twin.within(twin.rounded(a32, kind), d, kind), (order, kind)
        shares[order] = twin.worst(a32, d)
    print(name, {k: "%.3g" % v for k, v in shares.items()})
    assert max(shares.values()) <= 1


@pytest.mark.parametrize("name", list(twin.EXACT_CASES))
def test_exact_sum_cases_are_order_independent(name):
    d = twin.reference(name)
    assert np.isfinite(d["a64"]).all() and (d["a64"] > 0).any() and (d["a64"] < 0).any()
    assert d["a32"].astype(np.float64).tobytes() == d["a64"].tobytes()             # the float32 evaluation IS a64
    for order in twin.ORDERS[1:]:
        a32 = twin.stage(*(d[k] for k in twin.KEYS), d["slope"], up=d["up"], order=order, seed=11)["a32"]
        assert twin.same_bits(a32, d["a32"]), order


# ------------------------------------------------------------------------------------------------ 4. mutations
MUTATIONS = {
    "truncation_instead_of_nearest_even": (dict(rounding="truncate"), ("odd_chunks", "exact_up", "exact_same")),
    "an_unrounded_weight": (dict(round_w=False), ("odd_chunks", "stage_2s", "c17")),
    "an_unrounded_z": (dict(round_z=False), ("odd_chunks", "stage_2s", "exact_same")),
    "skip_channels_first": (dict(channels="skip_a"), ("straddle", "exact_up", "stage_2s")),
    "align_corners_false": (dict(coords="half_pixel"), ("straddle", "exact_up", "stage_2s")),
    "a_replicated_ring": (dict(ring="edge"), ("c33", "exact_same", "exact_up")),
    "an_upsample_where_the_same_resolution_was_meant": (dict(crop=True), ("no_skip_same_res", "exact_same")),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_rule_stated_wrongly_leaves_the_bound_or_the_exact_bits(mutation):
    kw, names = MUTATIONS[mutation]
    left = {}
    for name in names:
        d = twin.reference(name)
        assert twin.within(d["a32"], d)                                             # the rule stated rightly does not
        wrong = twin.stage(*(d[k] for k in twin.KEYS), d["slope"], up=d["up"], order="ascending", **kw)["a32"]
        left[name] = not twin.same_bits(wrong, d["a32"]) if name in twin.EXACT_CASES else not twin.within(wrong, d)
    print(mutation, left)
    assert any(left.values())


# ------------------------------------------------------------------------------------------------ 5. the built kernels
LDS_BYTES = {1: 16 * (340 * 5 + 9 * 4 * 36), 2: 16 * (340 * 5 + 9 * 4 * 68), 4: 16 * (340 * 3 + 9 * 2 * 136)}   # StageBf16Lds<N1>::bytes


def test_the_kernels_spill_nothing_and_take_the_lds_the_host_states():
    """Every built instantiation of k_head_stage_bf16, read from the metadata of the translation unit compiled with the shipped
    flags (tests/test_host.py's listing): no spilled VGPR, no scratch, at most 256 VGPRs -- two workgroups per CU --, no static
    LDS beside the dynamic LDS of the host's expression, which the source states per N1 and of which two fit a CU's 160 KiB."""
    from tests.test_host import _kernel_isa, _meta, _vote_isa
    asm = _vote_isa()
    names = set(re.findall(r"^(_ZN\S*k_head_stage_bf16\S*):", asm, re.M))
    assert len(names) == 6
    with open(os.path.join(ROOT, "clean-pvnet_amd", "csrc", "head_stage_bf16.hpp")) as f:
        src = f.read()
    for n1 in (1, 2, 4):
        assert 2 * LDS_BYTES[n1] <= 160 * 1024 and "= %d bytes" % LDS_BYTES[n1] in src
        for up in (0, 1):
            body, meta = _kernel_isa(asm, "k_head_stage_bf16ILi%dELb%dE" % (n1, up))
            assert _meta(meta, "vgpr_spill_count") == 0 and _meta(meta, "private_segment_fixed_size") == 0, (n1, up)
            assert _meta(meta, "vgpr_count") <= 256 and _meta(meta, "group_segment_fixed_size") == 0, (n1, up)
            assert body.count("v_mfma_f32_32x32x16_bf16") >= 9 * 2 * n1 and "v_mfma_f32_32x32x2_f32" not in body
    assert "static constexpr size_t bytes = 16 * (size_t)(halo_slots + w_slots);" in src
    assert src.count("StageBf16Lds<N1>::bytes") == 1 and "L::halo_slots" in src     # the launch and the kernel take the one expression
