"""What the ``ransac_voting`` extension module refuses, and in which words: every public function on one tiny problem
(B = 2, H = 16, W = 24, K = 3, 8 hypotheses) with ONE argument wrong at a time.  The fragments are those of the shim
(csrc/ransac_voting_ext.cpp) and, for the three-class seg, of the library behind it; every refusal comes before the first launch.
``test_gpu_parity.py::test_extension_rejects_bad_inputs`` holds the device / contiguity / dtype checks of the reference's four functions.

Also here: the first test of ``count_kernel_ms_in_pipeline``, the event pair around the inlier-count launch.
"""
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W, K, HN, HN_EST = 2, 16, 24, 3, 8, 16
HN_RANGE = "hypothesis count must be in [1, 2^24)"
SEG_SHAPE = "seg must be [b,c,h,w] matching vertex [b,h,w,vn,2]"


@pytest.fixture(scope="module")
def ext(pkg):
    from clean_pvnet_amd import ransac_voting
    return ransac_voting


@pytest.fixture(scope="module")
def good(gpu):
    """One valid value of every argument; the tests swap a single one out and never write to these."""
    g = torch.Generator().manual_seed(5)
    mask = torch.zeros(B, H, W, dtype=torch.int64)
    mask[:, 3:13, 4:20] = 1
    t = dict(mask=mask,
             vertex=torch.randn(B, H, W, K, 2, generator=g),
             seg=torch.stack([1.0 - mask, mask.float()], 1),
             idxs=torch.randint(0, 160, (B, HN, K, 2), generator=g, dtype=torch.int32),
             idxs_est=torch.randint(0, 160, (B, HN_EST, K, 2), generator=g, dtype=torch.int32),
             selection=torch.rand(B, H, W, generator=g),
             mean=torch.rand(B, K, 2, generator=g) * 16,
             status=torch.zeros(B, dtype=torch.int32),
             out=torch.zeros(B, K, 2),
             ws=torch.zeros(64, dtype=torch.uint8))
    return {k: v.to(gpu) for k, v in t.items()}


def _calls(ext):
    """name -> function of the argument dict: every public call that takes a batch, with the module's own argument order."""
    R = ext.SINGULAR_REFERENCE
    return {
        "ransac_voting_v3": lambda a: ext.ransac_voting_v3(a["mask"], a["vertex"], a["hn"], 0.99, 5, 30000, a["idxs"], a["selection"], 0, R,
                                                           status=a["status"], cap=a["cap"], out=a["out"]),
        "decode_keypoint_v3": lambda a: ext.decode_keypoint_v3(a["seg"], a["vertex"], a["hn"], 0.99, 5, 30000, a["idxs"], a["selection"], 0, R),
        "decode_keypoint_un_pnp": lambda a: ext.decode_keypoint_un_pnp(a["seg"], a["vertex"], a["hn"], a["hyp_est"], 0.99, 5, 30000, a["idxs"],
                                                                       a["idxs_est"], a["selection"], 0, R),
        "estimate_voting_distribution": lambda a: ext.estimate_voting_distribution(a["mask"], a["vertex"], a["mean"], a["hn"], 0.99, 5, 30000,
                                                                                   a["idxs"], a["selection"], 0, False),
        "rerun_count_kernel": lambda a: ext.rerun_count_kernel(a["mask"], a["vertex"], a["hn"], 0.99, 5, 30000, a["ws"], True, cap=a["cap"]),
        "stage_hint": lambda a: ext.stage_hint(a["mask"], a["vertex"], a["hn"]),
        "stage_ms_in_pipeline": lambda a: ext.stage_ms_in_pipeline([a["mask"]], [a["vertex"]], a["hn"], 0.99, 5, 30000, 0, 2),
        "stage_ms_in_pipeline[segs]": lambda a: ext.stage_ms_in_pipeline([], [a["vertex"]], a["hn"], 0.99, 5, 30000, 0, 2, segs=[a["seg"]]),
        "stage_ms_in_pipeline[means]": lambda a: ext.stage_ms_in_pipeline([a["mask"]], [a["vertex"]], a["hn"], 0.99, 5, 30000, 0, 2, estimate=True,
                                                                          means=[a["mean"]]),
        "count_kernel_ms_in_pipeline": lambda a: ext.count_kernel_ms_in_pipeline([a["mask"]], [a["vertex"]], a["hn"], 0.99, 5, 30000, 0, 2),
    }


MASK_VERTEX = ["ransac_voting_v3", "estimate_voting_distribution", "rerun_count_kernel", "stage_hint", "stage_ms_in_pipeline",
               "count_kernel_ms_in_pipeline"]
SEG = ["decode_keypoint_v3", "decode_keypoint_un_pnp"]
DRAWS = ["ransac_voting_v3", "decode_keypoint_v3", "decode_keypoint_un_pnp", "estimate_voting_distribution"]
# the timing aid words its seg refusal like the two public calls or, before it shared their set-up, around the same core
SEG_SHAPE_AID = "[b,c,h,w] matching vertex"

# (what is wrong, argument, its bad value from the good ones, {call: message fragment})
CASES = [
    ("vertex of rank 4", "vertex", lambda g: g["vertex"][..., 0].contiguous(),
     {**{c: "vertex must be [b,h,w,vn,2]" for c in MASK_VERTEX}, **{c: SEG_SHAPE for c in SEG}}),
    ("mask of another height", "mask", lambda g: g["mask"][:, :H - 1].contiguous(), {c: "mask must be [b,h,w] matching vertex" for c in MASK_VERTEX}),
    ("hn = 0", "hn", lambda g: 0, {c: HN_RANGE for c in MASK_VERTEX + SEG + ["stage_ms_in_pipeline[segs]"]}),
    ("idxs on the CPU", "idxs", lambda g: g["idxs"].cpu(), {c: "idxs must be a CUDA tensor" for c in DRAWS}),
    ("idxs as int64", "idxs", lambda g: g["idxs"].long(), {c: "idxs must have dtype Int, got Long" for c in DRAWS}),
    ("idxs of a wrong shape", "idxs", lambda g: g["idxs"][:, :HN - 1].contiguous(), {c: "idxs must be [b,hn,vn,2] = [2,8,3,2]" for c in DRAWS}),
    ("idxs_est on the CPU", "idxs_est", lambda g: g["idxs_est"].cpu(), {"decode_keypoint_un_pnp": "idxs must be a CUDA tensor"}),
    ("idxs_est as int64", "idxs_est", lambda g: g["idxs_est"].long(), {"decode_keypoint_un_pnp": "idxs must have dtype Int, got Long"}),
    ("idxs_est of a wrong shape", "idxs_est", lambda g: g["idxs_est"][:, :, :K - 1].contiguous(),
     {"decode_keypoint_un_pnp": "idxs must be [b,hn,vn,2] = [2,16,3,2]"}),
    ("selection of a wrong shape", "selection", lambda g: g["selection"][:, :, :W - 1].contiguous(), {c: "selection must be [b,h,w]" for c in DRAWS}),
    ("status of a wrong shape", "status", lambda g: g["status"][:1].contiguous(), {"ransac_voting_v3": "status must be [b]"}),
    ("cap = 0", "cap", lambda g: 0, {"ransac_voting_v3": "cap must be in [1, h*w]", "rerun_count_kernel": "cap must be in [1, H*W]"}),
    ("cap = H*W + 1", "cap", lambda g: H * W + 1, {"ransac_voting_v3": "cap must be in [1, h*w]", "rerun_count_kernel": "cap must be in [1, H*W]"}),
    ("out of a wrong shape", "out", lambda g: g["out"][:, :K - 1].contiguous(), {"ransac_voting_v3": "out must be [b,vn,2] = [2,3,2]"}),
    ("mean of a wrong shape", "mean", lambda g: g["mean"][:1].contiguous(),
     {"estimate_voting_distribution": "mean must be [b,vn,2]", "stage_ms_in_pipeline[means]": "mean must be [b,vn,2]"}),
    ("seg of rank 3", "seg", lambda g: g["seg"][:, 0].contiguous(), {**{c: SEG_SHAPE for c in SEG}, "stage_ms_in_pipeline[segs]": SEG_SHAPE_AID}),
    ("seg of another width", "seg", lambda g: g["seg"][..., :W - 1].contiguous(),
     {**{c: SEG_SHAPE for c in SEG}, "stage_ms_in_pipeline[segs]": SEG_SHAPE_AID}),
    ("seg as float64", "seg", lambda g: g["seg"].double(),
     {c: "seg must be float32, float16 or bfloat16, got Double" for c in SEG + ["stage_ms_in_pipeline[segs]"]}),
    ("hyp_est = 0", "hyp_est", lambda g: 0, {"decode_keypoint_un_pnp": "hypothesis count of the estimate must be in [1, 2^24)"}),
    ("a three-class seg", "seg", lambda g: torch.cat([g["seg"], g["seg"][:, :1]], 1).contiguous(),
     {"decode_keypoint_un_pnp": "the fused un_pnp pass needs seg_classes == 2"}),
]


@pytest.mark.parametrize("what,arg,bad,expect", CASES, ids=[c[0] for c in CASES])
def test_one_wrong_argument_is_refused_in_the_shims_words(ext, good, what, arg, bad, expect):
    calls = _calls(ext)
    args = {**good, "hn": HN, "hyp_est": HN_EST, "cap": None, arg: bad(good)}
    for name, fragment in expect.items():
        with pytest.raises(RuntimeError, match=re.escape(fragment)):
            calls[name](args)
    torch.cuda.synchronize()


def test_count_inliers_refuses_vanishing_point_hypotheses(ext, gpu):
    d, c = torch.zeros(10, K, 2, device=gpu), torch.zeros(10, 2, device=gpu)
    with pytest.raises(RuntimeError, match=re.escape("hypo_pts must be [hn,vn,2]")):
        ext.count_inliers(d, c, torch.zeros(HN, K, 3, device=gpu), 0.99)
    with pytest.raises(RuntimeError, match=re.escape("direct must be [tn,vn,2]")):
        ext.count_inliers(torch.zeros(10, K, 3, device=gpu), c, torch.zeros(HN, K, 2, device=gpu), 0.99)
    with pytest.raises(RuntimeError, match=re.escape("coords must be [tn,2]")):
        ext.count_inliers(d, torch.zeros(9, 2, device=gpu), torch.zeros(HN, K, 2, device=gpu), 0.99)


def test_the_good_arguments_are_accepted(ext, good):
    """The other half of every case above: with nothing swapped out the same calls go through (the workspace of rerun_count_kernel
    is the producing call's)."""
    calls = _calls(ext)
    ws = ext.ransac_voting_v3(good["mask"], good["vertex"], HN, 0.99, 5, 30000, None, None, 0, ext.SINGULAR_REFERENCE)[3]
    args = {**good, "hn": HN, "hyp_est": HN_EST, "cap": None, "ws": ws}
    for call in calls.values():
        call(args)
    torch.cuda.synchronize()


def test_count_kernel_ms_in_pipeline_returns_one_duration_per_call(ext, good, gpu):
    one = ext.count_kernel_ms_in_pipeline([good["mask"]], [good["vertex"]], HN, 0.99, 5, 30000, 0, 3)
    assert len(one) == 3 and all(math.isfinite(t) and t >= 0 for t in one)
    m2, v2 = good["mask"].flip(0).contiguous(), good["vertex"].flip(0).contiguous()
    two = ext.count_kernel_ms_in_pipeline([good["mask"], m2], [good["vertex"], v2], HN, 0.99, 5, 30000, 0, 3)
    assert len(two) == 3 and all(math.isfinite(t) and t >= 0 for t in two)
