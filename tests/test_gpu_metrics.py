"""The batched pose scores on the MI355X (include/pvnet_metrics.h, clean_pvnet_amd.metrics): every fixture made by the
reference's own evaluator, the ADD-S search bit-exact against the oracle for several slab counts, determinism and batch
independence, the mask counts, and network output -> pose -> score with no host synchronisation.  Bounds and their
derivation: tests/metrics_twin.py."""
import os

import numpy as np
import pytest

from oracle import pnp_oracle as po
from tests import metrics_twin as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VALUES = ("add", "adds", "proj2d", "trans_cm", "ang_deg")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _t(gpu, a, dtype=None):
    import torch
    return torch.tensor(np.asarray(a), dtype=dtype, device=gpu)


def _same_bits(a, b):
    import torch
    if a.dtype.is_floating_point:
        a, b = torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)
    return torch.equal(a, b)


def _poses(b, seed):
    """b (prediction, ground truth) pairs with errors from rounding-noise size to a quarter turn."""
    rng = np.random.RandomState(seed)
    Pp, Pg = [], []
    for i in range(b):
        G = twin.pose(rng.uniform(-1, 1, 3), [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.0)])
        e = (0.0, 1e-4, 0.003, 0.03, 0.3, 1.5)[i % 6]
        dw, dt = rng.randn(3), rng.randn(3)
        P = np.concatenate([twin.rodrigues(e * dw / np.linalg.norm(dw)) @ G[:, :3], (G[:, 3] + 0.1 * e * dt).reshape(3, 1)], 1)
        Pp.append(P)
        Pg.append(G)
    return np.stack(Pp), np.stack(Pg)


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("name", ["metrics_n5841", "metrics_n777"])
def test_fixture_cases_batched(oracle, pkg, gpu, name):
    import torch
    from clean_pvnet_amd.metrics import PoseEvaluator, pose_metrics
    c = load(name)
    n, diameter = int(c["n"]), float(c["diameter"])
    model = twin.cloud(n, int(c["cloud_seed"]))
    Pp, Pg, K, md = _t(gpu, c["pose_pred"]), _t(gpu, c["pose_gt"]), _t(gpu, c["K"]), _t(gpu, model)
    nb = len(c["names"])
    bad = [i for i in range(nb) if not np.isfinite(c["pose_pred"][i]).all()]
    assert len(bad) == 1
    for slabs in (0, 1, 5):
        out = pose_metrics(Pp, Pg, md, K, symmetric=True, return_idx=True, slabs=slabs)
        idx = out["adds_idx"].cpu().numpy()
        got = {k: out[k].cpu().numpy() for k in VALUES}
        assert idx.dtype == np.int32 and idx.shape == (nb, n)
        for i, case in enumerate(c["names"]):
            if i in bad:
                assert all(np.isnan(got[k][i]) for k in VALUES) and not idx[i].any()
                continue
            np.testing.assert_array_equal(idx[i], c["adds_idx"][i], err_msg="%s slabs=%d" % (case, slabs))
            want = twin.pose_metrics(c["pose_pred"][i], c["pose_gt"][i], model, c["K"], search=oracle.find_nearest_point_idx)
            want.update({k: float(c[k][i]) for k in VALUES})            # the values the reference compared
            twin.assert_close({k: got[k][i] for k in VALUES}, want, n, what="%s/%s/slabs=%d" % (name, case, slabs))
    for sym, key in ((False, "hit_add"), (True, "hit_adds")):
        ev = PoseEvaluator(model, diameter, symmetric=sym, device=gpu)
        hits = ev.evaluate({"pose": Pp}, Pg, K)
        np.testing.assert_array_equal(hits["add"].cpu().numpy(), c[key])
        np.testing.assert_array_equal(hits["proj2d"].cpu().numpy(), c["hit_proj2d"])
        np.testing.assert_array_equal(hits["cmd5"].cpu().numpy(), c["hit_cmd5"])
        assert not any(bool(hits[k][bad[0]]) for k in hits)
        assert torch.isnan(ev.last["values"]["add"][bad[0]])
        s = ev.summarize()
        assert s["add"] == np.mean(c[key]) and s["proj2d"] == np.mean(c["hit_proj2d"]) and s["cmd5"] == np.mean(c["hit_cmd5"])
        assert np.isnan(s["ap"])                                         # no mask was given: np.mean([])
        assert all(np.isnan(v) for v in ev.summarize().values())         # summarize() starts the counters again


def test_evaluator_counts_over_calls_with_masks(pkg, gpu):
    from clean_pvnet_amd.metrics import PoseEvaluator
    c, m = load("metrics_n777"), load("metrics_masks")
    model = twin.cloud(int(c["n"]), int(c["cloud_seed"]))
    nm = len(m["hit_ap"])
    ev = PoseEvaluator(model, float(c["diameter"]), device=gpu)
    Pp, Pg, K = _t(gpu, c["pose_pred"]), _t(gpu, c["pose_gt"]), _t(gpu, c["K"])
    mp, mg = _t(gpu, m["mask_pred"].astype(np.int64)), _t(gpu, m["mask_gt"].astype(np.int64))
    h = ev.evaluate({"pose": Pp[:nm], "mask": mp}, Pg[:nm], K, mask_gt=mg)
    np.testing.assert_array_equal(h["ap"].cpu().numpy(), m["hit_ap"])
    ev.evaluate({"pose": Pp[nm:]}, Pg[nm:], K)                           # a second batch, without masks
    s = ev.summarize()
    assert s == {"proj2d": np.mean(c["hit_proj2d"]), "add": np.mean(c["hit_add"]), "cmd5": np.mean(c["hit_cmd5"]),
                 "ap": np.mean(m["hit_ap"])}


# ------------------------------------------------------------------------------------------------ 2. the search, bit-exact
@pytest.mark.parametrize("b", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 255, 777, 4097, 5841])
def test_adds_search_bit_exact_for_every_slab_count(oracle, pkg, gpu, n, b):
    from clean_pvnet_amd.metrics import adds_slabs, pose_metrics
    model = twin.cloud(n, 100 + n)
    Pp, Pg = _poses(b, 7 * n + b)
    want = np.stack([oracle.find_nearest_point_idx(twin.transform(model, Pp[i]).astype(np.float32),
                                                   twin.transform(model, Pg[i]).astype(np.float32)) for i in range(b)])
    if n > 10:
        assert (want[0] == np.minimum(want[0], np.arange(n))).all() and want[0][7] == 3    # identical poses: ties -> lower index
    tp, tg, md, K = _t(gpu, Pp), _t(gpu, Pg), _t(gpu, model), _t(gpu, twin.LINEMOD_K)
    values = None
    for slabs in (0, 1, 7, 64, 100):                                    # 0 = the library's choice; 7 divides none of the sizes
        out = pose_metrics(tp, tg, md, K, symmetric=True, return_idx=True, slabs=slabs)
        np.testing.assert_array_equal(out["adds_idx"].cpu().numpy(), want, err_msg="n=%d b=%d slabs=%d (auto=%d)" %
                                      (n, b, slabs, adds_slabs(b, n)))
        cur = out["adds"].clone()
        assert values is None or _same_bits(cur, values), slabs          # and the value does not depend on the split
        values = cur
    i = b - 1
    ref = twin.pose_metrics(Pp[i], Pg[i], model, twin.LINEMOD_K, search=oracle.find_nearest_point_idx)
    twin.assert_close({k: float(out[k][i]) for k in VALUES}, ref, n, what="n=%d b=%d image %d" % (n, b, i))


# ------------------------------------------------------------------------------------------------ 3. determinism, layouts
def test_determinism_batch_independence_and_layouts(oracle, pkg, gpu):
    import torch
    from clean_pvnet_amd.metrics import pose_metrics
    n, b = 5841, 64
    model = twin.cloud(n, 21)
    Pp, Pg = _poses(b, 22)
    Pp[5, 1, 2] = np.inf                                                 # one image without a pose
    tp, tg, md, K = _t(gpu, Pp), _t(gpu, Pg), _t(gpu, model), _t(gpu, twin.LINEMOD_K)
    keys = VALUES + ("adds_idx",)
    a = pose_metrics(tp, tg, md, K, symmetric=True, return_idx=True)
    a2 = pose_metrics(tp, tg, md, K, symmetric=True, return_idx=True)
    for k in keys:
        assert _same_bits(a[k], a2[k]), k                                # two identical calls: the same bits
    assert all(bool(torch.isnan(a[k][5])) for k in VALUES) and not bool(a["adds_idx"][5].any())
    for i in (0, 4, 5, 6, 63):                                           # image i of the batch == the batch of image i alone
        one = pose_metrics(tp[i:i + 1], tg[i:i + 1], md, K, symmetric=True, return_idx=True)
        for k in keys:
            assert _same_bits(a[k][i:i + 1], one[k]), (i, k)
    # a camera per image == per-image calls
    Kb = torch.stack([K * torch.tensor([[1 + 0.01 * i] * 3, [1 + 0.01 * i] * 3, [1.0] * 3], dtype=torch.float64, device=gpu)
                      for i in range(b)])
    kb = pose_metrics(tp, tg, md, Kb, symmetric=True)
    for i in (0, 9, 63):
        one = pose_metrics(tp[i:i + 1], tg[i:i + 1], md, Kb[i], symmetric=True)
        for k in VALUES:
            assert _same_bits(kb[k][i:i + 1], one[k]), (i, k)
    assert not _same_bits(kb["proj2d"][9:10], a["proj2d"][9:10]) and _same_bits(kb["add"], a["add"])
    # mixed flags: NaN exactly where unset, everything else unchanged
    flags = torch.arange(b, device=gpu) % 3 == 0
    mixed = pose_metrics(tp, tg, md, K, symmetric=flags, return_idx=True)
    expect = torch.where(flags, a["adds"], torch.full_like(a["adds"], float("nan")))
    assert _same_bits(mixed["adds"], expect)
    assert _same_bits(mixed["adds_idx"], a["adds_idx"] * flags[:, None].to(torch.int32))
    none = pose_metrics(tp, tg, md, K, return_idx=True)
    assert bool(torch.isnan(none["adds"]).all()) and not bool(none["adds_idx"].any())
    for k in ("add", "proj2d", "trans_cm", "ang_deg"):
        assert _same_bits(mixed[k], a[k]) and _same_bits(none[k], a[k]), k
    # an empty batch
    e = pose_metrics(tp[:0], tg[:0], md, K, symmetric=True, return_idx=True)
    assert all(e[k].shape == (0,) and e[k].dtype == torch.float64 for k in VALUES) and e["adds_idx"].shape == (0, n)


# ------------------------------------------------------------------------------------------------ 4. masks
def test_mask_counts_dtypes_strides_and_empty_union(pkg, gpu):
    import torch
    from clean_pvnet_amd.metrics import mask_counts, mask_iou
    c = load("metrics_masks")
    p, g = c["mask_pred"].astype(np.int64), c["mask_gt"]
    for dt in (torch.int64, torch.uint8, torch.bool):
        inter, union = mask_counts(_t(gpu, p), _t(gpu, g).to(dt))
        assert inter.dtype == torch.int64
        np.testing.assert_array_equal(inter.cpu().numpy(), c["inter"])
        np.testing.assert_array_equal(union.cpu().numpy(), c["union"])
    iou = mask_iou(_t(gpu, p), _t(gpu, g)).cpu().numpy()
    assert iou.dtype == np.float64 and np.isnan(iou[-1])                 # 0 / 0, as numpy gives; a miss
    np.testing.assert_array_equal(iou > 0.7, c["hit_ap"])
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(iou, c["inter"] / c["union"])
    # image size of the evaluators, a batch-strided slice of a larger batch, values other than 0 / 1
    rng = np.random.RandomState(8)
    big_p = rng.randint(0, 4, (10, 480, 640)).astype(np.int64)
    big_g = rng.randint(0, 3, (10, 480, 640)).astype(np.uint8)
    tp, tg = _t(gpu, big_p)[1::2], _t(gpu, big_g)[::2]
    assert not tp.is_contiguous()
    inter, union = mask_counts(tp, tg)
    np.testing.assert_array_equal(inter.cpu().numpy(), (big_p[1::2] & big_g[::2]).sum((1, 2)))
    np.testing.assert_array_equal(union.cpu().numpy(), (big_p[1::2] | big_g[::2]).sum((1, 2)))
    e, _ = mask_counts(tp[:0], tg[:0])
    assert e.shape == (0,)


# ------------------------------------------------------------------------------------------------ 5. end to end, no sync
def _rendered_fields(gpu):
    """Synthetic network output as in test_gpu_pose._rendered_fields."""
    import torch
    B, H, W, K = 4, 240, 320, 9
    rng = np.random.RandomState(5)
    P = rng.uniform(-0.05, 0.05, (K, 3))
    Kc = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1.0]])
    rts = np.stack([np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-0.03, 0.03, 2), rng.uniform(0.5, 0.7, 1)]) for _ in range(B)])
    kpts = []
    for rt in rts:
        X = np.array([po.angle_axis_rotate_point(rt[:3], p) for p in P]) + rt[3:]
        kpts.append(np.stack([Kc[0, 0] * X[:, 0] / X[:, 2] + Kc[0, 2], Kc[1, 1] * X[:, 1] / X[:, 2] + Kc[1, 2]], 1))
    kpts = torch.tensor(np.stack(kpts), dtype=torch.float32)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    x = torch.zeros(B, 2 + 2 * K, H, W)
    for b in range(B):
        c = kpts[b].mean(0)
        m = ((xs - c[0]) ** 2 + (ys - c[1]) ** 2) <= 30.0 ** 2
        x[b, 0] = 1.0
        x[b, 1] = torch.where(m, torch.tensor(4.0), torch.tensor(-4.0))
        g = torch.Generator().manual_seed(b)
        for k in range(K):
            dx, dy = kpts[b, k, 0] - xs, kpts[b, k, 1] - ys
            n = torch.sqrt(dx * dx + dy * dy).clamp(min=1e-3)
            x[b, 2 + 2 * k] = dx / n + 0.03 * torch.randn(H, W, generator=g)
            x[b, 3 + 2 * k] = dy / n + 0.03 * torch.randn(H, W, generator=g)
    return x.to(gpu), P, Kc, rts


@pytest.mark.parametrize("symmetric", [False, True])
def test_network_output_to_score_with_no_host_sync(oracle, pkg, gpu, symmetric):
    import torch
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.metrics import PoseEvaluator
    from clean_pvnet_amd.pose import solve_pose
    x, P, Kc, rts = _rendered_fields(gpu)
    n, diameter = 777, 0.15
    model = twin.cloud(n, 33)
    gt = np.stack([np.concatenate([po.rodrigues(rt[:3]), rt[3:].reshape(3, 1)], 1) for rt in rts])
    Pt, Kt, Gt = _t(gpu, P), _t(gpu, Kc), _t(gpu, gt)
    ev = PoseEvaluator(model, diameter, symmetric=symmetric, device=gpu)
    seen = {}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for un_pnp in (True, False):
            o = {"seg": x[:, :2], "vertex": x[:, 2:]}
            decode_keypoint(o, un_pnp=un_pnp, weights=un_pnp, seed=3)
            solve_pose(o, Pt, Kt, un_pnp=un_pnp)
            ev.evaluate(o, Gt, Kt, mask_gt=o["mask"])
            seen[un_pnp] = (o["pose"], ev.last)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = ev.summarize()                                                   # the one read-back: 8 images
    print("summarize:", s)
    for un_pnp, (pose, last) in seen.items():
        pose = pose.cpu().numpy()
        vals = {k: last["values"][k].cpu().numpy() for k in VALUES}
        for b in range(len(rts)):
            want = twin.pose_metrics(pose[b], gt[b], model, Kc, symmetric=symmetric, search=oracle.find_nearest_point_idx)
            twin.assert_close({k: vals[k][b] for k in VALUES}, want, n, what="un_pnp=%s image %d" % (un_pnp, b))
            h = twin.hits(want, diameter, symmetric)
            assert {k: bool(last["hits"][k][b]) for k in h} == h
    assert s["add"] == 1.0 and s["proj2d"] == 1.0 and s["ap"] == 1.0, s
