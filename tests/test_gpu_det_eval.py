"""Detector evaluation on the MI355X (clean_pvnet_amd.det_eval): the box IoU, every stage's output and the evaluator's results
equal the numpy twin (tests/det_eval_twin.py, itself held to the reference's ``Evaluator`` and ``COCOeval`` in
tests/test_det_eval.py) bit for bit, for any split of the images into calls and for a second epoch; the error flag raises; and
``crop.decode_ct_hm``'s output runs through as it lies on the device.  Three tests feed what no fixture can: the rounding at the
exact ties of the second decimal against Python's own formatting, the accumulation on made-up stage outputs whose categories end
on and around the 64-lane chunks, and ``num`` as int32 and outside ``[0, K]``."""
import numpy as np
import pytest

from tests import det_eval_twin as twin

pytestmark = pytest.mark.gpu

FIXTURES = tuple(twin.SCENARIOS)
RESULTS = ("precision", "recall", "scores")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _feed(ev, s, splits, gpu):
    import torch
    det = torch.from_numpy(s["detection"]).to(gpu)
    for idx in splits:
        idx = list(idx)
        num = None if s["num"] is None else torch.from_numpy(np.asarray(s["num"])[idx]).to(gpu)
        ev.evaluate(det[idx], [s["img_ids"][b] for b in idx], s["center"][idx], s["scale"][idx], s["inp_hw"], num=num)


def test_box_iou_equals_the_twin(pkg, gpu):
    import torch
    from clean_pvnet_amd import det_eval
    rng = np.random.default_rng(3)
    gt = np.array([[0, 0, 2, 1], [10, 10, 40, 40], [10, 10, 40, 40], [3.25, 7.5, 11.13, 9.87], [50, 50, 0, 10]], np.float64)
    crowd = np.array([0, 0, 1, 0, 0], np.int32)
    dt = np.concatenate([np.array([[0, 0, 1, 1],            # exactly 0.5 against the first
                                   [2, 0, 5, 5],            # touching: w == 0
                                   [100, 100, 5, 5],        # disjoint
                                   [12, 12, 20, 20],        # nested; the crowd divides by the detection's area
                                   [10, 10, 40, 40],        # identical
                                   [0, 0, 0, 0]], np.float64),   # empty against empty: 0 / 0 only where they overlap, never here
                         np.round(rng.uniform(0, 45, (59, 4)), 2)])
    got = det_eval.box_iou(torch.from_numpy(dt).to(gpu), torch.from_numpy(gt).to(gpu), torch.from_numpy(crowd).to(gpu)).cpu().numpy()
    want = twin.box_iou(dt, gt, crowd)
    assert got[0, 0] == 0.5 and got[1, 0] == 0 and got[2].max() == 0 and got[3, 2] == 1.0 and got[4, 1] == 1.0
    assert _same(got, want)
    assert det_eval.box_iou(torch.zeros(0, 4, dtype=torch.float64, device=gpu), torch.from_numpy(gt).to(gpu),
                            torch.from_numpy(crowd).to(gpu)).shape == (0, 5)


@pytest.mark.parametrize("name", FIXTURES)
def test_stage_outputs_equal_the_twin(pkg, gpu, name):
    from clean_pvnet_amd import det_eval
    s, want = twin.fixture_with_twin(name)
    ev = det_eval.DetEvaluator(s)
    _feed(ev, s, [range(len(s["img_ids"]))], gpu)
    mapped = {k: v.cpu().numpy() for k, v in ev.last["mapped"].items()}
    for k in ("box", "score", "area", "n", "cat"):
        assert _same(mapped[k], want["mapped"][0][k]), k                                   # every row, the unused ones included
    assert _same(ev.last["keys"].cpu().numpy(), want["keys"][0])
    assert _same(ev.last["words"].cpu().numpy().view(np.uint32), want["words"][0])
    ev.summarize()
    assert _same(ev.npig.astype(np.int32), want["npig"])
    keys_sorted, perm = ev.order["keys"].cpu().numpy(), ev.order["perm"].cpu().numpy()
    assert _same(keys_sorted, want["keys_sorted"])
    live = keys_sorted != twin.SENTINEL                                                    # the rows left out share one key
    assert _same(perm[live], want["perm"][live]) and sorted(perm[~live]) == sorted(want["perm"][~live])
    for k in RESULTS:
        assert _same(ev.eval[k], want[k]), k


@pytest.mark.parametrize("name", FIXTURES)
def test_evaluator_is_the_reference_for_any_split_and_epoch(pkg, gpu, name):
    from clean_pvnet_amd import det_eval
    s, want = twin.fixture_with_twin(name)
    B = len(s["img_ids"])
    ev = det_eval.DetEvaluator(s)
    for epoch, splits in enumerate(([range(B)], [[b] for b in range(B)], [[0, 1, 2], [3], range(4, B)], [range(B)])):
        _feed(ev, s, splits, gpu)
        ret = ev.summarize()
        for k in RESULTS:
            assert _same(ev.eval[k], want[k]) and _same(ev.eval[k], s["ref_" + k]), (epoch, k)
        assert _same(ev.stats, s["ref_stats"]) and ret == {"ap": s["ref_stats"][0]}
    assert len(ev.aps) == 4 and len(set(ev.aps)) == 1


def test_error_flag_raises_on_a_nan_score(pkg, gpu):
    import torch
    from clean_pvnet_amd import det_eval
    s, want = twin.fixture_with_twin("det_eval_random")
    ev = det_eval.DetEvaluator(s)
    bad = dict(s, detection=s["detection"].copy())
    bad["detection"][2, 5, 4] = np.nan
    _feed(ev, bad, [range(len(s["img_ids"]))], gpu)
    with pytest.raises(RuntimeError, match="not finite"):
        ev.summarize()
    big = dict(s, detection=s["detection"].copy())
    big["detection"][1, 0, 4] = 90000.0                                                    # n = 9e6 does not fit 24 signed bits
    _feed(ev, big, [range(len(s["img_ids"]))], gpu)
    with pytest.raises(RuntimeError, match="24-bit"):
        ev.summarize()
    _feed(ev, s, [range(len(s["img_ids"]))], gpu)                                          # the state started again
    ev.summarize()
    assert _same(ev.eval["precision"], want["precision"])
    with pytest.raises(ValueError, match="twice"):
        _feed(ev, s, [[0], [0]], gpu)


def test_decoded_heat_maps_run_through(pkg, gpu):
    import torch
    from clean_pvnet_amd import crop, det_eval
    rng = np.random.default_rng(11)
    B, C, H, W, K = 3, 4, 34, 45, 20
    hm = rng.uniform(0, 0.3, (B, C, H, W)).astype(np.float32)
    for b in range(B):
        for _ in range(12 if b else 0):                                                    # the first image has no peak above zero
            hm[b, rng.integers(C), rng.integers(H), rng.integers(W)] = rng.uniform(0.4, 1.0)
    hm[0] = 0
    wh = rng.uniform(2, 14, (B, 2, H, W)).astype(np.float32)
    _, det, count = crop.decode_ct_hm(torch.from_numpy(hm).to(gpu), torch.from_numpy(wh).to(gpu), K=K)
    det_h, count_h = det.cpu().numpy(), count.cpu().numpy()
    assert count_h[0] == 0 and (count_h[1:] == K).all()
    ids, inp_hw = [31, 7, 19], (4 * H, 4 * W)
    center = np.array([[360, 270], [350.5, 260], [372, 281.25]], np.float32)
    scale = np.array([[720, 720], [655, 655], [810.5, 810.5]], np.float32)
    cat_ids = [4, 2, 9, 6]
    g0 = twin.prepare_gt(dict(image_id=np.array(ids), category_id=np.array(cat_ids), ann_image_id=np.zeros(0, np.int64),
                              ann_category_id=np.zeros(0, np.int64), ann_bbox=np.zeros((0, 4)), ann_area=np.zeros(0), ann_iscrowd=np.zeros(0, np.int32)))
    boxes = twin.map_rows(det_h, twin.make_block(g0["images"], ids, center, scale, inp_hw), g0["label_to_cat"])[0]["box"].reshape(B, K, 4)
    ann = [(ids[b], cat_ids[int(det_h[b, k, 5])], boxes[b, k] + [1.5, -1, 2, 3]) for b in range(B) for k in range(0, K, 3)]
    s = {"ann_image_id": np.array([a[0] for a in ann]), "ann_category_id": np.array([a[1] for a in ann]),
         "ann_bbox": np.array([a[2] for a in ann]), "ann_area": np.array([a[2][2] * a[2][3] for a in ann]),
         "ann_iscrowd": np.zeros(len(ann), np.int32), "image_id": np.array(ids), "image_height": np.full(3, 540), "image_width": np.full(3, 720),
         "category_id": np.array(cat_ids), "detection": det_h, "num": count_h, "img_ids": np.array(ids), "center": center, "scale": scale,
         "inp_hw": np.array(inp_hw)}
    want = twin.evaluate(s)
    ev = det_eval.DetEvaluator(s)
    ev.evaluate(det, ids, center, scale, inp_hw, num=count)                                # as it lies on the device
    ret = ev.summarize()
    for k in RESULTS:
        assert _same(ev.eval[k], want[k]), k
    assert 0 < ret["ap"] <= 1 and (want["npig"][:, 0] > 0).any()
    assert want["npig"][:, 0].sum() == sum(1 for a in ann if a[0] != ids[0])                # the skipped image's ground truth is left out


# ------------------------------------------------------------------------------------------------ the rounding on its ties
def _python_round2(v):
    return float("{:.2f}".format(v))


def _map_translations(det_eval, gpu, t2, t5, score):
    """One row per block (K = 1) with zero corners under the map [1, 0, t2; 0, 1, t5]: ``(0*1 + 0*0) + t2`` is ``t2`` itself, so
    ``box[:, :2]`` is the rounding of the doubles that were uploaded.  Returns (the device's rows, err, the twin's rows)."""
    import torch
    B = len(t2)
    det = np.zeros((B, 1, 6), np.float32)
    det[:, 0, 4] = score
    block = np.zeros((B, 8), np.float64)
    block[:, 0], block[:, 2], block[:, 4], block[:, 5] = 1.0, t2, 1.0, t5
    err = torch.zeros(1, dtype=torch.int32, device=gpu)
    out = det_eval.map_detections(torch.from_numpy(det).to(gpu), torch.from_numpy(block).to(gpu),
                                  torch.zeros(1, dtype=torch.int32, device=gpu), 4.0, err)
    return {k: v.cpu().numpy() for k, v in out.items()}, int(err.item()), twin.map_rows(det, block, [0])


def test_rounding_ties_equal_pythons_format(pkg, gpu):
    from fractions import Fraction
    from clean_pvnet_amd import det_eval
    vals = twin.seeded_round2_values()
    want = np.array([_python_round2(v) for v in vals.tolist()])
    # what the set holds, before the device is touched: products that land exactly on a half, the exact residual on either side
    p = vals * 100.0
    on_half = np.flatnonzero(np.abs(p - np.rint(p)) == 0.5)
    sign = np.array([(lambda e: (e > 0) - (e < 0))(Fraction(float(vals[i])) * 100 - Fraction(float(p[i]))) for i in on_half])
    assert min((sign > 0).sum(), (sign < 0).sum(), (sign == 0).sum()) >= 1000, np.bincount(sign + 1)
    assert (np.rint(p) / 100.0 != want).sum() >= 1000                                      # rint alone gives another cent there
    # every score that can tie (a float32 times 100 is exact in binary64: only k/8) and the decimals a detector prints
    scores = np.concatenate([np.arange(9) / 8.0, np.arange(201) / 200.0]).astype(np.float32)
    want_score = np.array([_python_round2(float(v)) for v in scores])
    assert {0.12, 0.38, 0.62, 0.88} <= set(want_score[:9].tolist())                        # ties to even
    B = 30000
    vals = np.concatenate([vals, vals[:4 * B - len(vals)]]).reshape(2, B, 2)               # two calls of 30 000 blocks, two values each
    want = np.concatenate([want, want[:4 * B - len(want)]]).reshape(2, B, 2)
    idx = np.arange(B) % len(scores)
    for call in range(2):
        got, err, (tw, _, tw_err) = _map_translations(det_eval, gpu, vals[call, :, 0], vals[call, :, 1], scores[idx])
        assert err == 0 and tw_err == 0
        assert _same(got["box"][:, :2], want[call])                                        # Python itself, the sign of a zero included
        assert _same(got["score"], want_score[idx]) and _same(got["n"], np.rint(want_score[idx] * 100).astype(np.int32))
        for k in ("box", "score", "area", "n", "cat"):
            assert _same(got[k], tw[k]), k                                                 # the differences box[:, 2:] among them
    t2 = vals[0, :64, 0].copy()
    t2[17] = 5e13                                                                          # |100 v| >= 2^52: no room for a half
    got, err, (_, _, tw_err) = _map_translations(det_eval, gpu, t2, vals[0, :64, 1], scores[:64])
    assert err == 1 and tw_err == 1


# ------------------------------------------------------------------------------------------------ the accumulation at its chunk edges
def _made_up_stage_outputs(rng, counts, n_sentinel=37):
    """Sorted keys as the twin builds them, a random permutation and words, for categories with ``counts`` rows."""
    p_rank = np.concatenate([[0.15], np.full(9, 0.35 / 9), np.full(90, 0.5 / 90)])         # caps 1 and 10 keep a scattered subset
    keys = []
    for c, n in enumerate(counts):
        fields, seen = rng.integers(0, 1 << 24, 12), set()                                 # few score values: many repeats
        while len(seen) < n:
            seen.add((int(rng.choice(fields)) << 31) | (int(rng.integers(0, 301)) << 7) | int(rng.choice(100, p=p_rank)))
        keys += [(c << 55) | v for v in seen]
    keys = np.sort(np.array(keys + [twin.SENTINEL] * n_sentinel, np.int64))
    N = len(keys)
    perm = rng.permutation(N).astype(np.int64)
    words = rng.integers(0, 1 << 20, (N, twin.A)).astype(np.uint32)
    npig = rng.integers(1, 60, (len(counts), twin.A)).astype(np.int32)
    return keys, perm, words, npig


def test_accumulate_at_chunk_edges_equals_the_twin(pkg, gpu):
    import torch
    from clean_pvnet_amd import det_eval
    T, R, A, M = twin.T, twin.R, twin.A, twin.M
    rng = np.random.default_rng(65)
    counts = np.array([0, 1, 63, 64, 65, 127, 128, 129, 1000])
    C = len(counts)
    for shuffled in range(2):
        keys, perm, words, npig = _made_up_stage_outputs(rng, counts)
        c_empty, c_dark = int(np.flatnonzero(counts == 65)[0]), int(np.flatnonzero(counts == 129)[0])
        npig[c_empty, 2] = 0                                                               # this cell stays -1
        lo, hi = np.searchsorted(keys, c_dark << 55), np.searchsorted(keys, (c_dark + 1) << 55)
        words[perm[lo:hi]] |= np.uint32(1 << (T + 3))                                      # every row ignored at one threshold: tp == 0
        assert hi - lo == 129 and ((keys[lo:hi] & 127) < 1).sum() > 1
        big = keys[(keys >> 55) == int(np.flatnonzero(counts == 1000)[0])]
        assert 64 < ((big & 127) < 1).sum() < ((big & 127) < 10).sum() < 1000              # the kept rows span chunks at every cap
        want = twin.accumulate(keys, perm, words, npig, C)
        assert (want[0][:, :, c_empty, 2] == -1).all() and (want[1][3, c_dark] == 0).all() and (want[1][2, c_dark] > 0).all()
        assert (want[1][:, int(np.flatnonzero(counts == 0)[0])] == 0).all()
        res = [torch.full((n,), -1.0, dtype=torch.float64, device=gpu) for n in (T * R * C * A * M, T * C * A * M, T * R * C * A * M)]
        det_eval.accumulate(torch.from_numpy(keys).to(gpu), torch.from_numpy(perm).to(gpu), torch.from_numpy(words.view(np.int32)).to(gpu),
                            torch.from_numpy(npig.ravel()).to(gpu), C, torch.from_numpy(twin.REC_THRS).to(gpu), res[0], res[1], res[2])
        assert _same(res[0].cpu().numpy().reshape(T, R, C, A, M), want[0]), ("precision", shuffled)
        assert _same(res[1].cpu().numpy().reshape(T, C, A, M), want[1]), ("recall", shuffled)
        assert _same(res[2].cpu().numpy().reshape(T, R, C, A, M), want[2]), ("scores", shuffled)
        counts = rng.permutation(counts)                                                   # then another category has each count


# ------------------------------------------------------------------------------------------------ the counts of rows
def _run(det_eval, s, gpu):
    ev = det_eval.DetEvaluator(s)
    _feed(ev, s, [range(len(s["img_ids"]))], gpu)
    last = {"keys": ev.last["keys"].cpu().numpy(), "words": ev.last["words"].cpu().numpy().view(np.uint32)}
    ev.summarize()
    return dict(last, npig=ev.npig.astype(np.int32), **{k: ev.eval[k] for k in RESULTS})


def test_num_dtypes_and_out_of_range_counts(pkg, gpu):
    from clean_pvnet_amd import det_eval
    s, want = twin.fixture_with_twin("det_eval_rules")
    K, feed = s["detection"].shape[1], list(s["img_ids"])
    assert s["num"].dtype == np.int64
    as64, as32 = _run(det_eval, s, gpu), _run(det_eval, dict(s, num=s["num"].astype(np.int32)), gpu)
    for k in as64:
        assert _same(as32[k], as64[k]), k
    assert _same(as64["keys"], want["keys"][0]) and all(_same(as64[k], want[k]) for k in RESULTS)
    # below 0 reads as 0 and the image leaves with its ground truth; above K reads as K and the rows of zeros count
    b0, bK = feed.index(33), feed.index(12)
    num = s["num"].copy()
    assert 0 < num[b0] and 0 < num[bK] < K
    num[b0], num[bK] = -3, K + 5
    clamped = twin.evaluate(dict(s, num=np.clip(num, 0, K)))
    in_b0 = (s["ann_image_id"] == 33) & (s["ann_iscrowd"] == 0)
    gone = np.bincount(np.searchsorted(np.unique(s["category_id"]), s["ann_category_id"][in_b0]), minlength=len(want["npig"]))
    assert gone.sum() > 0 and np.array_equal(want["npig"][:, 0] - clamped["npig"][:, 0], gone)
    assert (clamped["keys"][0].reshape(-1, K)[b0] == twin.SENTINEL).all() and (clamped["keys"][0].reshape(-1, K)[bK] != twin.SENTINEL).sum() > s["num"][bK]
    for dtype in (np.int64, np.int32):
        other = dict(s, num=num.astype(dtype))
        tw = twin.evaluate(other)
        assert _same(tw["keys"][0], clamped["keys"][0]) and all(_same(tw[k], clamped[k]) for k in RESULTS)   # the twin clamps
        got = _run(det_eval, other, gpu)
        assert _same(got["keys"], clamped["keys"][0]) and _same(got["words"], clamped["words"][0]) and _same(got["npig"], clamped["npig"])
        for k in RESULTS:
            assert _same(got[k], clamped[k]), (k, dtype)
    assert not _same(clamped["precision"], want["precision"])
