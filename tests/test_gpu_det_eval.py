"""Detector evaluation on the MI355X (clean_pvnet_amd.det_eval): the box IoU, every stage's output and the evaluator's results
equal the numpy twin (tests/det_eval_twin.py, itself held to the reference's ``Evaluator`` and ``COCOeval`` in
tests/test_det_eval.py) bit for bit, for any split of the images into calls and for a second epoch; the error flag raises; and
``crop.decode_ct_hm``'s output runs through as it lies on the device."""
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
