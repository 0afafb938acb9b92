"""The detector's score on the device: COCO box AP (``libpvnet_vote.so``, "Detector evaluation" in include/pvnet_vote.h).

The reference's detector evaluator (lib/evaluators/tless_test/ct.py:32-79) copies every image's detections to the host, maps them
back with ``get_affine_transform(..., inv=1)``, rounds them through ``'{:.2f}'.format``, writes a JSON file and runs a pure-Python
``COCOeval`` (lib/evaluators/tless_test/coco_eval.py): a greedy matching loop per (image, category, area range, IoU threshold)
and an accumulate loop per (category, area range, detection cap, threshold).  ``DetEvaluator`` is that path for
``crop.decode_ct_hm``'s ``detection`` as it lies on the device: ``evaluate`` maps and matches a batch on the current stream and
reads nothing back, ``summarize`` orders, accumulates and does the one read-back.  Every step equals its numpy twin
(tests/det_eval_twin.py) bit for bit, and the twin equals the reference's own classes on the fixtures of tests/golden; parity of
the box IoU with the compiled pycocotools is unpinned.  There is no CPU fallback.

Stated deviations: a match is a flag (in the reference a ground truth whose id is 0 reads as "unmatched"); a score whose
two-decimal integer does not fit 24 signed bits, a value that is not finite or a label without a category raise in ``summarize``;
an image id may be passed once per epoch even when its ``num`` is 0.
"""
import ctypes

import numpy as np

from . import _native
from .ct_augment import affine, invert_affine

_lib = _native.bind("det_eval", "libpvnet_vote.so", last_error="pvv_last_error", prefix="det_eval", plain_calls=True)

T, R, A, M = 10, 101, 4, 3         # PVV_DET_T, _R, _A, _M
MAX_K = 128                        # PVV_DET_MAX_K
MAX_D = 100                        # PVV_DET_MAX_D
MAX_G = 64                         # PVV_DET_MAX_G
MAX_C = 255                        # PVV_DET_MAX_C
MAX_IMAGES = 1 << 24               # PVV_DET_MAX_IMAGES
SENTINEL = (1 << 63) - 1

# Params.setDetParams (coco_eval.py:507-511): the tables come from numpy.linspace as there, never from k/100
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]

GT_FIELDS = ("ann_image_id", "ann_category_id", "ann_bbox", "ann_area", "ann_iscrowd", "image_id", "image_height", "image_width",
             "category_id")


def gt_from_coco(dataset):
    """The ground-truth arrays of a COCO annotation file's dict (``json.load`` of it): what the reference reads from it."""
    anns, imgs, cats = dataset["annotations"], dataset["images"], dataset["categories"]
    return {"ann_image_id": np.array([a["image_id"] for a in anns], np.int64),
            "ann_category_id": np.array([a["category_id"] for a in anns], np.int64),
            "ann_bbox": np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4),
            "ann_area": np.array([a["area"] for a in anns], np.float64),
            "ann_iscrowd": np.array([a.get("iscrowd", 0) for a in anns], np.int32),
            "image_id": np.array([i["id"] for i in imgs], np.int64),
            "image_height": np.array([i["height"] for i in imgs], np.int64),
            "image_width": np.array([i["width"] for i in imgs], np.int64),
            "category_id": np.array([c["id"] for c in cats], np.int64)}


def prepare_gt(gt):
    """Host side of the ground truth: images and categories in ascending id (coco_eval.py:135-137), the label -> category index
    table (ct.py:25-30, 59), and the annotations sorted by (image rank, category index), in annotation order inside a cell
    (coco_eval.py:115-116), with the cells' offsets.  Raises ValueError on what cannot be evaluated."""
    missing = [k for k in GT_FIELDS if k not in gt]
    if missing:
        raise ValueError("det_eval: gt lacks %s" % ", ".join(missing))
    img_id = np.asarray(gt["image_id"], np.int64).ravel()
    cat_id = np.asarray(gt["category_id"], np.int64).ravel()
    images, cats = np.unique(img_id), np.unique(cat_id)
    if len(images) != len(img_id) or len(cats) != len(cat_id):
        raise ValueError("det_eval: an image id or a category id is listed twice in gt")
    if not 1 <= len(cats) <= MAX_C or not 1 <= len(images) <= MAX_IMAGES:
        raise ValueError("det_eval: gt needs 1..%d categories and 1..%d images" % (MAX_C, MAX_IMAGES))
    a_img = np.asarray(gt["ann_image_id"], np.int64).ravel()
    a_cat = np.asarray(gt["ann_category_id"], np.int64).ravel()
    n = len(a_img)
    box = np.asarray(gt["ann_bbox"], np.float64).reshape(-1, 4)
    area = np.asarray(gt["ann_area"], np.float64).ravel()
    crowd = (np.asarray(gt["ann_iscrowd"]).ravel() != 0).astype(np.int32)
    if not (len(a_cat) == len(box) == len(area) == len(crowd) == n):
        raise ValueError("det_eval: the annotation arrays of gt differ in length")
    rank, ci = np.searchsorted(images, a_img), np.searchsorted(cats, a_cat)
    if n and (not np.array_equal(images[np.minimum(rank, len(images) - 1)], a_img)
              or not np.array_equal(cats[np.minimum(ci, len(cats) - 1)], a_cat)):
        raise ValueError("det_eval: an annotation of gt names an image or a category that gt does not list")
    cell = rank * len(cats) + ci
    order = np.argsort(cell, kind="stable")
    counts = np.bincount(cell, minlength=len(images) * len(cats))
    if n and counts.max() > MAX_G:
        raise ValueError("det_eval: %d ground truths of one category in one image; at most %d are supported" % (counts.max(), MAX_G))
    off = np.zeros(len(images) * len(cats) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return {"images": images, "cats": cats, "label_to_cat": np.searchsorted(cats, cat_id).astype(np.int32),
            "box": np.ascontiguousarray(box[order]), "area": np.ascontiguousarray(area[order]),
            "crowd": np.ascontiguousarray(crowd[order]), "off": off.astype(np.int32)}


def inverse_transform(center, scale, inp_hw):
    """``get_affine_transform(center, scale, 0, [w, h], inv=1)`` (ct.py:46-47) as six binary64 values: the closed form of the forward
    transform (``ct_augment.affine``) inverted in the operation order of ``invertAffineTransform``."""
    h, w = (int(v) for v in inp_hw)
    c = np.asarray(center, np.float32).ravel()
    s = np.asarray(scale, np.float32).ravel()
    return invert_affine(affine(float(c[0]), float(c[1]), float(s[0]), 0, w, h))


def summarize_stats(precision, recall):
    """The 12 values of ``COCOeval.summarize`` (coco_eval.py:428-473), taken with numpy exactly as ``_summarize`` takes them."""
    def one(ap=1, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    stats = np.zeros((12,))
    stats[0] = one(1)
    stats[1] = one(1, iou_thr=.5, max_dets=MAX_DETS[2])
    stats[2] = one(1, iou_thr=.75, max_dets=MAX_DETS[2])
    stats[3] = one(1, area="small", max_dets=MAX_DETS[2])
    stats[4] = one(1, area="medium", max_dets=MAX_DETS[2])
    stats[5] = one(1, area="large", max_dets=MAX_DETS[2])
    stats[6] = one(0, max_dets=MAX_DETS[0])
    stats[7] = one(0, max_dets=MAX_DETS[1])
    stats[8] = one(0, max_dets=MAX_DETS[2])
    stats[9] = one(0, area="small", max_dets=MAX_DETS[2])
    stats[10] = one(0, area="medium", max_dets=MAX_DETS[2])
    stats[11] = one(0, area="large", max_dets=MAX_DETS[2])
    return stats


def box_iou(dt, gt, iscrowd):
    """``maskUtils.iou`` for boxes (coco_eval.py:189-190): ``dt`` [D,4], ``gt`` [G,4] xywh float64 CUDA tensors, ``iscrowd`` [G]
    (any integer or bool dtype); returns [D,G] float64.  ``u = crowd ? da : (da + ga) - i``, everything binary64, uncontracted."""
    import torch
    _native.need_cuda(dt, "dt", "det_eval")
    _native.need_cuda(gt, "gt", "det_eval")
    _native.need_cuda(iscrowd, "iscrowd", "det_eval")
    if dt.dtype != torch.float64 or gt.dtype != torch.float64:
        raise TypeError("det_eval: dt and gt must be float64, got %s and %s" % (dt.dtype, gt.dtype))
    D, G = dt.shape[0], gt.shape[0]
    assert tuple(dt.shape) == (D, 4) and tuple(gt.shape) == (G, 4) and tuple(iscrowd.shape) == (G,), (dt.shape, gt.shape, iscrowd.shape)
    d, g, c = dt.contiguous(), gt.contiguous(), (iscrowd != 0).to(torch.int32).contiguous()
    out = torch.empty(D, G, dtype=torch.float64, device=dt.device)
    _lib.call("pvv_det_box_iou", dt.device, d.data_ptr(), D, g.data_ptr(), c.data_ptr(), G, out.data_ptr())
    return out


def map_detections(detection, block, label_to_cat, down_ratio, err):
    """``pvv_det_map``: ``detection`` [B,K,6] float32, ``block`` [B,8] float64, ``label_to_cat`` int32, ``err`` int32 [1], all on the
    device.  Returns the dict of ``box`` [B*K,4], ``score``, ``area`` float64 and ``n``, ``cat`` int32."""
    import torch
    B, K = detection.shape[:2]
    dev = detection.device
    out = {"box": torch.empty(B * K, 4, dtype=torch.float64, device=dev), "score": torch.empty(B * K, dtype=torch.float64, device=dev),
           "area": torch.empty(B * K, dtype=torch.float64, device=dev), "n": torch.empty(B * K, dtype=torch.int32, device=dev),
           "cat": torch.empty(B * K, dtype=torch.int32, device=dev)}
    _lib.call("pvv_det_map", dev, detection.data_ptr(), block.data_ptr(), label_to_cat.data_ptr(), label_to_cat.numel(), B, K,
              float(down_ratio), out["box"].data_ptr(), out["score"].data_ptr(), out["area"].data_ptr(), out["n"].data_ptr(),
              out["cat"].data_ptr(), err.data_ptr())
    return out


def match_detections(mapped, num, block, gt_dev, B, K, tables, npig):
    """``pvv_det_match`` on the output of ``map_detections``: returns ``keys`` [B*K] int64 and ``words`` [B*K,4] int32 (the bits of
    the unsigned words) at the ordered position of each row, and adds to ``npig`` [C,4] int32."""
    import torch
    dev = block.device
    keys = torch.empty(B * K, dtype=torch.int64, device=dev)
    words = torch.empty(B * K, A, dtype=torch.int32, device=dev)
    _lib.call("pvv_det_match", dev, mapped["box"].data_ptr(), mapped["area"].data_ptr(), mapped["n"].data_ptr(),
              mapped["cat"].data_ptr(), _native.ptr(num), int(num is not None and num.dtype == torch.int64), block.data_ptr(), B, K,
              gt_dev["box"].data_ptr(), gt_dev["area"].data_ptr(), gt_dev["crowd"].data_ptr(), gt_dev["off"].data_ptr(),
              gt_dev["I"], gt_dev["C"], tables["iou"].data_ptr(), tables["area"].data_ptr(), keys.data_ptr(), words.data_ptr(),
              npig.data_ptr())
    return keys, words


def accumulate(keys_sorted, perm, words, npig, C, rec_thrs, precision, recall, scores):
    """``pvv_det_accumulate``: fills the cells with ``npig > 0`` of ``precision``, ``scores`` [T,R,C,A,M] and ``recall`` [T,C,A,M]
    (float64 device tensors the caller has filled with -1)."""
    N = keys_sorted.numel()
    dev = npig.device
    ws, _ = _lib.workspace("pvv_det_accumulate_workspace_bytes", dev, N, refused=lambda nbytes: N and nbytes == 0)
    caps = (ctypes.c_int32 * M)(*MAX_DETS)
    _lib.call("pvv_det_accumulate", dev, keys_sorted.data_ptr(), perm.data_ptr(), words.data_ptr(), N, npig.data_ptr(), C,
              rec_thrs.data_ptr(), caps, ws.data_ptr(), ws.numel(), precision.data_ptr(), recall.data_ptr(), scores.data_ptr())


class DetEvaluator:
    """The reference's detector ``Evaluator`` (tless_test/ct.py) with its ``COCOeval`` on the device.

    :param gt:          the ground truth as host arrays (``GT_FIELDS``; ``gt_from_coco`` makes them from an annotation file's dict):
                        per annotation ``ann_image_id``, ``ann_category_id``, ``ann_bbox`` [N,4] xywh, ``ann_area``, ``ann_iscrowd``;
                        ``image_id`` with ``image_height`` / ``image_width``; ``category_id`` in the order of ``getCatIds()`` (a
                        detection's label indexes this list).  It is uploaded once, at the first ``evaluate``.
    :param down_ratio:  ``tless_config.down_ratio``
    ``evaluate`` per batch, ``summarize`` per epoch: ``{'ap': stats[0]}``, with ``.eval`` (``precision`` [T,R,K,A,M], ``recall``
    [T,K,A,M], ``scores`` [T,R,K,A,M]), ``.stats`` (the 12 values) and ``.aps`` kept as the reference keeps them."""

    def __init__(self, gt, *, down_ratio=4, device="cuda"):
        self._gt = prepare_gt(gt)
        self.image_hw = {int(i): (int(h), int(w)) for i, h, w in zip(np.asarray(gt["image_id"]).ravel(),
                                                                     np.asarray(gt["image_height"]).ravel(),
                                                                     np.asarray(gt["image_width"]).ravel())}
        self.down_ratio = float(down_ratio)
        self.device = device
        self.aps, self.eval, self.stats = [], {}, None
        self._dev = None
        self._seen = set()
        self._keys, self._words = [], []
        self.last = None

    def _put_gt(self, dev):
        import torch
        g = self._gt
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self._dev = {"box": put(g["box"].reshape(-1, 4)) if len(g["box"]) else torch.zeros(1, 4, dtype=torch.float64, device=dev),
                     "area": put(g["area"]) if len(g["area"]) else torch.zeros(1, dtype=torch.float64, device=dev),
                     "crowd": put(g["crowd"]) if len(g["crowd"]) else torch.zeros(1, dtype=torch.int32, device=dev),
                     "off": put(g["off"]), "I": len(g["images"]), "C": len(g["cats"]), "label_to_cat": put(g["label_to_cat"])}
        self._tables = {"iou": put(IOU_THRS), "rec": put(REC_THRS), "area": put(np.array(AREA_RNG, np.float64))}
        self._npig = torch.zeros(len(g["cats"]) * A, dtype=torch.int32, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)

    def evaluate(self, detection, img_ids, center, scale, inp_hw, num=None):
        """Map and match the detections of a batch (ct.py:32-66 and coco_eval.py:122-159 for these images).
        :param detection:  [B,K,6] float32 CUDA tensor (x0, y0, x1, y1, score, label) on the output map, ``K <= 128``
        :param img_ids:    B image ids (host)
        :param center:     [B,2] and ``scale`` [B,2] or [B]: ``batch['meta']`` of each image (host)
        :param inp_hw:     (h, w) of the network input
        :param num:        [B] int32 / int64 CUDA tensor (``decode_ct_hm``'s ``count``) or host integers: the rows of each image that
                           count; None for all ``K``.  An image with 0 is left out, its ground truth with it (ct.py:43-44)."""
        import torch
        if not isinstance(detection, torch.Tensor) or detection.dtype != torch.float32:
            raise TypeError("det_eval: detection must be a float32 tensor, got %s" % getattr(detection, "dtype", type(detection)))
        if detection.dim() != 3 or detection.shape[2] != 6:
            raise ValueError("det_eval: detection must be [B,K,6], got %s" % (tuple(detection.shape),))
        B, K = int(detection.shape[0]), int(detection.shape[1])
        if not 1 <= K <= MAX_K:
            raise ValueError("det_eval: K must lie in [1, %d], got %d" % (MAX_K, K))
        ids = [int(v) for v in np.asarray(img_ids).ravel()]
        center = np.asarray(center, np.float32).reshape(-1, 2)
        scale = np.asarray(scale, np.float32).reshape(len(center), -1 if len(center) else 2)      # (an empty batch is a no-op below)
        if not (len(ids) == len(center) == B):
            raise ValueError("det_eval: %d images, %d ids, %d centres" % (B, len(ids), len(center)))
        images = self._gt["images"]
        rank = np.searchsorted(images, ids)
        for i, r in zip(ids, rank):
            if r >= len(images) or images[r] != i:
                raise ValueError("det_eval: image %d is not in gt" % i)
        if len(set(ids)) != len(ids) or self._seen.intersection(ids):
            raise ValueError("det_eval: an image id was passed twice: %s" % sorted(set(i for i in ids if ids.count(i) > 1) | self._seen.intersection(ids)))
        if num is not None and isinstance(num, torch.Tensor) and num.dtype not in (torch.int32, torch.int64):
            raise TypeError("det_eval: num must be int32 or int64, got %s" % num.dtype)
        _native.need_cuda(detection, "detection", "det_eval")
        if B == 0:
            return
        dev = detection.device
        if self._dev is None:
            self._put_gt(dev)
        block = np.zeros((B, 8), np.float64)
        for b in range(B):
            block[b, :6] = inverse_transform(center[b], scale[b], inp_hw)
            block[b, 6] = float(rank[b])
        block = torch.from_numpy(block).to(dev)
        if num is not None:
            num = (num if isinstance(num, torch.Tensor) else torch.as_tensor(np.asarray(num, np.int64))).to(dev).contiguous()
            if tuple(num.shape) != (B,):
                raise ValueError("det_eval: num must be [B], got %s" % (tuple(num.shape),))
        det = detection.contiguous()
        mapped = map_detections(det, block, self._dev["label_to_cat"], self.down_ratio, self._err)
        keys, words = match_detections(mapped, num, block, self._dev, B, K, self._tables, self._npig)
        self._seen.update(ids)
        self._keys.append(keys)
        self._words.append(words)
        self.last = {"mapped": mapped, "keys": keys, "words": words}

    def summarize(self):
        """Order, accumulate, read back once (ct.py:68-79, coco_eval.py:316-473); then the state starts again."""
        import torch
        if self._dev is None:
            raise RuntimeError("det_eval: summarize() before any evaluate()")
        C = self._dev["C"]
        dev = self._npig.device
        keys, words = torch.cat(self._keys), torch.cat(self._words)
        keys_sorted, perm = torch.sort(keys)                   # unique keys (all but the rows left out): any sort gives this order
        n_p, n_r = T * R * C * A * M, T * C * A * M
        res = torch.full((2 * n_p + n_r + 1 + C * A,), -1.0, dtype=torch.float64, device=dev)
        precision, scores, recall = res[:n_p], res[n_p:2 * n_p], res[2 * n_p:2 * n_p + n_r]
        accumulate(keys_sorted, perm, words, self._npig, C, self._tables["rec"], precision, recall, scores)
        res[2 * n_p + n_r] = self._err[0].to(torch.float64)
        res[2 * n_p + n_r + 1:] = self._npig.to(torch.float64)
        host = res.cpu().numpy()                               # the one read-back
        self.order = {"keys": keys_sorted, "perm": perm}
        self._keys, self._words, self._seen = [], [], set()
        self._npig.zero_()
        self._err.zero_()
        if host[2 * n_p + n_r] != 0:
            raise RuntimeError("det_eval: a detection was not finite, its score outside the 24-bit range of the order's key, or its "
                               "label without a category")
        self.eval = {"precision": host[:n_p].reshape(T, R, C, A, M).copy(), "scores": host[n_p:2 * n_p].reshape(T, R, C, A, M).copy(),
                     "recall": host[2 * n_p:2 * n_p + n_r].reshape(T, C, A, M).copy(), "counts": [T, R, C, A, M]}
        self.npig = host[2 * n_p + n_r + 1:].astype(np.int64).reshape(C, A)
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"])
        self.aps.append(self.stats[0])
        return {"ap": self.stats[0]}
