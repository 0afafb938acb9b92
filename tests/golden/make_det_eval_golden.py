#!/usr/bin/env python
"""Generate tests/golden/det_eval_*.npz by running THE REFERENCE'S OWN detector evaluator on the CPU.

``lib/evaluators/tless_test/ct.py`` (``Evaluator.evaluate`` and ``summarize``, called on an instance made without ``__init__``,
which only opens the annotation file) and ``lib/evaluators/tless_test/coco_eval.py`` (``COCOeval``) are imported where they lie
under /root/reference, with ``lib/utils/data_utils.py`` (``get_affine_transform``, ``affine_transform``) and
``lib/utils/tless/tless_config.py``.  What is absent where this runs is replaced for the import: ``pycocotools`` by the minimal
ground-truth / result container below (``getCatIds``, ``getImgIds``, ``getAnnIds``, ``loadAnns``, ``loadImgs`` and ``loadRes`` with
its ``area = w*h``, ``id = index + 1``, ``iscrowd = 0``) and by the box rule of tests/det_eval_twin.py for ``maskUtils.iou``;
``lib.config``, ``lib.datasets.dataset_catalog`` and ``imgaug`` by empty stand-ins; ``cv2`` by the binary64 three-point solve of
tests/ct_augment_twin.py for ``getAffineTransform``.  ``np.float`` and a ``np.linspace`` that accepts the float count ``Params``
passes are put back while the reference runs (it was written for an older numpy).  The fixtures therefore pin everything around
the IoU rule -- the map with its rounding, the orders, the greedy loop, the accumulation and the 12 means -- and not the compiled
pycocotools.  Nothing of the reference's program text enters the repository: the files hold data only.

Run from the repository root in the build container:  python tests/golden/make_det_eval_golden.py
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import ct_augment_twin  # noqa: E402
from tests import det_eval_twin as twin  # noqa: E402


class _Anything:
    def __getattr__(self, name):
        return _Anything()


class COCO:
    """The part of pycocotools.coco.COCO the reference touches, for boxes."""

    def __init__(self, dataset=None):
        self.dataset = dataset or {"images": [], "annotations": [], "categories": []}
        self.anns = {a["id"]: a for a in self.dataset["annotations"]}
        self.imgs = {i["id"]: i for i in self.dataset["images"]}
        self.imgToAnns = {}
        for a in self.dataset["annotations"]:
            self.imgToAnns.setdefault(a["image_id"], []).append(a)

    def getCatIds(self):
        return [c["id"] for c in self.dataset["categories"]]

    def getImgIds(self):
        return list(self.imgs.keys())

    def getAnnIds(self, imgIds=[], catIds=[]):
        anns = [a for i in imgIds if i in self.imgToAnns for a in self.imgToAnns[i]]
        if len(catIds):
            anns = [a for a in anns if a["category_id"] in catIds]
        return [a["id"] for a in anns]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def loadImgs(self, ids):
        return [self.imgs[i] for i in (ids if isinstance(ids, (list, tuple)) else [ids])]

    def loadRes(self, path):
        anns = json.load(open(path))
        for k, a in enumerate(anns):
            bb = a["bbox"]
            a["area"], a["id"], a["iscrowd"] = bb[2] * bb[3], k + 1, 0
        return COCO({"images": list(self.dataset["images"]), "annotations": anns, "categories": list(self.dataset["categories"])})


def _iou(d, g, iscrowd):
    if len(d) == 0 or len(g) == 0:
        return []
    return twin.box_iou(d, g, iscrowd)


def load_reference():
    cv2 = types.ModuleType("cv2")
    cv2.getAffineTransform = ct_augment_twin.getAffineTransform
    config = types.ModuleType("lib.config")
    config.cfg = _Anything()
    catalog = types.ModuleType("lib.datasets.dataset_catalog")
    catalog.DatasetCatalog = _Anything()
    imgaug, augmenters = types.ModuleType("imgaug"), types.ModuleType("imgaug.augmenters")
    imgaug.augmenters = augmenters
    pyc, mask, coco = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.mask"), types.ModuleType("pycocotools.coco")
    mask.iou, coco.COCO, pyc.mask, pyc.coco = _iou, COCO, mask, coco
    stubs = {"cv2": cv2, "lib.config": config, "lib.datasets.dataset_catalog": catalog, "imgaug": imgaug, "imgaug.augmenters": augmenters,
             "pycocotools": pyc, "pycocotools.mask": mask, "pycocotools.coco": coco}
    before = set(sys.modules)
    held = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "lib" or k.startswith("lib.")}
    sys.modules.update(stubs)
    sys.path.insert(0, REF)
    try:
        ct = importlib.import_module("lib.evaluators.tless_test.ct")
    finally:
        sys.path.remove(REF)
        for k in set(sys.modules) - before:
            del sys.modules[k]
        for k in [k for k in sys.modules if k == "lib" or k.startswith("lib.")]:
            del sys.modules[k]
        sys.modules.update(held)
    return ct


@contextlib.contextmanager
def old_numpy():
    linspace = np.linspace
    np.linspace = lambda start, stop, num=50, **kw: linspace(start, stop, int(num), **kw)
    had = "float" in np.__dict__
    np.float = float
    try:
        yield
    finally:
        np.linspace = linspace
        if not had:
            del np.float


def run_reference(ct, s):
    dataset = {"images": [{"id": int(i), "height": int(h), "width": int(w)}
                          for i, h, w in zip(s["image_id"], s["image_height"], s["image_width"])],
               "categories": [{"id": int(c)} for c in s["category_id"]],
               "annotations": [{"id": k + 1, "image_id": int(s["ann_image_id"][k]), "category_id": int(s["ann_category_id"][k]),
                                "bbox": [float(v) for v in s["ann_bbox"][k]], "area": float(s["ann_area"][k]),
                                "iscrowd": int(s["ann_iscrowd"][k])} for k in range(len(s["ann_image_id"]))]}
    h, w = (int(v) for v in s["inp_hw"])
    with tempfile.TemporaryDirectory() as tmp, old_numpy(), contextlib.redirect_stdout(io.StringIO()):
        ev = object.__new__(ct.Evaluator)
        ev.results, ev.img_ids, ev.aps, ev.result_dir = [], [], [], tmp
        ev.coco = COCO(dataset)
        ev.json_category_id_to_contiguous_id = {v: i for i, v in enumerate(ev.coco.getCatIds())}
        ev.contiguous_category_id_to_json_id = {v: k for k, v in ev.json_category_id_to_contiguous_id.items()}
        for b, i in enumerate(s["img_ids"]):
            rows = s["detection"].shape[1] if s["num"] is None else int(s["num"][b])
            output = {"detection": torch.from_numpy(s["detection"][b:b + 1, :rows].copy())}
            batch = {"meta": {"img_id": [int(i)], "center": torch.from_numpy(s["center"][b:b + 1].copy()),
                              "scale": torch.from_numpy(s["scale"][b:b + 1].copy())}, "inp": torch.zeros(1, 3, h, w)}
            ev.evaluate(output, batch)
        results = [dict(r) for r in ev.results]
        captured = {}
        init = ct.COCOeval.__init__

        def spy(self, *a, **k):
            init(self, *a, **k)
            captured["e"] = self
        ct.COCOeval.__init__ = spy
        try:
            ret = ev.summarize()
        finally:
            ct.COCOeval.__init__ = init
    e = captured["e"]
    assert ret["ap"] == e.stats[0]
    return {"ref_box": np.array([r["bbox"] for r in results], np.float64).reshape(-1, 4),
            "ref_score": np.array([r["score"] for r in results], np.float64),
            "ref_image": np.array([r["image_id"] for r in results], np.int64),
            "ref_category": np.array([r["category_id"] for r in results], np.int64),
            "ref_precision": e.eval["precision"], "ref_recall": e.eval["recall"], "ref_scores": e.eval["scores"],
            "ref_stats": np.asarray(e.stats, np.float64), "ref_iou_thrs": np.asarray(e.params.iouThrs, np.float64),
            "ref_rec_thrs": np.asarray(e.params.recThrs, np.float64)}


def main():
    ct = load_reference()
    assert "cv2" not in sys.modules and "pycocotools" not in sys.modules
    for name, make in twin.SCENARIOS.items():
        s = make()
        ref = run_reference(ct, s)
        path = os.path.join(OUT, name + ".npz")
        inputs = {k: v for k, v in s.items() if v is not None}
        np.savez_compressed(path, has_num=np.array(s["num"] is not None), **inputs, **ref)
        print("%s: %d bytes, %d results, ap %.6f, numpy %s" % (name, os.path.getsize(path), len(ref["ref_score"]), ref["ref_stats"][0], np.__version__))


if __name__ == "__main__":
    main()
