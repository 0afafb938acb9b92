#!/usr/bin/env python
"""Generate tests/golden/augment_*.npz by running THE REFERENCE'S OWN augmentation control flow on the CPU.

``lib/datasets/augmentation.py`` and ``lib/datasets/transforms.py`` are loaded where they lie under /root/reference.
``torchvision`` is stubbed for their imports (nothing here calls it) and ``cv2`` -- not installed where this runs -- is replaced
by the stub below, whose ``getRotationMatrix2D``, ``warpAffine`` and ``resize`` are those of tests/augment_twin.py: what the
fixtures pin is therefore everything *around* the samplers -- the branch, the centre of rotation, the windows with their
``int()`` truncations, the crop and the pad, the order of the stages, the keypoints through ``np.matmul`` and the in-place
steps, ``ToTensor`` and ``Normalize`` -- and not OpenCV's own resampling.  ``np.random.uniform`` / ``np.random.randint`` are
patched while the reference runs so that they consume the draw table: ``uniform(lo, hi)`` is ``lo + (hi - lo) * u`` of
column 0 (the degree) and column 1 (the ratio), ``randint(lo, hi)`` is ``lo + floor(u * (hi - lo))`` of column 2 (rows) and
column 3 (columns) and raises where numpy does.  The few lines of ``Dataset.augment`` (lib/datasets/linemod/pvnet.py:62-78)
that call into augmentation.py are followed here call by call.  Nothing of the reference's program text enters the
repository: the files hold data only.

Stored per case: ``img``, ``mask``, ``kpt_2d``, ``draws``, ``out_size``, ``rotate``, ``overlap_ratio``, ``resize_ratio`` and
the reference's ``ref_img``, ``ref_mask``, ``ref_kpt_2d``, ``ref_path`` (0: ``crop_or_padding_to_fixed_size``, 1: the instance
branch) and ``ref_inp`` (``make_transforms(cfg, False)`` on ``ref_img``).  Every case is one the reference completes.

Run from the repository root in the build container:  python tests/golden/make_augment_golden.py
"""
import importlib.util
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import augment_twin as twin  # noqa: E402


def _cv2_stub():
    m = types.ModuleType("cv2")
    m.INTER_NEAREST, m.INTER_LINEAR, m.BORDER_CONSTANT = twin.INTER_NEAREST, twin.INTER_LINEAR, twin.BORDER_CONSTANT
    m.getRotationMatrix2D, m.warpAffine, m.resize = twin.getRotationMatrix2D, twin.warpAffine, twin.resize
    return m


def load_reference():
    """(augmentation, transforms) of the reference, imported with ``cv2`` and ``torchvision`` replaced for the import."""
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")
    tv.transforms, tvt.functional = tvt, tvf
    stubs = {"cv2": _cv2_stub(), "torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf}
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        mods = []
        for name in ("augmentation", "transforms"):
            spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "lib", "datasets", name + ".py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k, old in saved.items():
            if old is None:
                del sys.modules[k]
            else:
                sys.modules[k] = old
    return mods


class Draws:
    """``np.random.uniform`` / ``np.random.randint`` for one sample, fed from its row of the table."""

    def __init__(self, u, randint_columns):
        self.u, self.uniform_columns, self.randint_columns = u, [0, 1], list(randint_columns)

    def uniform(self, lo, hi):
        return lo + (hi - lo) * float(self.u[self.uniform_columns.pop(0)])

    def randint(self, lo, hi):
        if hi <= lo:
            raise ValueError("low >= high")
        return int(lo) + int(math.floor(float(self.u[self.randint_columns.pop(0)]) * float(hi - lo)))


def reference_augment(aug, img, mask, kpt_2d, height, width, u, rotate, overlap_ratio, resize_ratio):
    """lib/datasets/linemod/pvnet.py:62-78 call by call, with the draws of ``u``."""
    H, W = mask.shape
    hcoords = np.concatenate((kpt_2d, np.ones((len(kpt_2d), 1))), axis=-1)
    img = np.asarray(img).astype(np.uint8)
    foreground = np.sum(mask)
    ratio = resize_ratio[0] + (resize_ratio[1] - resize_ratio[0]) * float(u[1])
    th, tw = (int(height * ratio), int(width * ratio)) if foreground > 0 else (height, width)
    feed = Draws(u, ([] if th >= H else [2]) + ([] if tw >= W else [3]))
    old = np.random.uniform, np.random.randint
    np.random.uniform, np.random.randint = feed.uniform, feed.randint
    try:
        if foreground > 0:
            img, mask, hcoords = aug.rotate_instance(img, mask, hcoords, rotate[0], rotate[1])
            img, mask, hcoords = aug.crop_resize_instance_v1(img, mask, hcoords, height, width, overlap_ratio, resize_ratio[0], resize_ratio[1])
        else:
            img, mask = aug.crop_or_padding_to_fixed_size(img, mask, height, width)
    finally:
        np.random.uniform, np.random.randint = old
    assert not feed.randint_columns and (foreground == 0 or not feed.uniform_columns)
    return img, mask, hcoords[:, :2], int(foreground > 0)


CASES = {
    "augment_mixed_40x66": dict(batch=lambda: twin.mixed_batch((40, 66)), out_size=(40, 66), **twin.MIXED_KW),
    "augment_mixed_44x40": dict(batch=lambda: twin.mixed_batch((44, 40)), out_size=(44, 40), **twin.MIXED_KW),
    "augment_defaults_40x66": dict(batch=lambda: twin.mixed_batch((40, 66))[:3] + (twin.draws_for(5, 77),), out_size=(40, 66),
                                   rotate=twin.ROTATE, resize_ratio=twin.RESIZE),
}


def main():
    aug, tr = load_reference()
    assert "cv2" not in sys.modules and "torchvision" not in sys.modules          # the stubs are gone again
    to_tensor = tr.make_transforms(None, False)
    for name, case in CASES.items():
        img, mask, kpt, d = case["batch"]()
        height, width = case["out_size"]
        outs = [reference_augment(aug, img[b].copy(), mask[b].copy(), kpt[b].copy(), height, width, d[b], case["rotate"], twin.OVERLAP,
                                  case["resize_ratio"]) for b in range(len(img))]
        inp = [to_tensor(o[0], o[2], o[1])[0] for o in outs]
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, img=img, mask=mask, kpt_2d=kpt, draws=d, out_size=np.array(case["out_size"]), rotate=np.array(case["rotate"], np.float64),
                            overlap_ratio=np.float64(twin.OVERLAP), resize_ratio=np.array(case["resize_ratio"], np.float64),
                            ref_img=np.stack([o[0] for o in outs]), ref_mask=np.stack([o[1] for o in outs]),
                            ref_kpt_2d=np.stack([o[2] for o in outs]), ref_path=np.array([o[3] for o in outs], np.int32), ref_inp=np.stack(inp))
        print("%s: %d bytes, paths %s" % (name, os.path.getsize(path), [o[3] for o in outs]))


if __name__ == "__main__":
    main()
