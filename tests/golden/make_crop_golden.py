#!/usr/bin/env python
"""Generate tests/golden/crop_ct_*.npz by running THE REFERENCE'S OWN ``decode_ct_hm`` on the CPU.

``lib/utils/ct/ct_decode.py`` is imported from where it lies under /root/reference (never copied); its one import,
``lib.utils.data_utils`` (which needs OpenCV), is a stub module while it loads -- ``decode_ct_hm`` itself uses nothing of it.
``clip_to_image`` lives in that stubbed module, so the clipped rows stored here are the reference's unclipped rows with the
three clamps of data_utils.py:373-377 applied by this script (``clamp_rows``).

Heat maps are ``np.random.default_rng(seed).random(shape, dtype=float32)`` (tests/crop_twin.py::heat_maps) plus planted cases:
no transcendental function, so every machine regenerates the same bits.  Small fixtures store their inputs, the full-size one
its seed and outputs only.

  crop_ct_small   B=2, C=3, 16 x 20, K=10
  crop_ct_seams   B=1, C=2, 70 x 75 (3 x 3 tiles of 32 x 32, neither side a multiple), K=20: a planted peak on both sides of every
                  tile seam and in every image corner of both classes, and one two-pixel plateau across a seam whose value lies
                  below the 21 largest (the GPU test decodes the same maps with a larger K too, where the plateau shows)
  crop_ct_full    B=1, C=30, 135 x 180, K=100, seed only

Asserted while writing (a fixture that misses one takes the next seed):
  * the K + 1 largest candidate values of every image are distinct (below that the reference's rows depend on torch.topk's tie order);
  * every image has at least K candidates;
  * the twin (tests/crop_twin.py::decode_ct_hm) equals the reference on all six columns and on ``ct``, bit for bit, clipped and not.

Run from the repository root in the build container:  python tests/golden/make_crop_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference/lib/utils"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import crop_twin as twin  # noqa: E402

TILE = 32


def load_reference():
    """ct_decode with ``lib.utils.data_utils`` stubbed; the names it imports are in sys.modules only while it loads."""
    names = ("lib.utils", "lib.utils.data_utils")
    saved = {n: sys.modules.get(n) for n in names}
    try:
        for n in names:
            sys.modules[n] = types.ModuleType(n)
        sys.modules["lib.utils"].__path__ = []
        sys.modules["lib.utils"].data_utils = sys.modules["lib.utils.data_utils"]
        spec = importlib.util.spec_from_file_location("ref_ct_decode", os.path.join(REF, "ct", "ct_decode.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


def clamp_rows(det, H, W):
    out = det.clone()
    out[..., 0:2].clamp_(min=0)
    out[..., 2].clamp_(max=W - 1)
    out[..., 3].clamp_(max=H - 1)
    return out


def plant_seams(hm):
    """ct_seams: the background is halved, the planted values are distinct and above it."""
    hm *= np.float32(0.5)
    _, C, H, W = hm.shape
    seams_x = [s for s in range(TILE, W, TILE)]
    seams_y = [s for s in range(TILE, H, TILE)]
    spots = []
    for c in range(C):
        for i, s in enumerate(seams_x):
            spots += [(c, 10 + 4 * i + c, s - 1), (c, 16 + 4 * i + c, s)]                 # left and right of a vertical seam
        for i, s in enumerate(seams_y):
            spots += [(c, s - 1, 8 + 5 * i + c), (c, s, 14 + 5 * i + c)]                  # above and below a horizontal seam
        spots += [(c, 0, 0), (c, 0, W - 1), (c, H - 1, 0), (c, H - 1, W - 1)]
    for i, (c, y, x) in enumerate(spots):
        hm[0, c, y, x] = np.float32(0.6) + np.float32(i) / np.float32(128)
    hm[0, 0, 50, TILE - 1] = hm[0, 0, 50, TILE] = np.float32(0.55)                        # the plateau, across the first seam
    return len(spots)


def definitions():
    return {"crop_ct_small": dict(shape=(2, 3, 16, 20), K=10, seed=11, store=True, plant=None),
            "crop_ct_seams": dict(shape=(1, 2, 70, 75), K=20, seed=12, store=True, plant=plant_seams),
            "crop_ct_full": dict(shape=(1, 30, 135, 180), K=100, seed=513, store=False, plant=None)}     # 13 ... 413: a tie among the 101 largest


def make(name, d, ref):
    seed = d["seed"]
    while True:
        hm, wh = twin.heat_maps(seed, d["shape"])
        planted = d["plant"](hm) if d["plant"] else 0
        tops = [(k >> np.uint64(32))[:d["K"] + 1] for k in (twin.keys(hm[b]) for b in range(d["shape"][0]))]
        if all(len(t) == d["K"] + 1 and len(np.unique(t)) == d["K"] + 1 for t in tops):
            break
        print("%s: seed %d has a tie among the %d largest values or too few candidates, taking the next" % (name, seed, d["K"] + 1))
        seed += 100
    B, C, H, W = d["shape"]
    K = d["K"]
    with torch.no_grad():
        ref_ct, ref_det = ref.decode_ct_hm(torch.from_numpy(hm.copy()), torch.from_numpy(wh.copy()), K=K)
        ref_clip = clamp_rows(ref_det, H, W)
    ref_ct, ref_det, ref_clip = ref_ct.numpy(), ref_det.numpy(), ref_clip.numpy()
    for clip, want in ((False, ref_det), (True, ref_clip)):
        ct, det, count = twin.decode_ct_hm(hm, wh, K=K, clip=clip)
        assert ct.dtype == det.dtype == ref_det.dtype == np.float32
        assert np.array_equal(det.view(np.uint32), want.view(np.uint32)), (name, clip)
        assert np.array_equal(ct.view(np.uint32), ref_ct.view(np.uint32)), (name, clip)
        assert (count == K).all()
    assert (ref_clip != ref_det).any(), "no row of %s is clipped" % name
    if d["plant"]:
        assert planted >= K + 1 and (ref_det[0, :, 4] >= np.float32(0.6)).all()
    c = dict(shape=np.array(d["shape"]), K=K, seed=seed, ref_ct=ref_ct, ref_detection=ref_det, ref_detection_clip=ref_clip,
             count=count)
    if d["store"]:
        c.update(ct_hm=hm, wh=wh)
    print("%s: seed %d, %d of %d rows clipped, lowest kept value %.6f" %
          (name, seed, int((ref_clip != ref_det).any(2).sum()), B * K, float(ref_det[..., 4].min())))
    return c


def main():
    ref = load_reference()
    for name, d in definitions().items():
        if len(sys.argv) > 1 and not sys.argv[1].startswith("--") and sys.argv[1] != name:
            continue
        c = make(name, d, ref)
        path = os.path.join(OUT, name + ".npz")
        if os.path.exists(path) and "--force" not in sys.argv:       # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v)) for k, v in c.items())
            print(name, "exists,", "identical content" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, "written,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
