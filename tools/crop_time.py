#!/usr/bin/env python
"""The four calls of ``clean_pvnet_amd.crop`` at the T-LESS sizes, timed with device events after warm-up (ms per call, median
and range over the timed rounds), the forms alternated in one process on the same inputs:

  decode_ct_hm      C=30 heat maps of 135 x 180 per image, K=100;
  crop_boxes        N crops of 256 x 256 from 540 x 720 images (one box per image), with the test loader's blanking;
  uncrop_keypoints  N x 9 keypoints;
  uncrop_mask       N crop masks (int64, as ``decode_keypoint`` returns them) onto the 720 x 540 canvas;
  host              the route the reference takes for the last three: the images, keypoints and masks copied to the host, the
                    numpy twin per crop (tests/crop_twin.py; the reference calls OpenCV there, which is not available here, so
                    this is a stand-in for it and not a measurement of OpenCV), the crops copied back.

N = B images per call.  There is no earlier device version to compare with.  Nothing is asserted.  ``--out`` writes the JSON
lines to a file.

    python tools/crop_time.py [--shapes 1,64] [--rounds 20] [--warmup 3] [--host-rounds 1] [--out profiles/crop_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import crop as C  # noqa: E402
from tests import crop_twin as twin  # noqa: E402

IMAGE, CANVAS, OUT, HEAT, K = (540, 720), (720, 540), (256, 256), (30, 135, 180), 100
KW = dict(scale_ratio=twin.SCALE_RATIO, box_ratio=twin.BOX_RATIO, mean=twin.MEAN, std=twin.STD)


def inputs(B, dev, seed=0):
    rng = np.random.default_rng(seed)
    hm, wh = twin.heat_maps(seed, (B,) + HEAT)
    img = rng.integers(0, 256, (B,) + IMAGE + (3,), dtype=np.uint8)
    c = rng.random((B, 2)) * [CANVAS[0] - 200, CANVAS[1] - 200] + 100
    half = rng.random((B, 2)) * 60 + 40
    boxes = np.concatenate([c - half, c + half], 1)
    kpt = rng.random((B, 9, 2)).astype(np.float32) * OUT[0]
    mask = (rng.random((B, OUT[1], OUT[0])) < 0.5).astype(np.int64)
    n = {"hm": hm, "wh": wh, "img": img, "boxes": boxes, "index": np.arange(B), "kpt": kpt, "mask": mask}
    t = {k: torch.from_numpy(v).to(dev) for k, v in n.items()}
    t["trans"] = C.crop_boxes(t["img"], t["boxes"], t["index"], OUT, **KW)["trans"]
    return t


def host_form(t):
    img, boxes, index = t["img"].cpu().numpy(), t["boxes"].cpu().numpy(), t["index"].cpu().numpy()      # copies + sync
    out = twin.crop_boxes(img, boxes, index, OUT, **KW)
    inp = torch.from_numpy(out["inp"]).to(t["img"].device)
    twin.uncrop_keypoints(t["kpt"].cpu().numpy(), out["trans"])
    twin.uncrop_mask(t["mask"].cpu().numpy(), out["trans"], CANVAS)
    return inp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,64", help="B: images per call, one box each")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=1, help="timed rounds of the host form")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for shape in a.shapes.split(","):
        B = int(shape)
        t = inputs(B, dev)
        forms = {"decode_ct_hm": lambda: C.decode_ct_hm(t["hm"], t["wh"], K=K),
                 "crop_boxes": lambda: C.crop_boxes(t["img"], t["boxes"], t["index"], OUT, **KW),
                 "uncrop_keypoints": lambda: C.uncrop_keypoints(t["kpt"], t["trans"]),
                 "uncrop_mask": lambda: C.uncrop_mask(t["mask"], t["trans"], CANVAS),
                 "host": lambda: host_form(t)}
        # the host form only in the first host_rounds timed rounds and never in the warm-up
        ms = alternate(forms, a.rounds, a.warmup, skip=lambda name, i: name == "host" and not a.warmup <= i < a.warmup + a.host_rounds)
        res = {"B": B, "N": B, "image": list(IMAGE), "out": list(OUT), "canvas": list(CANVAS), "heat": list(HEAT), "K": K,
               "rounds": a.rounds, "warmup": a.warmup, "host_rounds": min(a.host_rounds, a.rounds),
               "host_note": "crop_boxes + uncrop_keypoints + uncrop_mask through the numpy twin, copies included; decode_ct_hm not included",
               "bytes": {"crop_boxes_out": B * 3 * OUT[0] * OUT[1] * 4, "uncrop_mask_out": B * CANVAS[0] * CANVAS[1],
                         "decode_ct_hm_in": B * (HEAT[0] + 2) * HEAT[1] * HEAT[2] * 4}}
        for name, v in ms.items():
            if v:
                res[name + "_ms"] = summary(v, 4)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
