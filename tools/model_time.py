#!/usr/bin/env python
"""``clean_pvnet_amd.model`` timed with device events after warm-up (ms per call, median and range over the timed rounds; each
round is ``--reps`` calls back to back) at the size of a LINEMOD mesh (5841 vertices) and of a CAD model (100 000), for one
cloud and for eight:

  fps_one_block / fps_tiled   ``farthest_point_sampling(points, 8)`` with the form forced (ONE_BLOCK where the cloud fits);
                              the two are checked to give the same indices in the same run
  bounds                      ``bounds(points)``
  diameter                    ``diameter(points)``, with ``pairs_per_s`` = B * N * (N + 1) / 2 over the time: the pairs the
                              contract asks for (the kernel visits each pair of tiles once, the diagonal tiles in full)

No time is a pass criterion anywhere; this is for whoever has the card.  ``--out`` writes the JSON lines to a file.

    python tools/model_time.py [--sizes 5841,100000] [--batches 1,8] [--rounds 20] [--warmup 3] [--reps 5] [--out profiles/model_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5841,100000")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--sn", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls back to back inside one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    lines = []
    for N in (int(v) for v in a.sizes.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            g = torch.Generator(device="cpu").manual_seed(N + B)
            pts = (torch.randn(B, N, 3, generator=g) * torch.tensor([0.04, 0.03, 0.02])).to(dev)
            forms = {"fps_tiled": lambda: [model.farthest_point_sampling(pts, a.sn, path=model.TILED) for _ in range(a.reps)],
                     "bounds": lambda: [model.bounds(pts) for _ in range(a.reps)],
                     "diameter": lambda: [model.diameter(pts) for _ in range(a.reps)]}
            res = {"N": N, "B": B, "sn": a.sn, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps}
            if N <= model.ONE_BLOCK_MAX:
                forms["fps_one_block"] = lambda: [model.farthest_point_sampling(pts, a.sn, path=model.ONE_BLOCK) for _ in range(a.reps)]
                res["forms_agree"] = bool(torch.equal(forms["fps_one_block"]()[0], forms["fps_tiled"]()[0]))
                assert res["forms_agree"], "ONE_BLOCK and TILED give different indices"
            ms = alternate(forms, a.rounds, a.warmup)
            for name in forms:
                res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
            res["diameter_pairs_per_s"] = round(B * N * (N + 1) / 2 / (res["diameter_ms"]["median"] * 1e-3), 0)
            print(json.dumps(res), flush=True)
            lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
