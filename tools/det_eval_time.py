#!/usr/bin/env python
"""``clean_pvnet_amd.det_eval`` timed against its numpy twin on the host for the same data -> profiles/det_eval_time.json.

One epoch of ``--images`` images (default 64) of 720x540 with ``--k`` detection rows each (default 100) and 4 categories, the
seeded scenario of tests/det_eval_twin.py, fed in batches of ``--batch`` (default 16):

  (a) evaluate_ms    all ``DetEvaluator.evaluate`` calls of the epoch (the host's block and its copy, map and match per call), wall
                     clock from the first call to a synchronisation behind the last
      summarize_ms   ``DetEvaluator.summarize``: the concatenation, ``torch.sort`` of the keys, the accumulation and the one
                     read-back, wall clock (it ends with the read-back)
      sort_ms        ``torch.sort`` of the epoch's keys alone, device events
  (b) twin_ms        tests/det_eval_twin.py ``evaluate`` on the host, the same images in one call, wall clock, run once: plain
                     Python loops like the reference's ``COCOeval``, which cannot run where the card is

The device's results are compared with the twin's as bytes before anything is timed.  No time is a pass criterion anywhere; this
is for whoever has the card.

    python tools/det_eval_time.py [--images 64] [--k 100] [--batch 16] [--rounds 10] [--warmup 2] [--out profiles/det_eval_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import det_eval  # noqa: E402
from tests import det_eval_twin as twin  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_eval_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_eval_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    s = twin.scenario_random(seed=64, B=a.images, K=a.k)
    t0 = time.perf_counter()
    want = twin.evaluate(s)
    twin_ms = (time.perf_counter() - t0) * 1e3
    det = torch.from_numpy(s["detection"]).to(dev)
    ev = det_eval.DetEvaluator(s)
    chunks = [list(range(lo, min(lo + a.batch, a.images))) for lo in range(0, a.images, a.batch)]
    per_call = [(det[c].contiguous(), [int(s["img_ids"][b]) for b in c], s["center"][c], s["scale"][c]) for c in chunks]

    def feed():
        for d, ids, center, scale in per_call:
            ev.evaluate(d, ids, center, scale, s["inp_hw"])

    feed()
    ev.summarize()
    for k in ("precision", "recall", "scores"):
        assert ev.eval[k].tobytes() == want[k].tobytes(), "the device differs from the twin in " + k
    keys = ev.order["keys"].clone()
    ev_ms, sum_ms = [], []
    for i in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feed()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ev.summarize()
        t2 = time.perf_counter()
        if i >= a.warmup:
            ev_ms.append((t1 - t0) * 1e3), sum_ms.append((t2 - t1) * 1e3)
    sort_ms = alternate({"sort": lambda: torch.sort(keys)}, a.rounds, a.warmup)["sort"]
    res = {"images": a.images, "rows_per_image": a.k, "categories": int(len(s["category_id"])), "calls": len(chunks), "rounds": a.rounds,
           "warmup": a.warmup, "evaluate_ms": summary(ev_ms, 3), "summarize_ms": summary(sum_ms, 3), "sort_ms": summary(sort_ms, 4),
           "twin_ms": round(twin_ms, 1), "ap": float(ev.stats[0])}
    res["device_epoch_ms"] = round(res["evaluate_ms"]["median"] + res["summarize_ms"]["median"], 3)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump([res], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
