#!/usr/bin/env python
"""Forward + backward of one trainable ``DCN`` layer's convolution (``clean_pvnet_amd.dcn_train.dcn_v2_conv``) at the detector's
shapes -- 3 x 3, stride 1, padding 1, one deformable group; 64 -> 64 at 135 x 180 and 128 -> 64 at 68 x 90; B = 1 and B = 32 --
timed with device events after warm-up (ms per step, median and range over the timed rounds), alternated in one process on the
same inputs with

  torch    the same function written with torch ops on the device -- the four ``gather``s and the blend of tools/dcn_time.py,
           ``baddbmm`` on the bias --, its backward by autograd: the only alternative a user has today.

A step is: forward, then backward from a fixed upstream gradient, with all five inputs requiring grad.  At B = 1 the two forms'
gradients are compared and the largest differences printed (both are float32 evaluations of the same derivative; this is a
sanity check, the tests hold the device to its twin bit for bit).  ``groups_ms`` times the backward alone with ``need`` set
to one group of gradients at a time (offset and mask: gcol + coord; input: gcol + coord's maximum + the scatter and its finish;
weight: the column GEMM and its reduction; bias), ``workspace_bytes`` is what the backward allocates.  ``--kernel-stats DIR``
adds ``kernels_us`` from ``DIR/<C>x<M>x<H>x<W>xB<B>*kernel_stats.csv``, written by a profiler run of ``--profile-pass`` on one
``--config`` (the profiler goes in a run of its own: its numbers are not mixed into the event timings).

    python tools/dcn_train_time.py [--rounds 10] [--warmup 3] [--out profiles/dcn_train_time.json] [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats -d DIR -o 64x64x135x180xB1 --output-format csv -- \\
        python tools/dcn_train_time.py --config 64,64,135,180,1 --profile-pass
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from dcn_time import torch_form  # noqa: E402
from clean_pvnet_amd import dcn_train  # noqa: E402

CONFIGS = [(64, 64, 135, 180, 1), (128, 64, 68, 90, 1), (64, 64, 135, 180, 32), (128, 64, 68, 90, 32)]      # C, M, H, W, B
KEYS = ("input", "offset", "mask", "weight", "bias")
GROUPS = {"offset_mask": (False, True, True, False, False), "input": (True, False, False, False, False),
          "weight": (False, False, False, True, False), "bias": (False, False, False, False, True)}


def make(C, M, H, W, B, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    t = {"input": r(B, C, H, W), "weight": r(M, C, 3, 3) / (C * 9) ** 0.5, "bias": r(M), "offset": 2 * r(B, 18, H, W),
         "mask": torch.sigmoid(r(B, 9, H, W)), "gout": r(B, M, H, W)}
    return {k: v.to(dev) for k, v in t.items()}


def step(form, t):
    """Forward + backward; the five gradients."""
    leaves = {k: t[k].detach().requires_grad_(True) for k in KEYS}
    form(leaves).backward(t["gout"])
    return [leaves[k].grad for k in KEYS]


def device_form(t):
    return dcn_train.dcn_v2_conv(t["input"], t["offset"], t["mask"], t["weight"], t["bias"], 1, 1, 1, 1)


def backward_only(t, need):
    return dcn_train.dcn_v2_backward(t["input"], t["offset"], t["mask"], t["weight"], t["bias"], t["gout"], 1, 1, 1, 1, need=need)


def kernel_stats(directory, tag):
    out = {}
    for f in glob.glob(os.path.join(directory, "**", tag + "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_dcn_[a-z_]+", r["Name"])
            if m:
                out[m.group(0)] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="device steps back to back inside one timed window (the torch form takes one)")
    ap.add_argument("--config", default=None, help="C,M,H,W,B: this one instead of the detector's four")
    ap.add_argument("--profile-pass", action="store_true", help="a few device steps and nothing else: what a profiler run wraps")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    configs = [tuple(int(v) for v in a.config.split(","))] if a.config else CONFIGS
    if not torch.cuda.is_available():
        raise SystemExit("dcn_train_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    lines = []
    for C, M, H, W, B in configs:
        t = make(C, M, H, W, B, dev)
        if a.profile_pass:
            for _ in range(5):
                step(device_form, t)
            torch.cuda.synchronize()
            continue
        nbytes = dcn_train._lib.pvv_dcn_backward_workspace_bytes(B, C, H, W, M, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0)
        res = {"layer": "%d->%d" % (C, M), "C": C, "M": M, "H": H, "W": W, "B": B, "rounds": a.rounds, "warmup": a.warmup,
               "reps": a.reps, "workspace_bytes": int(nbytes)}
        if B == 1:
            ours, theirs = step(device_form, t), step(torch_form, t)
            res["max_abs_diff_to_torch"] = {k: float((x - y).abs().max()) for k, x, y in zip(KEYS, ours, theirs)}
            res["max_abs_grad"] = {k: float(x.abs().max()) for k, x in zip(KEYS, ours)}
            del ours, theirs
        forms = {"device": lambda: [step(device_form, t) for _ in range(a.reps)], "torch": lambda: step(torch_form, t)}
        ms = alternate(forms, a.rounds, a.warmup)
        res["device_ms"] = summary([v / a.reps for v in ms["device"]], 4)
        res["torch_ms"] = summary(ms["torch"], 4)
        res["torch_over_device"] = round(res["torch_ms"]["median"] / res["device_ms"]["median"], 2)
        with torch.no_grad():
            group = lambda need: lambda: [backward_only(t, need) for _ in range(a.reps)]      # noqa: E731
            groups = {name: group(need) for name, need in GROUPS.items()}
            groups["forward"] = lambda: [device_form(t) for _ in range(a.reps)]
            gms = alternate(groups, a.rounds, a.warmup)
        res["groups_ms"] = {name: summary([v / a.reps for v in vals], 4) for name, vals in gms.items()}
        if a.kernel_stats:
            stats = kernel_stats(a.kernel_stats, "%dx%dx%dx%dxB%d" % (C, M, H, W, B))
            if stats:
                res["kernels_us"] = stats
        print(json.dumps(res), flush=True)
        lines.append(res)
        del t
        torch.cuda.empty_cache()
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
