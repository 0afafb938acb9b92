#!/usr/bin/env python
"""``clean_pvnet_amd.ct_train`` timed with device events after warm-up (ms per call, median and range over the timed rounds; each
round is ``--reps`` calls back to back), legs alternated in one process on the same inputs -> profiles/ct_train_time.json.

Per shape (30 classes on the 135x180 map of the 540x720 training canvas, B in {1, 32}, 6 objects per image):

  (a) fused          ``ct_loss``: forward + backward, the two heads slices of one [B,32,H,W] tensor
  (b) torch_ops      the reference's formula (lib/train/trainers/ct.py:20-26 over lib/utils/net_utils.py:9-49, 195-246) in torch
                     ops with autograd on the same GPU and the same slices; before timing (a) and (b) are held to the same formula
                     in binary64 on the device, clamped at the float32 values of 1e-4 and 0.9999 as net_utils.py:10 clamps a
                     float32 tensor: (a) within two float32 ulps, (b) within the any-order bound of a float32 sum where that
                     says anything (fewer than 2^24 elements) -- the values are recorded either way
  *_leaves           (a) and (b) with the two heads as separate contiguous leaf tensors: without autograd's backward of the two
                     slices, which is torch's cost in every other leg and no kernel of this project
  targets_kernel     ``ct_targets(boxes, cls, num, 30, H, W)`` on the device
  (c) host_targets   what it removes, per image: the heat map drawn in numpy on the host from the contract of include/pvnet_vote.h
                     (the work of lib/datasets/tless_train/ct.py:46-66 per object, timed on the host clock) plus the host-to-device
                     copy of one image's [30,H,W] map

``fused_gbps`` is the effective bandwidth of the pass pair: logits and targets read twice, the gradient written once, the wh
gradient filled once.  The baseline is (b) and (c), never the code under test.  No time is a pass criterion anywhere; this is for
whoever has the card.

    python tools/ct_train_time.py [--shapes 1x30x135x180,32x30x135x180] [--objects 6] [--rounds 20] [--warmup 3] [--reps 3]
                                  [--out profiles/ct_train_time.json]
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
from clean_pvnet_amd import ct_train  # noqa: E402
from tests import ct_train_twin as twin  # noqa: E402


def torch_ops(hp, wp, ct_hm, wh, ct_ind, ct_01, lo=1e-4, hi=1 - 1e-4):
    """The reference's formula, written from lib/utils/net_utils.py's behaviour: clamped sigmoid, the two focal sums, the gathered
    smooth L1 over weight.sum() * 2 + 1e-4.  torch.clamp takes ``lo`` and ``hi`` to the tensor's type: for a float32 tensor they
    become the float32 values of 1e-4 and 0.9999, which the binary64 evaluation is given as they are."""
    pred = torch.clamp(hp.sigmoid(), min=lo, max=hi)
    pos, neg = ct_hm.eq(1).to(pred.dtype), ct_hm.lt(1).to(pred.dtype)
    pos_loss = (torch.log(pred) * torch.pow(1 - pred, 2) * pos).sum()
    neg_loss = (torch.log(1 - pred) * torch.pow(pred, 2) * torch.pow(1 - ct_hm, 4) * neg).sum()
    num_pos = pos.sum()
    ct = torch.where(num_pos == 0, -neg_loss, -(pos_loss + neg_loss) / num_pos.clamp(min=1))
    B, _, H, W = wp.shape
    feat = wp.permute(0, 2, 3, 1).reshape(B, H * W, 2).gather(1, ct_ind[:, :, None].expand(-1, -1, 2))
    weight = ct_01[:, :, None]
    wl = torch.nn.functional.smooth_l1_loss(feat * weight, wh * weight, reduction='sum') / (weight.sum() * 2 + 1e-4)
    return ct, wl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x30x135x180,32x30x135x180")
    ap.add_argument("--objects", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ct_train_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ct_train_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    N = a.objects
    lines = []
    for shape in a.shapes.split(","):
        B, C, H, W = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(B * 1000 + H)
        x0, y0 = rng.uniform(0, W - 40, (B, N)), rng.uniform(0, H - 40, (B, N))
        boxes_h = np.stack([x0, y0, x0 + rng.uniform(8, 40, (B, N)), y0 + rng.uniform(8, 40, (B, N))], 2).astype(np.float32)
        cls_h, num_h = rng.integers(0, C, (B, N)), np.full(B, N, np.int64)
        t0 = time.perf_counter()
        host = twin.ct_targets(boxes_h[:min(B, 4)], cls_h[:min(B, 4)], num_h[:min(B, 4)], C, H, W)
        host_ms = (time.perf_counter() - t0) * 1e3 / min(B, 4)
        boxes, cls, num = torch.tensor(boxes_h, device=dev), torch.tensor(cls_h, device=dev), torch.tensor(num_h, device=dev)
        ct_hm, wh, _, ct_ind, ct_01, ct_num = ct_train.ct_targets(boxes, cls, num, C, H, W)
        n4 = min(B, 4)
        assert ct_ind[:n4].cpu().numpy().tobytes() == host["ct_ind"].tobytes() and wh[:n4].cpu().numpy().tobytes() == host["wh"].tobytes()
        assert twin.ulp_apart(ct_hm[:n4].cpu().numpy(), host["ct_hm"]).max() <= 1, "the device heat map differs from the host's"
        g = torch.Generator(device="cpu").manual_seed(B + H)
        whole = (torch.randn(B, 32, H, W, generator=g) * 3).to(dev).requires_grad_(True)      # one tensor, the heads its slices
        hp, wp = whole[:, :C], whole[:, C:C + 2]
        hpl, wpl = hp.detach().clone().requires_grad_(True), wp.detach().clone().requires_grad_(True)
        pinned = torch.from_numpy(np.ascontiguousarray(host["ct_hm"][0])).pin_memory()
        map_dev = torch.empty_like(ct_hm[0])
        tg = (ct_hm, wh, ct_ind, ct_01)

        def step(f):
            whole.grad = hpl.grad = wpl.grad = None
            ct, wl = f()
            (ct + 0.1 * wl).backward()
            return ct, wl

        legs = {"fused": lambda: ct_train.ct_loss(hp, wp, *tg), "torch_ops": lambda: torch_ops(hp, wp, *tg)}
        got = {}
        for name, f in legs.items():
            ct, wl = step(f)
            got[name] = (float(ct.detach()), float(wl.detach()), whole.grad.clone())
        with torch.no_grad():                                                       # the same formula in binary64: what both are held to
            c64, w64 = (float(v) for v in torch_ops(hp.double(), wp.double(), ct_hm.double(), wh.double(), ct_ind, ct_01.double(),
                                                    float(twin.LO), float(twin.HI)))
        ulp = lambda v: float(np.spacing(np.float32(abs(v))))                               # noqa: E731
        n_el = B * C * H * W
        assert abs(got["fused"][0] - c64) <= 2 * ulp(c64), (got["fused"][0], c64)
        assert abs(got["fused"][1] - w64) <= 2 * ulp(w64), (got["fused"][1], w64)
        if (n_el + 8) * twin.U < 1:
            assert abs(got["torch_ops"][0] - c64) <= (n_el + 8) * twin.U / (1 - (n_el + 8) * twin.U) * abs(c64)
        gdiff = float((got["fused"][2] - got["torch_ops"][2]).abs().max())

        def steps(f):
            return lambda: [step(f) for _ in range(a.reps)]

        forms = {name: steps(f) for name, f in legs.items()}
        forms["fused_leaves"] = steps(lambda: ct_train.ct_loss(hpl, wpl, *tg))
        forms["torch_ops_leaves"] = steps(lambda: torch_ops(hpl, wpl, *tg))
        forms["targets_kernel"] = lambda: [ct_train.ct_targets(boxes, cls, num, C, H, W) for _ in range(a.reps)]
        forms["h2d_map"] = lambda: [map_dev.copy_(pinned, non_blocking=True) for _ in range(a.reps)]
        ms = alternate(forms, a.rounds, a.warmup)
        res = {"B": B, "C": C, "H": H, "W": W, "objects": N, "positives": int((ct_hm == 1).sum()), "rounds": a.rounds, "warmup": a.warmup,
               "reps": a.reps, "max_grad_diff_to_torch": gdiff,
               "ct_loss": {"fused": got["fused"][0], "torch_ops": got["torch_ops"][0], "binary64": c64},
               "wh_loss": {"fused": got["fused"][1], "torch_ops": got["torch_ops"][1], "binary64": w64}}
        for name in forms:
            res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
        res["host_targets_ms_per_image"] = round(host_ms, 3)
        res["host_plus_h2d_ms_per_image"] = round(host_ms + res["h2d_map_ms"]["median"], 3)
        moved = 5 * n_el * 4 + B * 2 * H * W * 4                                    # logits and targets read twice, one gradient; the wh fill
        res["fused_gbps"] = round(moved / (res["fused_ms"]["median"] * 1e-3) / 1e9, 1)
        res["fused_leaves_gbps"] = round(moved / (res["fused_leaves_ms"]["median"] * 1e-3) / 1e9, 1)
        res["speedup_over_torch"] = round(res["torch_ops_ms"]["median"] / res["fused_ms"]["median"], 2)
        res["speedup_over_torch_leaves"] = round(res["torch_ops_leaves_ms"]["median"] / res["fused_leaves_ms"]["median"], 2)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
