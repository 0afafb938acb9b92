#!/usr/bin/env python
"""``clean_pvnet_amd.train`` timed with device events after warm-up (ms per forward + backward, median and range over the timed
rounds; each round is ``--reps`` steps back to back), legs alternated in one process on the same inputs -> profiles/train_time.json.

Per shape (480x640 at K = 9, C = 2 for B in {1, 8, 32}; 256x256 for B = 32) and mask density (2 % and 30 %):

  (a) fused_kpt     ``pvnet_loss(..., kpt_2d=)``: forward + backward, the target recomputed per pixel
  (b) fused_field   ``pvnet_loss(..., vertex=)``: forward + backward, the target read
  (c) torch_ops     the reference's formula (lib/train/trainers/pvnet.py:25-34) in torch ops with autograd on the same GPU, the
                    target resident on the device; before timing (a), (b) and (c) are held to the same formula in binary64 on the
                    device within the bounds of tests/train_twin.py (the any-order float32 bound of (c) says nothing from 2^24
                    summed elements on; the three values are recorded either way)
  (d) host_target   what (a) removes, per image: ``compute_vertex`` in numpy on the host (the work of the reference's
                    lib/utils/pvnet/pvnet_data_utils.py:30-44, timed on the host clock) plus the host-to-device copy of the field
  *_leaves          (a) and (c) with the two predictions as separate contiguous leaf tensors instead of slices of one: without
                    autograd's backward of the two slices (zeros of the whole tensor, a copy, an accumulation each), which is
                    torch's cost in every other leg and no kernel of this project
  target_kernel     ``compute_vertex(mask, kpt_2d)`` on the device, for a loader that keeps the field

``*_gbps`` is the effective bandwidth of a fused pass pair: the bytes forward and backward must move (predictions read twice,
gradients written once, the mask twice, the target field twice in form (b)) over the time.  The baseline is (c) and (d), never
the code under test.  No time is a pass criterion anywhere; this is for whoever has the card.

    python tools/train_time.py [--shapes 1x480x640,8x480x640,32x480x640,32x256x256] [--densities 0.02,0.3] [--rounds 20] [--warmup 3]
                               [--reps 3] [--out profiles/train_time.json]
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
from clean_pvnet_amd import train  # noqa: E402
from tests import train_twin as twin  # noqa: E402


def disc_mask(B, H, W, density, rng):
    """uint8 masks: one disc per image that covers ``density`` of it."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r2 = density * H * W / np.pi
    m = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        cy, cx = rng.uniform(0.35, 0.65) * H, rng.uniform(0.35, 0.65) * W
        m[b] = (y - cy) ** 2 + (x - cx) ** 2 < r2
    return m


def host_compute_vertex(mask, kpt_2d):
    """The loader's per-sample host step in numpy, from the contract of include/pvnet_vote.h: the foreground pixels, a binary64
    norm per (pixel, keypoint), a scatter into a [2K,H,W] float32 field."""
    ys, xs = np.nonzero(mask == 1)
    dx, dy = kpt_2d[None, :, 0] - xs[:, None], kpt_2d[None, :, 1] - ys[:, None]
    n = np.sqrt(dx * dx + dy * dy)
    n = np.where(n < 1e-3, n + 1e-3, n)
    out = np.zeros((2 * kpt_2d.shape[0],) + mask.shape, np.float32)
    out[0::2, ys, xs] = (dx / n).T
    out[1::2, ys, xs] = (dy / n).T
    return out


def torch_ops(vp, sp, mask, target):
    weight = mask[:, None].float()
    vote = torch.nn.functional.smooth_l1_loss(vp * weight, target * weight, reduction='sum') / weight.sum() / target.size(1)
    seg = torch.nn.functional.cross_entropy(sp, mask.long())
    return vote, seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x480x640,8x480x640,32x480x640,32x256x256")
    ap.add_argument("--densities", default="0.02,0.3")
    ap.add_argument("--K", type=int, default=9)
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="steps back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    K, C = a.K, a.C
    lines = []
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        for density in (float(v) for v in a.densities.split(",")):
            rng = np.random.default_rng(B * 1000 + H)
            mask_h = disc_mask(B, H, W, density, rng)
            kpt_h = np.stack([rng.uniform(0, W, (B, K)), rng.uniform(0, H, (B, K))], 2)
            t0 = time.perf_counter()
            target_h = np.stack([host_compute_vertex(mask_h[b], kpt_h[b]) for b in range(min(B, 4))])
            host_ms = (time.perf_counter() - t0) * 1e3 / min(B, 4)
            mask, kpt = torch.tensor(mask_h, device=dev), torch.tensor(kpt_h, device=dev)
            target = train.compute_vertex(mask, kpt)
            assert target[:min(B, 4)].cpu().numpy().tobytes() == np.ascontiguousarray(target_h).tobytes(), "the device target differs from the host's"
            g = torch.Generator(device="cpu").manual_seed(B + H)
            whole = torch.randn(B, C + 2 * K, H, W, generator=g).to(dev).requires_grad_(True)      # resnet18.py:93-94: one tensor, two slices
            sp, vp = whole[:, :C], whole[:, C:]
            pinned = torch.from_numpy(np.ascontiguousarray(target_h[0])).pin_memory()
            field_dev = torch.empty_like(target[0])

            vpl, spl = vp.detach().clone().requires_grad_(True), sp.detach().clone().requires_grad_(True)   # the same values as leaves

            def step(f):
                whole.grad = vpl.grad = spl.grad = None
                vote, seg = f()
                (vote + seg).backward()
                return vote, seg

            legs = {"fused_kpt": lambda: train.pvnet_loss(vp, sp, mask, kpt_2d=kpt),
                    "fused_field": lambda: train.pvnet_loss(vp, sp, mask, vertex=target),
                    "torch_ops": lambda: torch_ops(vp, sp, mask, target)}
            got = {}
            for name, f in legs.items():
                vote, seg = step(f)
                got[name] = (float(vote.detach()), float(seg.detach()), whole.grad.clone())
            with torch.no_grad():                                                   # the same formula in binary64: what both are held to
                v64, s64 = (float(v) for v in torch_ops(vp.double(), sp.double(), mask, target.double()))
            n_el = B * 2 * K * H * W
            zmax = float(whole.detach().abs().max())
            for name in ("fused_kpt", "fused_field"):
                assert abs(got[name][0] - v64) <= twin.vote_bound_f64(v64) and abs(got[name][1] - s64) <= twin.seg_bound_f64(s64), (name, got[name][:2], v64, s64)
            assert abs(got["torch_ops"][0] - v64) <= twin.vote_bound_f32(v64, n_el) and abs(got["torch_ops"][1] - s64) <= twin.seg_bound_f32(s64, B * H * W, C, zmax)
            assert got["fused_kpt"][0] == got["fused_field"][0] and torch.equal(got["fused_kpt"][2], got["fused_field"][2])
            gdiff = float((got["fused_kpt"][2] - got["torch_ops"][2]).abs().max())
            def steps(f):
                return lambda: [step(f) for _ in range(a.reps)]

            forms = {name: steps(f) for name, f in legs.items()}
            forms["fused_kpt_leaves"] = steps(lambda: train.pvnet_loss(vpl, spl, mask, kpt_2d=kpt))
            forms["torch_ops_leaves"] = steps(lambda: torch_ops(vpl, spl, mask, target))
            forms["target_kernel"] = lambda: [train.compute_vertex(mask, kpt) for _ in range(a.reps)]
            forms["h2d_field"] = lambda: [field_dev.copy_(pinned, non_blocking=True) for _ in range(a.reps)]
            ms = alternate(forms, a.rounds, a.warmup)
            res = {"B": B, "H": H, "W": W, "K": K, "C": C, "density": density, "foreground": int(mask_h.sum()), "rounds": a.rounds,
                   "warmup": a.warmup, "reps": a.reps, "max_grad_diff_to_torch": gdiff,
                   "vote_loss": {"fused": got["fused_kpt"][0], "torch_ops": got["torch_ops"][0], "binary64": v64},
                   "seg_loss": {"fused": got["fused_kpt"][1], "torch_ops": got["torch_ops"][1], "binary64": s64}}
            for name in forms:
                res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
            res["host_target_ms_per_image"] = round(host_ms, 3)
            res["host_plus_h2d_ms_per_image"] = round(host_ms + res["h2d_field_ms"]["median"], 3)
            field = B * 2 * K * H * W * 4
            moved = 3 * (field + B * C * H * W * 4) + 2 * B * H * W                 # read twice, gradient written once; the mask twice
            res["fused_kpt_gbps"] = round(moved / (res["fused_kpt_ms"]["median"] * 1e-3) / 1e9, 1)
            res["fused_field_gbps"] = round((moved + 2 * field) / (res["fused_field_ms"]["median"] * 1e-3) / 1e9, 1)
            res["fused_kpt_leaves_gbps"] = round(moved / (res["fused_kpt_leaves_ms"]["median"] * 1e-3) / 1e9, 1)
            res["speedup_kpt_over_torch"] = round(res["torch_ops_ms"]["median"] / res["fused_kpt_ms"]["median"], 2)
            print(json.dumps(res), flush=True)
            lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
