#!/usr/bin/env python
"""``clean_pvnet_amd.dcn.dcn_v2_conv`` on every distinct DCN layer of the reference's detector -- DLA-34 at down ratio 4
(lib/networks/ct/dla_dcn.py:361-441, ``DLASeg('dla34', ..., down_ratio=4, last_level=5)``) for a 512 x 512 input -- timed with
device events after warm-up (ms per call, median and range over the timed rounds; each round is ``--reps`` calls back to back),
alternated in one process on the same inputs with

  torch    the op as it has to be written with torch alone: the bilinear columns by four ``gather``s and elementwise blends in
           the contract's order, written out as [B, C*9, Ho*Wo], then ``torch.baddbmm`` with the weights on the bias.

The layer list is derived below by walking ``DLAUp`` / ``IDAUp`` as the reference builds and runs them, and printed.  At the
first batch size the torch form is checked against the device: both are float32 evaluations of one function at the same sample
positions, each within gamma_(K+8) * (|bias| + |weight| . colabs) of its binary64 value (tests/dcn_twin.py derives the bound),
so they lie within twice that of each other; the run fails otherwise.  ``flops`` = 2 * B * M * K * P, ``of_peak`` that over
the time over the 157.3 TFLOP/s float32 matrix peak.  ``--out`` writes the JSON lines to a file.

    python tools/dcn_time.py [--batches 1,8] [--rounds 20] [--warmup 3] [--reps 10] [--out profiles/dcn_time.json]
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
from clean_pvnet_amd import dcn  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
DLA34_CHANNELS = (16, 32, 64, 128, 256, 512)
U = 2.0 ** -24


def dla34_dcn_layers(image=512, down_ratio=4, last_level=5):
    """[(C, M, side)] of all DeformConvs in execution order: every ``proj`` runs on its level's map, every ``node`` on the
    upsampled one (dla_dcn.py:379-385); ``DLAUp`` rewrites the channels and scales of the levels it has merged (:397-403)."""
    first = down_ratio.bit_length() - 1
    layers = []

    def ida(o, channels, sides):                        # IDAUp(o, channels, .): levels 1.. are projected to o and merged at sides[0]
        for c, side in zip(channels[1:], sides[1:]):
            layers.append((c, o, side))                 # proj_i on the level as it is
            layers.append((o, o, sides[0]))             # node_i after up_i

    channels = list(DLA34_CHANNELS[first:])
    sides = [image >> level for level in range(first, len(DLA34_CHANNELS))]
    in_channels, cur = list(channels), list(sides)
    for i in range(len(channels) - 1):                  # DLAUp
        j = len(channels) - i - 2
        ida(channels[j], in_channels[j:], cur[j:])
        in_channels[j + 1:] = [channels[j]] * (len(channels) - j - 1)
        cur[j + 1:] = [cur[j]] * (len(channels) - j - 1)
    # ida_up of DLASeg: the outputs of DLAUp, finest first, up to last_level: level l has channels[l] at its own side
    n = last_level - first
    ida(channels[0], channels[:n], sides[:n])
    return layers


def make(C, M, side, B, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    t = {"input": r(B, C, side, side), "weight": r(M, C, 3, 3) / (C * 9) ** 0.5, "bias": r(M), "offset": 2 * r(B, 18, side, side),
         "mask": torch.sigmoid(r(B, 9, side, side))}
    return {k: v.to(dev) for k, v in t.items()}


def torch_columns(x, offset, mask, dtype=torch.float32, absolute=False):
    """The contract's columns for 3 x 3, stride 1, padding 1, dilation 1, one group, with torch ops: [B, C*9, H*W]."""
    B, C, H, W = x.shape
    tap = torch.arange(9, device=x.device)
    ys, xs = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    off = offset.view(B, 9, 2, H, W)
    h = (ys[None, :, None] - 1 + (tap // 3)[:, None, None]).float()[None] + off[:, :, 0]
    w = (xs[None, None, :] - 1 + (tap % 3)[:, None, None]).float()[None] + off[:, :, 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    h, w = torch.where(inside, h, torch.zeros_like(h)), torch.where(inside, w, torch.zeros_like(w))
    h0, w0 = h.floor(), w.floor()
    lh, lw = h.to(dtype) - h0.to(dtype), w.to(dtype) - w0.to(dtype)
    hh, hw = 1 - lh, 1 - lw
    h0, w0 = h0.long(), w0.long()
    planes = x.reshape(B, C, 1, H * W).expand(B, C, 9, H * W)

    def corner(dy, dx, ok):
        flat = ((h0 + dy).clamp(0, H - 1) * W + (w0 + dx).clamp(0, W - 1)).view(B, 1, 9, H * W).expand(B, C, 9, H * W)
        v = torch.gather(planes, 3, flat) * (ok & inside).view(B, 1, 9, H * W)
        v = v.to(dtype)
        return v.abs() if absolute else v

    per_tap = lambda a: a.reshape(B, 1, 9, H * W)                                   # noqa: E731
    v1, v2 = corner(0, 0, (h0 >= 0) & (w0 >= 0)), corner(0, 1, (h0 >= 0) & (w0 + 1 <= W - 1))
    v3, v4 = corner(1, 0, (h0 + 1 <= H - 1) & (w0 >= 0)), corner(1, 1, (h0 + 1 <= H - 1) & (w0 + 1 <= W - 1))
    val = ((per_tap(hh * hw) * v1 + per_tap(hh * lw) * v2) + per_tap(lh * hw) * v3) + per_tap(lh * lw) * v4
    m = per_tap(mask).to(dtype)
    return (val * (m.abs() if absolute else m)).reshape(B, C * 9, H * W)


def torch_form(t):
    B, _, H, W = t["input"].shape
    M = t["weight"].shape[0]
    col = torch_columns(t["input"], t["offset"], t["mask"])
    wt = t["weight"].reshape(1, M, -1).expand(B, M, -1)
    return torch.baddbmm(t["bias"].view(1, M, 1), wt, col).view(B, M, H, W)


def device_form(t):
    return dcn.dcn_v2_conv(t["input"], t["offset"], t["mask"], t["weight"], t["bias"], 1, 1, 1, 1)


def check(t):
    """max over outputs of |torch - device| / (2 * bound); the run fails above 1."""
    M = t["weight"].shape[0]
    K = t["weight"][0].numel()
    mag = torch_columns(t["input"], t["offset"], t["mask"], torch.float64, absolute=True)
    wt = t["weight"].double().abs().reshape(1, M, K).expand(mag.shape[0], M, K)
    bound = (K + 8) * U * torch.baddbmm(t["bias"].double().abs().view(1, M, 1), wt, mag) / (1 - (K + 8) * U)
    diff = (torch_form(t).double() - device_form(t).double()).abs().flatten(2)
    return float((diff / (2 * bound)).max()), float(diff.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="calls back to back inside one timed window")
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    layers = dla34_dcn_layers(a.image)
    distinct = sorted(set(layers), key=lambda l: (l[2], -l[0], -l[1]))
    print("DLA-34, down ratio 4, %d x %d input: %d DCN layers in execution order (C -> M @ side):" % (a.image, a.image, len(layers)))
    print("  " + ", ".join("%d->%d@%d" % l for l in layers))
    print("%d distinct: " % len(distinct) + ", ".join("%d->%d@%d x%d" % (l + (layers.count(l),)) for l in distinct), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("dcn_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    batches = [int(b) for b in a.batches.split(",")]
    lines = []
    with torch.no_grad():
        for B in batches:
            for C, M, side in distinct:
                t = make(C, M, side, B, dev)
                res = {"layer": "%d->%d" % (C, M), "C": C, "M": M, "side": side, "B": B, "count_in_dla34": layers.count((C, M, side)),
                       "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps, "torch_reps": a.torch_reps}
                if B == batches[0]:
                    ratio, diff = check(t)
                    res["torch_vs_device_over_2_bounds"], res["torch_vs_device_max_abs"] = round(ratio, 4), diff
                    assert ratio <= 1.0, "the torch form differs from the device by %.3g of twice the bound" % ratio
                forms = {"device": lambda: [device_form(t) for _ in range(a.reps)],
                         "torch": lambda: [torch_form(t) for _ in range(a.torch_reps)]}
                ms = alternate(forms, a.rounds, a.warmup)
                flops = 2.0 * B * M * C * 9 * side * side
                for name, reps in (("device", a.reps), ("torch", a.torch_reps)):
                    res[name + "_ms"] = summary([v / reps for v in ms[name]], 4)
                res["flops"] = flops
                res["device_tflops"] = round(flops / (res["device_ms"]["median"] * 1e-3) / 1e12, 2)
                res["device_of_peak"] = round(flops / (res["device_ms"]["median"] * 1e-3) / PEAK_F32_MATRIX, 4)
                res["torch_over_device"] = round(res["torch_ms"]["median"] / res["device_ms"]["median"], 2)
                print(json.dumps(res), flush=True)
                lines.append(res)
                del t
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
