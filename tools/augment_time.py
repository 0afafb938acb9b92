#!/usr/bin/env python
"""``clean_pvnet_amd.augment`` timed with device events after warm-up (ms per batch, median and range over the timed rounds; each
round is ``--reps`` calls back to back), legs alternated in one process on the same inputs -> profiles/augment_time.json.

Per batch size (32 and 1) at 480x640 -> 480x640, K = 9, one disc of 5 % per mask, the reference's ranges and amplitudes:

  (a) device        ``PVNetAugment()(img, mask, kpt_2d, 480, 640, draws)``: the host's parameter blocks and their two copies, the
                    geometry launches and the transform launches
      augment       ``pvnet_augment`` alone;  transform  ``pvnet_transform`` alone (on (a)'s intermediate image)
  (b) torch_ops     the same chain in torch ops on the same GPU, in float32 and in the cheapest form torch offers: ONE
                    ``grid_sample`` per tensor for rotation, window and resize together (the reference resamples twice), a
                    separable ``conv2d`` on a reflect border, pointwise brightness / contrast / saturation (the hue step is left out
                    of this leg), the normalisation.  Its window comes from host numbers, not from the mask, so it also skips the
                    two reductions.  Different arithmetic: it is a cost comparison and is not compared for equality.
  (c) twin_cpu      tests/augment_twin.py per image on one CPU core, on the host clock: the numpy twin, NOT OpenCV (which is not
                    installed where this project is built), so it says what the contract costs in numpy and nothing about the
                    reference's loader.

No time is a pass criterion anywhere; this is for whoever has the card.

    python tools/augment_time.py [--batches 32,1] [--rounds 20] [--warmup 3] [--reps 3] [--out profiles/augment_time.json]
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
import torch.nn.functional as F  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import augment  # noqa: E402
from tests import augment_twin as twin  # noqa: E402

H, W, K = 480, 640, 9


def inputs(B, rng):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        cy, cx = rng.uniform(0.35, 0.65) * H, rng.uniform(0.35, 0.65) * W
        mask[b] = (y - cy) ** 2 + (x - cx) ** 2 < 0.05 * H * W / np.pi
    kpt = np.stack([rng.uniform(0, W, (B, K)), rng.uniform(0, H, (B, K))], 2)
    return img, mask, kpt


def torch_chain(img, mask, theta, taps, f, mean, std):
    B = img.shape[0]
    x = img.permute(0, 3, 1, 2).float()
    grid = F.affine_grid(theta, (B, 3, H, W), align_corners=False)
    x = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    m = F.grid_sample(mask[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)
    x = F.conv2d(F.pad(x, (4, 4, 0, 0), mode="reflect"), taps.view(1, 1, 1, 9).expand(3, 1, 1, 9), groups=3)
    x = F.conv2d(F.pad(x, (0, 0, 4, 4), mode="reflect"), taps.view(1, 1, 9, 1).expand(3, 1, 9, 1), groups=3)
    luma = lambda t: (0.299 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2])[:, None]      # noqa: E731
    x = (x * f[:, 0].view(B, 1, 1, 1)).clamp(0, 255)
    grey = luma(x).mean((1, 2, 3), keepdim=True)
    x = (grey + f[:, 1].view(B, 1, 1, 1) * (x - grey)).clamp(0, 255)
    g = luma(x)
    x = (g + f[:, 2].view(B, 1, 1, 1) * (x - g)).clamp(0, 255)
    return (x / 255 - mean) / std, m[:, 0].to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    lines = []
    for B in (int(v) for v in a.batches.split(",")):
        rng = np.random.default_rng(B)
        img_h, mask_h, kpt_h = inputs(B, rng)
        d = twin.draws_for(B, 7)
        d[:, 4] = 0.1                                                               # every image is blurred: the dearer case
        t0 = time.perf_counter()
        n = min(B, 2)
        g_h = twin.pvnet_augment(img_h[:n], mask_h[:n], kpt_h[:n], (H, W), d[:n])
        inp_h = twin.pvnet_transform(g_h["img"], d[:n])
        twin_ms = (time.perf_counter() - t0) * 1e3 / n
        img, mask, kpt = torch.tensor(img_h, device=dev), torch.tensor(mask_h, device=dev), torch.tensor(kpt_h, device=dev)
        aug = augment.PVNetAugment()
        g = augment.pvnet_augment(img, mask, kpt, (H, W), d)
        out = aug(img, mask, kpt, H, W, draws=d)
        assert g["img"][:n].cpu().numpy().tobytes() == g_h["img"].tobytes() and out["inp"][:n].cpu().numpy().tobytes() == inp_h.tobytes(), \
            "the device differs from the twin"
        gp, jp = augment.geometry_params(d, (H, W), [-30.0, 30.0], [0.8, 1.2]), augment.jitter_params(d, 0.5, [0.1, 0.1, 0.05, 0.05])
        theta = torch.tensor(np.stack([np.array([[p["cos"] * p["ratio"], p["sin"] * p["ratio"] * H / W, 0.05],
                                                 [-p["sin"] * p["ratio"] * W / H, p["cos"] * p["ratio"], -0.03]]) for p in gp]),
                             dtype=torch.float32, device=dev)
        taps = torch.tensor(twin.blur_taps(9), dtype=torch.float32, device=dev) / 256
        f = torch.tensor(np.asarray(jp["f"]), device=dev)
        mean, std = torch.tensor(twin.MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(twin.STD, device=dev).view(1, 3, 1, 1)
        forms = {"device": lambda: [aug(img, mask, kpt, H, W, draws=d) for _ in range(a.reps)],
                 "augment": lambda: [augment.pvnet_augment(img, mask, kpt, (H, W), d) for _ in range(a.reps)],
                 "transform": lambda: [augment.pvnet_transform(g["img"], d, mean=twin.MEAN, std=twin.STD) for _ in range(a.reps)],
                 "torch_ops": lambda: [torch_chain(img, mask, theta, taps, f, mean, std) for _ in range(a.reps)]}
        ms = alternate(forms, a.rounds, a.warmup)
        res = {"B": B, "H": H, "W": W, "K": K, "out_size": [H, W], "paths": g["path"].cpu().tolist(), "rounds": a.rounds, "warmup": a.warmup,
               "reps": a.reps}
        for name in forms:
            res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
        res["twin_cpu_ms_per_image"] = round(twin_ms, 1)
        res["device_us_per_image"] = round(res["device_ms"]["median"] * 1e3 / B, 1)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
