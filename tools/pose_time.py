#!/usr/bin/env python
"""Network output -> pose for a batch, two ways, alternated in one process and timed with device events after warm-up
(ms per call, median and spread over the timed rounds):

  device   decode_keypoint(un_pnp=True, weights=True) + pose.solve_pose(un_pnp=True): the start and the refinement in one
           launch on the stream, no host round trip;
  host     the same decode, then the only way there was to get a start: kpt_2d / var_weights copied to the host and
           un_pnp_utils.initial_pose_p3p (DLT fallback) per image, the starts copied back, uncertainty_pnp_batched.

Inputs are vote fields rendered from known poses of a 9-keypoint model (480 x 640, the LINEMOD camera), so the P3P path
runs as on real frames.  Kernel time is not taken here: run the device form alone under
``rocprofv3 --kernel-trace --stats -- python tools/pose_time.py --only device`` for that.

    python tools/pose_time.py [--batches 1,64] [--rounds 20] [--warmup 5] [--only device|host]
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
from clean_pvnet_amd.decode import decode_keypoint  # noqa: E402
from clean_pvnet_amd.pose import solve_pose  # noqa: E402
from clean_pvnet_amd.un_pnp_utils import initial_pose_dlt, initial_pose_p3p, uncertainty_pnp_batched  # noqa: E402

KMAT = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])


def rendered(B, dev, H=480, W=640, K=9, seed=0):
    """Logits + unit vectors towards the projected keypoints of a random pose per image, with noise."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(-0.05, 0.05, (K, 3))
    kp = []
    for _ in range(B):
        w = rng.uniform(-1, 1, 3)
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        X = P @ R.T + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(0.5, 0.7)])
        kp.append(np.stack([KMAT[0, 0] * X[:, 0] / X[:, 2] + KMAT[0, 2], KMAT[1, 1] * X[:, 1] / X[:, 2] + KMAT[1, 2]], 1))
    kp = torch.tensor(np.stack(kp), dtype=torch.float32, device=dev)                       # [B,K,2]
    ys = torch.arange(H, dtype=torch.float32, device=dev).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, 1, W)
    c = kp.mean(1)
    inside = ((xs[:, 0] - c[:, 0, None, None]) ** 2 + (ys[:, 0] - c[:, 1, None, None]) ** 2) <= 60.0 ** 2   # [B,H,W]
    g = torch.Generator(device=dev).manual_seed(seed)
    dx = kp[:, :, 0, None, None] - xs
    dy = kp[:, :, 1, None, None] - ys
    n = torch.sqrt(dx * dx + dy * dy).clamp(min=1e-3)
    vx = dx / n + 0.03 * torch.randn(dx.shape, device=dev, generator=g)
    vy = dy / n + 0.03 * torch.randn(dy.shape, device=dev, generator=g)
    x = torch.empty(B, 2 + 2 * K, H, W, device=dev)
    x[:, 0] = 0.0
    x[:, 1] = torch.where(inside, 4.0, -4.0)
    x[:, 2::2] = vx
    x[:, 3::2] = vy
    return x, torch.tensor(P, device=dev), torch.tensor(KMAT, device=dev), P


def device_form(x, Pt, Kt, i):
    o = decode_keypoint({"seg": x[:, :2], "vertex": x[:, 2:]}, un_pnp=True, weights=True, seed=7 + i)
    return solve_pose(o, Pt, Kt, un_pnp=True)["pose"]


def host_form(x, Pt, Kt, P, i):
    o = decode_keypoint({"seg": x[:, :2], "vertex": x[:, 2:]}, un_pnp=True, weights=True, seed=7 + i)
    kp = o["kpt_2d"].double().cpu().numpy()                                               # copy + sync
    wt = o["var_weights"].double().cpu().numpy()
    starts = []
    for b in range(kp.shape[0]):                                                           # the host twin per image
        key = wt[b, :, 0] + wt[b, :, 1]
        rt = initial_pose_p3p(P, kp[b], KMAT, key)
        starts.append(rt if rt is not None else initial_pose_dlt(P, kp[b], KMAT, key))
    init = torch.tensor(np.stack(starts), device=x.device)
    return uncertainty_pnp_batched(o["kpt_2d"], o["var_weights"], Pt, Kt, init)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["device", "host"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for B in [int(s) for s in a.batches.split(",")]:
        x, Pt, Kt, P = rendered(B, dev)
        forms = {"device": lambda i: device_form(x, Pt, Kt, i), "host": lambda i: host_form(x, Pt, Kt, P, i)}
        if a.only:
            forms = {a.only: forms[a.only]}
        ms = alternate(forms, a.rounds, a.warmup)
        res = {"B": B, "rounds": a.rounds}
        for name, v in ms.items():
            res[name + "_ms"] = summary(v, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
