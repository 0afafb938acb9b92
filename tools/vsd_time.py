#!/usr/bin/env python
"""Depth renders and VSD for a batch at the T-LESS image size (720 x 540), timed with device events after warm-up (ms per
call, median and range over the timed rounds), the forms alternated in one process on the same inputs:

  render   vsd.render_depth of the n*(p+g) poses of the batch: memset, k_vertices, k_raster, k_resolve on the stream;
  vsd      the whole vsd.vsd call: the same renders, then k_vsd and k_vsd_finish; nothing read back;
  host     the arithmetic alone as the host would do it: the device renders copied back, then per pair the numpy passes of
           tests/vsd_twin.py::vsd_pair (the reference's depth_im_to_dist_im, visibility masks and vsd).  The host has no
           renderer here (the reference's needs OpenGL), so its renders are not counted: this form is a lower bound on the
           host's time, not a measurement of the reference.

The model is the seeded mesh of the fixtures (tests/vsd_twin.py::mesh, 2306 triangles, or --subdiv for a finer one); the
sensor image is made once from the ground-truth renders.  Nothing is asserted.  ``--out`` writes the JSON lines to a file;
run ``--only render`` / ``--only vsd`` under ``rocprofv3 --kernel-trace --stats -- python tools/vsd_time.py --only ...`` for
per-kernel durations.

    python tools/vsd_time.py [--shapes 1x1x1,16x2x2] [--rounds 30] [--warmup 5] [--host-rounds 5] [--only render|vsd|host]
                             [--cost step] [--subdiv 48x24] [--out profiles/vsd_time.json]
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
from clean_pvnet_amd import vsd as V  # noqa: E402
from tests import vsd_twin as twin  # noqa: E402

SIZE = (720, 540)


def inputs(n, p, g, dev, mesh_args, seed=0):
    rng = np.random.RandomState(seed)
    pts, faces = twin.mesh(5, *mesh_args)
    gt = np.stack([[twin.pose(rng.uniform(-1.5, 1.5, 3), [rng.uniform(-0.12, 0.12), rng.uniform(-0.08, 0.08), rng.uniform(0.65, 0.8)])
                    for _ in range(g)] for _ in range(n)])
    est = np.stack([[np.concatenate([twin.rodrigues(rng.randn(3) * 0.03) @ gt[i, a % g][:, :3],
                                     (gt[i, a % g][:, 3] + rng.randn(3) * 0.003).reshape(3, 1)], 1) for a in range(p)] for i in range(n)])
    K = twin.camera(1.0)
    t = {"pts": torch.tensor(pts, device=dev), "faces": torch.tensor(faces, device=dev), "K": torch.tensor(K, device=dev),
         "est": torch.tensor(est, device=dev), "gt": torch.tensor(gt, device=dev)}
    renders = V.render_depth(t["pts"], t["faces"], torch.tensor(twin.scaled(gt, 1000.0).reshape(-1, 3, 4), device=dev), t["K"],
                             SIZE).cpu().numpy().reshape(n, g, SIZE[1], SIZE[0])
    raw = np.stack([twin.scene_depth(100 + i, renders[i]) for i in range(n)])
    t["raw"] = torch.from_numpy(raw).to(dev)
    t["poses"] = torch.tensor(np.concatenate([twin.scaled(est, 1000.0).reshape(-1, 3, 4), twin.scaled(gt, 1000.0).reshape(-1, 3, 4)]),
                              device=dev)
    return t, K, raw


def host_form(t, K, raw, n, p, g, cost):
    depth = V.render_depth(t["pts"], t["faces"], t["poses"], t["K"], SIZE).cpu().numpy()            # copy + sync
    est, gt = depth[:n * p].reshape(n, p, SIZE[1], SIZE[0]), depth[n * p:].reshape(n, g, SIZE[1], SIZE[0])
    out = []
    for i in range(n):
        d = twin.sensor_depth(raw[i])
        for a in range(p):
            for b in range(g):
                out.append(twin.vsd_pair(est[i, a], gt[i, b], d, K, cost=cost)["e"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1x1,16x2x2", help="n x p x g: images, predictions and ground truths per image")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=5, help="timed rounds of the host form (seconds per round at 16x2x2)")
    ap.add_argument("--only", choices=["render", "vsd", "host"], default=None)
    ap.add_argument("--cost", choices=["step", "tlinear"], default="step")
    ap.add_argument("--subdiv", default="48x24", help="torus grid nu x nv of the mesh: 2*nu*nv + 2 triangles")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mesh_args = tuple(int(v) for v in a.subdiv.split("x"))
    lines = []
    for shape in a.shapes.split(","):
        n, p, g = (int(v) for v in shape.split("x"))
        t, K, raw = inputs(n, p, g, dev, mesh_args)
        forms = {"render": lambda: V.render_depth(t["pts"], t["faces"], t["poses"], t["K"], SIZE),
                 "vsd": lambda: V.vsd(t["est"], t["gt"], t["raw"], t["K"], t["pts"], t["faces"], cost=a.cost),
                 "host": lambda: host_form(t, K, raw, n, p, g, a.cost)}
        if a.only:
            forms = {a.only: forms[a.only]}
        # the host form only in the first host_rounds timed rounds: seconds per round at 16x2x2
        ms = alternate(forms, a.rounds, a.warmup, skip=lambda name, i: name == "host" and i >= a.warmup + a.host_rounds)
        res = {"n": n, "p": p, "g": g, "size": list(SIZE), "triangles": int(t["faces"].shape[0]), "renders": n * (p + g),
               "pairs": n * p * g, "cost": a.cost, "rounds": a.rounds, "warmup": a.warmup,
               "host_rounds": min(a.host_rounds, a.rounds)}
        for name, v in ms.items():
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
