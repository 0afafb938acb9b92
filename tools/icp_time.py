#!/usr/bin/env python
"""The ICP refinement for a batch at the T-LESS image size (720 x 540), timed with device events after warm-up (ms per call,
median and range over the timed rounds), the forms alternated in one process on the same inputs:

  refine      one stage (icp.refine, depth_only with factor 5.0): the render, the front passes, and the launch chain of
              max_iterations rounds of k_search + k_fit on the stream; nothing read back;
  icp_refine  the evaluators' two stages (icp.icp_refine);
  host        a lower bound on the host, not a measurement of the reference: the device render of each stage copied back (the
              host has no renderer here -- the reference's needs OpenGL -- so its render is NOT counted), then the numpy twin
              of the stage (tests/icp_twin.py) with its search replaced by scikit-learn's NearestNeighbors, as the reference
              uses it, when that is importable (``host_search`` in the output says which), else the twin's brute force.

The model is the seeded mesh of the fixtures; each sensor image is made from the ground-truth render of its pose, the start
is that pose perturbed.  Nothing is asserted.  ``--out`` writes the JSON lines to a file.

    python tools/icp_time.py [--shapes 1,16,64] [--rounds 20] [--warmup 3] [--host-rounds 1] [--only refine|icp_refine|host]
                             [--out profiles/icp_time.json]
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
from clean_pvnet_amd import icp as I  # noqa: E402
from clean_pvnet_amd import vsd as V  # noqa: E402
from tests import icp_twin as twin  # noqa: E402
from tests import vsd_twin as vt  # noqa: E402

SIZE = (720, 540)

try:
    from sklearn.neighbors import NearestNeighbors
    HOST_SEARCH = "sklearn"

    def _nearest(src, dst):
        d, j = NearestNeighbors(n_neighbors=1).fit(dst).kneighbors(src, return_distance=True)
        return j.ravel(), d.ravel() ** 2
except ImportError:
    HOST_SEARCH = "brute force"
    _nearest = twin.nearest


def inputs(P, dev, seed=0):
    rng = np.random.RandomState(seed)
    pts, faces = vt.mesh(5)
    gt = np.stack([vt.pose(rng.uniform(-1.5, 1.5, 3), [rng.uniform(-0.12, 0.12), rng.uniform(-0.08, 0.08), rng.uniform(0.65, 0.8)])
                   for _ in range(P)])
    est = np.stack([np.concatenate([vt.rodrigues(rng.randn(3) * 0.03) @ g[:, :3], (g[:, 3] + rng.randn(3) * [0.003, 0.003, 0.008]).reshape(3, 1)], 1)
                    for g in gt])
    K = vt.camera(1.0)
    t = {"pts": torch.tensor(pts, device=dev), "faces": torch.tensor(faces, device=dev), "K": torch.tensor(K, device=dev),
         "est": torch.tensor(est, device=dev), "est_mm": torch.tensor(vt.scaled(est, 1000.0), device=dev)}
    renders = V.render_depth(t["pts"], t["faces"], torch.tensor(vt.scaled(gt, 1000.0), device=dev), t["K"], SIZE).cpu().numpy()
    raw = np.stack([vt.scene_depth(100 + i, renders[i:i + 1]) for i in range(P)])
    t["raw"] = torch.from_numpy(raw).to(dev)
    t["mask"] = torch.from_numpy((renders > 0).astype(np.uint8)).to(dev)
    return t, pts, faces, K, raw, (renders > 0).astype(np.uint8), est


def host_form(t, pts, faces, K, raw, mask, est, g):
    saved = twin.nearest
    twin.nearest = _nearest
    try:
        words = torch.randint(0, 2 ** 32, (len(est), 2, 2, 3000), dtype=torch.int64, device=t["K"].device, generator=g).cpu().numpy()
        poses = vt.scaled(est, 1000.0)
        for stage, kw in enumerate((dict(depth_only=True, max_mean_dist_factor=5.0), dict(no_depth=True))):
            renders = V.render_depth(t["pts"], t["faces"], torch.tensor(poses, device=t["K"].device), t["K"], SIZE).cpu().numpy()   # copy + sync
            poses = np.stack([twin.refine(vt.sensor_depth(raw[p]), poses[p], K, pts, faces, SIZE, mask=mask[p], words=words[p, stage],
                                          render=renders[p], **kw)[0] for p in range(len(est))])
        return poses
    finally:
        twin.nearest = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1,16,64", help="P: poses per call, one image each")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=1, help="timed rounds of the host form (seconds per pose)")
    ap.add_argument("--host-max-poses", type=int, default=16, help="the host form is left out of larger shapes")
    ap.add_argument("--only", choices=["refine", "icp_refine", "host"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for shape in a.shapes.split(","):
        P = int(shape)
        t, pts, faces, K, raw, mask, est = inputs(P, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        info = {}

        def stage():
            out, i = I.refine(t["raw"], t["est_mm"], t["K"], t["pts"], t["faces"], mask=t["mask"], depth_only=True,
                              max_mean_dist_factor=5.0, depth_scale=0.1, generator=g, return_info=True)
            info["refine"] = i
            return out

        def both():
            out, (i1, i2) = I.icp_refine(t["est"], t["raw"], t["mask"], t["K"], t["pts"], t["faces"], generator=g, return_info=True)
            info["icp_refine"] = (i1, i2)
            return out

        forms = {"refine": stage, "icp_refine": both, "host": lambda: host_form(t, pts, faces, K, raw, mask, est, g)}
        if P > a.host_max_poses:
            del forms["host"]
        if a.only:
            forms = {a.only: forms[a.only]} if a.only in forms else {}
        # the host form only in the first host_rounds timed rounds and never in the warm-up: seconds per pose
        ms = alternate(forms, a.rounds, a.warmup, skip=lambda name, i: name == "host" and not a.warmup <= i < a.warmup + a.host_rounds)
        res = {"P": P, "size": list(SIZE), "triangles": int(t["faces"].shape[0]), "n_max": 3000, "max_iterations": 200,
               "rounds": a.rounds, "warmup": a.warmup, "host_rounds": min(a.host_rounds, a.rounds), "host_search": HOST_SEARCH,
               "host_note": "lower bound: the host's render is not counted"}
        for name, v in ms.items():
            if v:
                res[name + "_ms"] = summary(v, 4)
        if "refine" in info:
            res["refine_loop_rounds"] = info["refine"]["rounds"].cpu().tolist()
        if "icp_refine" in info:
            res["icp_refine_loop_rounds"] = [i["rounds"].cpu().tolist() for i in info["icp_refine"]]
            res["icp_refine_status"] = [i["status"].cpu().tolist() for i in info["icp_refine"]]
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
