#!/usr/bin/env python
"""``clean_pvnet_amd.render.render_color`` timed with device events after warm-up (ms per batch, median and range over the timed
rounds; each round is ``--reps`` calls back to back), legs alternated in one process on the same inputs -> profiles/render_time.json.

At 640x480, B = 32, on a torus of about 5.8 k vertices (the LINEMOD model size) at seeded poses around 400 mm:

  color_m1      ``render_color`` with one instance per image
  color_m4      ``render_color`` with four instances per image (the first is color_m1's)
  depth         ``vsd.render_depth`` on the same mesh and the poses of color_m1: the yardstick -- the same raster work without the
                shading pass, the labels and the 8-byte keys
  depth_m4      ``vsd.render_depth`` at the 128 poses of color_m4 (four images where color_m4 writes one)

The colour render's depth is compared with the depth render's as bit patterns on the whole batch before anything is timed.  No
time is a pass criterion anywhere; this is for whoever has the card.

    python tools/render_time.py [--batch 32] [--rounds 20] [--warmup 3] [--reps 3] [--out profiles/render_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import render, vsd  # noqa: E402
from tests import render_twin as twin  # noqa: E402
from tests import vsd_twin  # noqa: E402

W, H = 640, 480
NEAR, FAR = 100.0, 10000.0


def poses(B, M, rng):
    """[B,M,3,4]: seeded rotations, the translations spread over the image at 350 to 500 mm."""
    out = np.empty((B, M, 3, 4))
    for b in range(B):
        for m in range(M):
            out[b, m] = vsd_twin.pose(rng.uniform(-1.5, 1.5, 3), [rng.uniform(-90, 90), rng.uniform(-60, 60), rng.uniform(350, 500)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    B = a.batch
    pts_h, faces_h = vsd_twin.mesh(1, nu=108, nv=54)                               # 5833 vertices, 11666 faces
    K_h = vsd_twin.camera(W / 720.0)
    p4_h = poses(B, 4, np.random.default_rng(5))
    pts, faces, K = torch.tensor(pts_h, device=dev), torch.tensor(faces_h, device=dev), torch.tensor(K_h, device=dev)
    colors = torch.tensor(twin.vertex_colors(1, len(pts_h)), device=dev)
    p4 = torch.tensor(p4_h, device=dev)
    p1 = p4[:, :1].contiguous()
    flat1, flat4 = p1.reshape(B, 3, 4).contiguous(), p4.reshape(B * 4, 3, 4).contiguous()
    kw = dict(near=NEAR, far=FAR)
    c1 = render.render_color(pts, colors, faces, p1, K, (W, H), **kw)
    d1 = vsd.render_depth(pts, faces, flat1, K, (W, H), NEAR, FAR)
    assert torch.equal(c1["depth"].view(torch.int32), d1.view(torch.int32)), "the colour render's depth differs from the depth render's"
    c4 = render.render_color(pts, colors, faces, p4, K, (W, H), **kw)
    covered = {"m1": round(float((c1["label"] > 0).float().mean()), 4), "m4": round(float((c4["label"] > 0).float().mean()), 4)}
    forms = {"color_m1": lambda: [render.render_color(pts, colors, faces, p1, K, (W, H), **kw) for _ in range(a.reps)],
             "color_m4": lambda: [render.render_color(pts, colors, faces, p4, K, (W, H), **kw) for _ in range(a.reps)],
             "depth": lambda: [vsd.render_depth(pts, faces, flat1, K, (W, H), NEAR, FAR) for _ in range(a.reps)],
             "depth_m4": lambda: [vsd.render_depth(pts, faces, flat4, K, (W, H), NEAR, FAR) for _ in range(a.reps)]}
    ms = alternate(forms, a.rounds, a.warmup)
    res = {"B": B, "size": [W, H], "vertices": int(len(pts_h)), "faces": int(len(faces_h)), "covered_fraction": covered, "rounds": a.rounds,
           "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name in forms:
        res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
    res["color_m1_over_depth"] = round(res["color_m1_ms"]["median"] / res["depth_ms"]["median"], 2)
    res["color_m4_over_depth_m4"] = round(res["color_m4_ms"]["median"] / res["depth_m4_ms"]["median"], 2)
    res["color_m1_us_per_image"] = round(res["color_m1_ms"]["median"] * 1e3 / B, 1)
    res["color_m4_us_per_image"] = round(res["color_m4_ms"]["median"] * 1e3 / B, 1)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump([res], fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
