#!/usr/bin/env python
"""Generate tests/golden/vsd_*.npz by running THE REFERENCE'S OWN VSD functions on the CPU.

``lib/utils/vsd/misc.py``, ``visibility.py`` and ``vsd_utils.py`` are imported from where they lie under /root/reference
(never copied), as submodules of a stub package whose ``renderer`` is an empty module: the reference renders through OpenGL,
which does not exist here, so the depth images come from the numpy twin of the rasteriser's contract
(tests/vsd_twin.py::render_depth).  ``misc.depth_im_to_dist_im``, ``visibility.estimate_visib_mask_gt`` / ``_est`` and
``vsd_utils.vsd`` then run on them exactly as ``Evaluator.vsd_metric`` (lib/evaluators/tless_test/pvnet.py:66-105) calls
them, with ``tless_config``'s delta = 15, tau = 20 and both cost types.

Stored per fixture: the seeds of the mesh and of the sensor images (the tests regenerate both, vsd_twin.regenerate), the
poses (translations in metres, as the evaluator holds them), the camera, the image size and the parameters; the reference's
``e`` for 'step' and 'tlinear', the three counts of every pair, the 'tlinear' cost sum, and the visibility masks as
``np.packbits``.  Asserted while writing: the twin's distance image equals the reference's ``np.linalg.norm(np.dstack(...))``
bit for bit for the sensor image and for every render, and no stored ``e`` lies within 1e-6 relative of the threshold 0.3.

``vsd_rules.npz`` (``make_rules``) holds constructed images instead of seeds: vsd_twin.rules_images(), whose differences lie
exactly on delta and tau and one float32 step to either side, under a camera for which distance equals depth (asserted).

Run from the repository root in the build container:  python tests/golden/make_vsd_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference/lib/utils/vsd"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import vsd_twin as twin  # noqa: E402

DELTA, TAU, THRESH = 15.0, 20.0, 0.3            # tless_config.vsd_delta, vsd_tau, error_thresh_vsd


def load_reference():
    pkg = types.ModuleType("ref_vsd")
    pkg.__path__ = []
    sys.modules["ref_vsd"] = pkg
    sys.modules["ref_vsd.renderer"] = pkg.renderer = types.ModuleType("ref_vsd.renderer")
    mods = {}
    for leaf in ("misc", "visibility", "vsd_utils"):
        spec = importlib.util.spec_from_file_location("ref_vsd." + leaf, os.path.join(REF, leaf + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_vsd." + leaf] = mod
        setattr(pkg, leaf, mod)
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods["misc"], mods["visibility"], mods["vsd_utils"]


def _near(P, dw, dt):
    return np.concatenate([twin.rodrigues(dw) @ P[:, :3], (P[:, 3] + np.asarray(dt)).reshape(3, 1)], 1)


def definitions():
    """name -> the inputs of a fixture (poses in metres)."""
    g0 = twin.pose([0.9, 0.4, -0.3], [-0.09, 0.02, 0.70])
    g1 = twin.pose([-0.5, 1.1, 0.6], [0.10, -0.03, 0.78])
    big = dict(mesh_seed=5, scene_seed=[51], size=(720, 540), K=twin.camera(1.0),
               pose_gt=[[g0, g1]],
               pose_est=[[_near(g0, [0.02, -0.01, 0.015], [0.001, -0.0015, 0.002]),          # close to g0
                          twin.pose([1.8, -0.7, 0.2], [0.16, 0.03, 0.74])]])                 # far off: e near 1
    h0 = twin.pose([0.3, -0.8, 0.5], [-0.03, 0.01, 0.66])
    h1 = twin.pose([1.2, 0.2, -0.9], [0.04, 0.00, 0.74])                                     # partly behind h0
    away = twin.pose([0.1, 0.2, 0.3], [2.0, 0.0, 0.70])                                      # outside the image: empty render
    half = dict(mesh_seed=6, scene_seed=[61, 62], size=(360, 270), K=twin.camera(0.5),
                pose_gt=[[h0, h1], [g0, away]],
                pose_est=[[_near(h0, [0.10, 0.05, -0.08], [0.006, 0.004, 0.010]), _near(h1, [0.01, 0.0, 0.01], [0.0, 0.001, 0.001])],
                          [_near(g0, [0.0, 0.03, 0.0], [0.002, 0.0, -0.003]), _near(away, [0.1, 0.0, 0.0], [0.1, 0.0, 0.0])]])
    c0 = twin.pose([0.4, 0.3, 0.1], [0.005, -0.004, 0.130])                                  # Z from 45 to 215 mm: straddles near
    close = dict(mesh_seed=7, scene_seed=[71], size=(240, 180), K=twin.camera(1.0 / 3.0, skew=0.7),
                 pose_gt=[[c0]], pose_est=[[_near(c0, [0.03, 0.0, -0.02], [0.001, 0.001, 0.002])]])
    return {"vsd_720": big, "vsd_360": half, "vsd_near": close}


def make(name, d, misc, visibility, vsd_utils):
    c = dict(mesh_seed=d["mesh_seed"], scene_seed=np.array(d["scene_seed"]), size=np.array(d["size"]), K=d["K"],
             pose_est=np.array(d["pose_est"]), pose_gt=np.array(d["pose_gt"]), t_scale=1000.0, depth_scale=0.1,
             delta=DELTA, tau=TAU, near=100.0, far=10000.0, error_thresh=THRESH)
    r = twin.regenerate(name, c)
    n, p = c["pose_est"].shape[:2]
    g = c["pose_gt"].shape[1]
    K = c["K"]
    e = {"step": np.zeros((n, p, g)), "tlinear": np.zeros((n, p, g))}
    counts = np.zeros((n, p, g, 3), np.int64)
    cost_sum = np.zeros((n, p, g))
    bits_gt, bits_est = [], []
    for i in range(n):
        depth = r["raw"][i].astype(np.float64) * 0.1                                # load_depth(path) * 0.1, in binary64
        dist_test = misc.depth_im_to_dist_im(depth, K)
        assert np.array_equal(dist_test, twin.dist_image(depth, K))
        dist_gt, visib_gt = {}, {}
        for b in range(g):                                                          # tless_test/pvnet.py:92-98
            dist_gt[b] = misc.depth_im_to_dist_im(r["gt"][i, b], K)
            assert np.array_equal(dist_gt[b], twin.dist_image(r["gt"][i, b], K))
            visib_gt[b] = visibility.estimate_visib_mask_gt(dist_test, dist_gt[b], DELTA)
            bits_gt.append(np.packbits(visib_gt[b]))
        for a in range(p):
            dist_est = misc.depth_im_to_dist_im(r["est"][i, a], K)
            assert np.array_equal(dist_est, twin.dist_image(r["est"][i, a], K))
            for b in range(g):
                for cost in ("step", "tlinear"):
                    e[cost][i, a, b] = vsd_utils.vsd(dist_est, dist_gt[b], dist_test, visib_gt[b], DELTA, TAU, cost)
                    assert abs(e[cost][i, a, b] - THRESH) > 1e-6 * THRESH, (name, i, a, b, cost)
                visib_est = visibility.estimate_visib_mask_est(dist_test, dist_est, visib_gt[b], DELTA)
                inter = np.logical_and(visib_gt[b], visib_est)
                costs = np.abs(dist_gt[b][inter] - dist_est[inter])
                counts[i, a, b] = (np.logical_or(visib_gt[b], visib_est).sum(), inter.sum(), (costs >= TAU).sum())
                costs *= (1.0 / TAU)
                costs[costs > 1.0] = 1.0
                cost_sum[i, a, b] = costs.sum()
                bits_est.append(np.packbits(visib_est))
    c.update(e_step=e["step"], e_tlinear=e["tlinear"], counts=counts, cost_sum=cost_sum,
             visib_gt_bits=np.stack(bits_gt).reshape(n, g, -1), visib_est_bits=np.stack(bits_est).reshape(n, p, g, -1))
    return c


def make_rules(misc, visibility, vsd_utils):
    """vsd_rules: the constructed images of vsd_twin.rules_images() -- differences exactly on, one float32 step below and
    one above delta and tau, invalid pixels, a partial tile -- through the same reference functions as ``make``.  The
    images themselves are stored (a few kilobytes); keys are ``<case>_<what>``."""
    K = twin.RULES_K
    c = dict(K=K, delta=twin.RULES_DELTA, tau=twin.RULES_TAU, cases=np.array(sorted(twin.rules_images())))
    for name, (depth, gt, est) in twin.rules_images().items():
        g, p = len(gt), len(est)
        dist_test = misc.depth_im_to_dist_im(depth, K)
        assert np.array_equal(dist_test, twin.dist_image(depth, K)) and np.array_equal(dist_test, depth)
        e = {"step": np.zeros((p, g)), "tlinear": np.zeros((p, g))}
        counts = np.zeros((p, g, 3), np.int64)
        cost_sum = np.zeros((p, g))
        dist_gt, visib_gt, bits_gt, bits_est = {}, {}, [], []
        for b in range(g):
            dist_gt[b] = misc.depth_im_to_dist_im(gt[b], K)
            assert np.array_equal(dist_gt[b], twin.dist_image(gt[b], K)) and np.array_equal(dist_gt[b], gt[b].astype(np.float64))
            visib_gt[b] = visibility.estimate_visib_mask_gt(dist_test, dist_gt[b], twin.RULES_DELTA)
            bits_gt.append(np.packbits(visib_gt[b]))
        for a in range(p):
            dist_est = misc.depth_im_to_dist_im(est[a], K)
            assert np.array_equal(dist_est, twin.dist_image(est[a], K)) and np.array_equal(dist_est, est[a].astype(np.float64))
            for b in range(g):
                for cost in ("step", "tlinear"):
                    e[cost][a, b] = vsd_utils.vsd(dist_est, dist_gt[b], dist_test, visib_gt[b], twin.RULES_DELTA, twin.RULES_TAU,
                                                  cost)
                visib_est = visibility.estimate_visib_mask_est(dist_test, dist_est, visib_gt[b], twin.RULES_DELTA)
                inter = np.logical_and(visib_gt[b], visib_est)
                costs = np.abs(dist_gt[b][inter] - dist_est[inter])
                counts[a, b] = (np.logical_or(visib_gt[b], visib_est).sum(), inter.sum(), (costs >= twin.RULES_TAU).sum())
                costs *= (1.0 / twin.RULES_TAU)
                costs[costs > 1.0] = 1.0
                cost_sum[a, b] = costs.sum()
                bits_est.append(np.packbits(visib_est))
        c.update({name + "_test": depth, name + "_gt": gt, name + "_est": est, name + "_e_step": e["step"],
                  name + "_e_tlinear": e["tlinear"], name + "_counts": counts, name + "_cost_sum": cost_sum,
                  name + "_visib_gt_bits": np.stack(bits_gt), name + "_visib_est_bits": np.stack(bits_est).reshape(p, g, -1)})
    return c


def main():
    misc, visibility, vsd_utils = load_reference()
    made = [(name, make(name, d, misc, visibility, vsd_utils)) for name, d in definitions().items()]
    made.append(("vsd_rules", make_rules(misc, visibility, vsd_utils)))
    for name, c in made:
        for k in sorted(c):
            if k.endswith("e_step"):
                print(name, k, np.round(c[k], 4).tolist(), "e_tlinear", np.round(c[k.replace("e_step", "e_tlinear")], 4).tolist(),
                      "union", c[k.replace("e_step", "counts")][..., 0].tolist())
        path = os.path.join(OUT, name + ".npz")
        if os.path.exists(path) and "--force" not in sys.argv:       # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v)) for k, v in c.items())
            print(name, "exists,", "identical content" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, "written,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
