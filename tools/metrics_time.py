#!/usr/bin/env python
"""Pose -> scores for a batch of a symmetric object (ADD-S search included), two ways, alternated in one process on the same
inputs and timed with device events after warm-up (ms per call, median and spread over the timed rounds):

  device   metrics.pose_metrics on the device poses: four launches on the stream, nothing read back;
  host     the only route there was: the poses copied to the host, then per image the numpy transforms,
           lib.csrc.nn.nn_utils.find_nearest_point_idx (three allocations, two copies in, one kernel, one copy out), the
           numpy norms and means -- the bodies of Evaluator.add_metric(syn=True) / projection_2d / cm_degree_5_metric.

A third form, ``--only nn``, is the existing batched search alone on the same float32 clouds through device pointers
(``pvv_nn_find_nearest``, no host traffic): run it and ``--only device`` each under
``rocprofv3 --kernel-trace --stats -- python tools/metrics_time.py --only ...`` to compare k_find_nearest with
k_adds_search + k_adds_merge kernel against kernel.  The model is a seeded synthetic cloud of LINEMOD size (5841 points).

    python tools/metrics_time.py [--batches 1,64] [--points 5841] [--rounds 20] [--warmup 5] [--only device|host|nn] [--slabs 0]
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
from clean_pvnet_amd import _native, metrics  # noqa: E402
from lib.csrc.nn.nn_utils import find_nearest_point_idx  # noqa: E402

KMAT = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])


def inputs(B, N, dev, seed=0):
    rng = np.random.RandomState(seed)
    model = (rng.randn(N, 3) * np.array([0.04, 0.03, 0.02])).astype(np.float32)

    def rot(w):
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    gt, pred = [], []
    for _ in range(B):
        R = rot(rng.uniform(-1, 1, 3))
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.0)])
        gt.append(np.concatenate([R, t.reshape(3, 1)], 1))
        pred.append(np.concatenate([rot(rng.randn(3) * 0.02) @ R, (t + rng.randn(3) * 0.004).reshape(3, 1)], 1))
    return (torch.tensor(np.stack(pred), device=dev), torch.tensor(np.stack(gt), device=dev), torch.tensor(model, device=dev),
            torch.tensor(KMAT, device=dev), model)


def device_form(Pp, Pg, md, Kt, slabs):
    return metrics.pose_metrics(Pp, Pg, md, Kt, symmetric=True, slabs=slabs)


def host_form(Pp, Pg, model):
    pp, pg = Pp.cpu().numpy(), Pg.cpu().numpy()                                           # copy + sync
    out = []
    for pose_pred, pose_targets in zip(pp, pg):
        model_pred = np.dot(model, pose_pred[:, :3].T) + pose_pred[:, 3]
        model_targets = np.dot(model, pose_targets[:, :3].T) + pose_targets[:, 3]
        idxs = find_nearest_point_idx(model_pred, model_targets)
        adds = np.mean(np.linalg.norm(model_pred[idxs] - model_targets, 2, 1))
        a = np.dot(model_pred, KMAT.T)
        b = np.dot(model_targets, KMAT.T)
        proj = np.mean(np.linalg.norm(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:], axis=-1))
        trans = np.linalg.norm(pose_pred[:, 3] - pose_targets[:, 3]) * 100
        trace = min(3.0, max(-1.0, np.trace(np.dot(pose_pred[:, :3], pose_targets[:, :3].T))))
        out.append((adds, proj, trans, np.rad2deg(np.arccos((trace - 1.) / 2.))))
    return out


def nn_form(nn, ref32, que32, idx, B, N):
    rc = nn.pvv_nn_find_nearest(ref32.data_ptr(), que32.data_ptr(), idx.data_ptr(), B, N, N, 3, 0,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--points", type=int, default=5841)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["device", "host", "nn"], default=None)
    ap.add_argument("--slabs", type=int, default=0, help="slab count of the ADD-S search; 0 lets the library choose")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    N = a.points
    nn = _native.load("metrics_time", "libpvnet_nn.so")
    for B in [int(s) for s in a.batches.split(",")]:
        Pp, Pg, md, Kt, model = inputs(B, N, dev)
        m64 = md.double()
        ref32 = (m64 @ Pp[:, :, :3].transpose(1, 2) + Pp[:, None, :, 3]).float().contiguous()      # [B,N,3] predicted clouds
        que32 = (m64 @ Pg[:, :, :3].transpose(1, 2) + Pg[:, None, :, 3]).float().contiguous()
        idx = torch.empty(B, N, dtype=torch.int32, device=dev)
        forms = {"device": lambda: device_form(Pp, Pg, md, Kt, a.slabs), "host": lambda: host_form(Pp, Pg, model)}
        if a.only == "nn":
            forms = {"nn": lambda: nn_form(nn, ref32, que32, idx, B, N)}
        elif a.only:
            forms = {a.only: forms[a.only]}
        ms = alternate(forms, a.rounds, a.warmup)
        res = {"B": B, "N": N, "rounds": a.rounds, "slabs": a.slabs or metrics.adds_slabs(B, N)}
        for name, v in ms.items():
            res[name + "_ms"] = summary(v, 4)
        if "device" in ms:                                     # a whole-call rate (four launches), not the search kernel's
            res["device_call_evals_per_s"] = float("%.4g" % (B * N * N / (np.median(ms["device"]) * 1e-3)))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
