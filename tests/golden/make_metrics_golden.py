#!/usr/bin/env python
"""Generate tests/golden/metrics_*.npz by running THE REFERENCE'S OWN evaluator methods on the CPU.

``lib/evaluators/linemod/pvnet.py`` and ``lib/utils/pvnet/pvnet_pose_utils.py`` are imported from where they lie under
/root/reference (never copied).  Their module-level imports that do not exist here are served by empty stub modules
(``cv2`` with the three SOLVEPNP_* constants, ``lib.config`` with ``cfg.test.icp = un_pnp = False``, ``pycocotools.coco``,
``PIL.Image``, ``transforms3d.quaternions``, ``lib.datasets.dataset_catalog``, ``lib.utils.img_utils``,
``lib.utils.vsd.inout``, ``lib.utils.linemod.linemod_config``, ``lib.utils.pvnet.pvnet_data_utils``), and
``lib.csrc.nn.nn_utils.find_nearest_point_idx`` -- a CUDA library in the reference -- by the CPU restatement of that search
in oracle/vote_oracle.c, which casts to float32 as the real wrapper does.  ``Evaluator.add_metric``, ``.projection_2d``,
``.cm_degree_5_metric`` and ``.mask_iou`` then run unbound on a ``types.SimpleNamespace`` that carries the model, the
diameter and the result lists.

Stored per model size: the cloud's seed (the tests regenerate the cloud, tests/metrics_twin.py::cloud), the camera, the
diameter, the pose pairs, the booleans the methods appended, the values they compared (the last ``np.mean`` of
``add_metric`` / ``projection_2d``, captured by wrapping ``np.mean`` for the duration of the call, and
``pvnet_pose_utils.cm_degree_5``'s return) and the neighbour indices the search stub returned.  Two conditions are asserted
while writing: for every pair the float32 roundings of ``np.dot(model, R.T) + t`` equal those of the explicit-order binary64
form of include/pvnet_metrics.h and the neighbour indices of the two agree (a pair that fails is drawn again from another
seed), and no stored value lies within 1e-6 relative of the threshold it is compared with.

Run from the repository root in the build container:  python tests/golden/make_metrics_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

from oracle import vote_oracle  # noqa: E402
from tests import metrics_twin as twin  # noqa: E402

asked = []            # the indices the search stub returned, in call order


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, mod)
    return mod


def load_reference():
    def find_nearest_point_idx(ref_pts, que_pts):
        idx = vote_oracle.find_nearest_point_idx(np.asarray(ref_pts), np.asarray(que_pts))
        asked.append(idx.copy())
        return idx

    _stub("cv2", SOLVEPNP_ITERATIVE=0, SOLVEPNP_EPNP=1, SOLVEPNP_P3P=2)
    for pkg in ("lib", "lib.datasets", "lib.utils", "lib.utils.pvnet", "lib.utils.linemod", "lib.utils.vsd", "lib.csrc",
                "lib.csrc.nn", "pycocotools", "PIL", "transforms3d"):
        _stub(pkg)
    _stub("lib.datasets.dataset_catalog", DatasetCatalog=None)
    _stub("lib.config", cfg=types.SimpleNamespace(test=types.SimpleNamespace(icp=False, un_pnp=False)))
    _stub("pycocotools.coco")
    _stub("lib.utils.pvnet.pvnet_data_utils")
    _stub("lib.utils.linemod.linemod_config")
    _stub("PIL.Image")
    _stub("lib.utils.img_utils", read_depth=None)
    _stub("lib.utils.vsd.inout")
    _stub("transforms3d.quaternions", mat2quat=None, quat2mat=None)
    _stub("lib.csrc.nn.nn_utils", find_nearest_point_idx=find_nearest_point_idx)
    utils = _load("lib.utils.pvnet.pvnet_pose_utils", os.path.join(REF, "lib/utils/pvnet/pvnet_pose_utils.py"))
    ev = _load("ref_linemod_evaluator", os.path.join(REF, "lib/evaluators/linemod/pvnet.py"))
    return ev.Evaluator, utils


def _namespace(model, diameter):
    return types.SimpleNamespace(model=model, diameter=diameter, add=[], proj2d=[], cmd5=[], mask_ap=[], icp_add=[],
                                 icp_proj2d=[], icp_cmd5=[])


def _last_mean(fn, *a, **kw):
    """Run ``fn`` with ``np.mean`` wrapped; return the value of its last ``np.mean`` call."""
    seen = []
    orig = np.mean

    def mean(*x, **k):
        r = orig(*x, **k)
        seen.append(r)
        return r
    np.mean = mean
    try:
        fn(*a, **kw)
    finally:
        np.mean = orig
    return float(seen[-1])


def _far(value, threshold):
    return abs(value - threshold) > 1e-6 * abs(threshold)


def _bisect(f, target, lo, hi, iters=40):
    """The s in [lo, hi] with f(s) = target, f increasing."""
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if f(mid) < target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _blas_agrees(model, P):
    """Condition 1 for one pose: float32(np.dot form) == float32(explicit-order form), element for element."""
    a = (np.dot(model, P[:, :3].T) + P[:, 3]).astype(np.float32)
    b = twin.transform(model, P).astype(np.float32)
    return np.array_equal(a, b)


def pairs_for(model, K, diameter, seed):
    """(name, ground truth, prediction) triples; thresholds are met by bisection on the size of the error."""
    rng = np.random.RandomState(seed)

    def gt():
        return twin.pose(rng.uniform(-1, 1, 3), [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.0)])

    def perturbed(G, dw, dt):
        return np.concatenate([twin.rodrigues(dw) @ G[:, :3], (G[:, 3] + dt).reshape(3, 1)], 1)

    def unit():
        v = rng.randn(3)
        return v / np.linalg.norm(v)

    out = []
    G = gt()
    out.append(("identical", G, G.copy()))
    for e in (0.002, 0.02, 0.2):
        G = gt()
        out.append(("err_%g" % e, G, perturbed(G, unit() * e, unit() * e * 0.3)))
    search = vote_oracle.find_nearest_point_idx
    thr_add = diameter * 0.1
    for name, key, thr, sym in (("add", "add", thr_add, False), ("adds", "adds", thr_add, True), ("proj2d", "proj2d", 5.0, False)):
        G, w, d = gt(), unit(), unit()
        f = lambda s: twin.pose_metrics(perturbed(G, w * s, d * s * 0.3), G, model, K, symmetric=sym, search=search)[key]  # noqa: E731
        s = _bisect(f, thr, 0.0, 1.0)
        out.append((name + "_inside", G, perturbed(G, w * s * 0.97, d * s * 0.97 * 0.3)))
        out.append((name + "_outside", G, perturbed(G, w * s * 1.03, d * s * 1.03 * 0.3)))
    G, d = gt(), unit()
    out.append(("trans_inside", G, perturbed(G, np.zeros(3), d * 0.0485)))
    out.append(("trans_outside", G, perturbed(G, np.zeros(3), d * 0.0515)))
    G, w = gt(), unit()
    out.append(("ang_inside", G, perturbed(G, w * np.deg2rad(4.85), np.zeros(3))))
    out.append(("ang_outside", G, perturbed(G, w * np.deg2rad(5.15), np.zeros(3))))
    G = gt()
    out.append(("rot180", G, np.concatenate([G[:, :3] @ np.diag([1.0, -1.0, -1.0]), G[:, 3:]], 1)))
    G = gt()
    out.append(("nan_prediction", G, np.full((3, 4), np.nan)))
    return out


def pose_case(Evaluator, utils, n, cloud_seed, diameter):
    model = twin.cloud(n, cloud_seed)
    K = twin.LINEMOD_K
    for seed in range(1000 * cloud_seed, 1000 * cloud_seed + 50):          # condition 1: draw again until every pair passes
        pairs = pairs_for(model, K, diameter, seed)
        ok = True
        for name, G, P in pairs:
            if not np.isfinite(P).all():
                continue
            if not (_blas_agrees(model, G) and _blas_agrees(model, P)):
                ok = False
                break
            a = vote_oracle.find_nearest_point_idx(np.dot(model, P[:, :3].T) + P[:, 3], np.dot(model, G[:, :3].T) + G[:, 3])
            b = vote_oracle.find_nearest_point_idx(twin.transform(model, P).astype(np.float32),
                                                   twin.transform(model, G).astype(np.float32))
            if not np.array_equal(a, b):
                ok = False
                break
        if ok:
            break
        print("n=%d: pair seed %d fails the BLAS-agreement condition at %s, drawing again" % (n, seed, name))
    else:
        raise SystemExit("no pair seed passed condition 1")
    c = dict(n=n, cloud_seed=cloud_seed, pair_seed=seed, K=K, diameter=diameter, names=np.array([p[0] for p in pairs]),
             pose_gt=np.stack([p[1] for p in pairs]), pose_pred=np.stack([p[2] for p in pairs]))
    vals = {k: [] for k in ("add", "adds", "proj2d", "trans_cm", "ang_deg")}
    ns, ns_sym = _namespace(model, diameter), _namespace(model, diameter)
    asked.clear()
    with np.errstate(all="ignore"):
        for name, G, P in pairs:
            vals["add"].append(_last_mean(Evaluator.add_metric, ns, P, G))
            vals["adds"].append(_last_mean(Evaluator.add_metric, ns_sym, P, G, syn=True))
            vals["proj2d"].append(_last_mean(Evaluator.projection_2d, ns, P, G, K))
            Evaluator.cm_degree_5_metric(ns, P, G)
            t, a = utils.cm_degree_5(P, G)
            vals["trans_cm"].append(float(t))
            vals["ang_deg"].append(float(a))
    assert len(asked) == len(pairs)
    c["adds_idx"] = np.stack(asked).astype(np.int32)
    for k, v in vals.items():
        c[k] = np.array(v, np.float64)
    c["hit_add"] = np.array(ns.add, bool)
    c["hit_adds"] = np.array(ns_sym.add, bool)
    c["hit_proj2d"] = np.array(ns.proj2d, bool)
    c["hit_cmd5"] = np.array(ns.cmd5, bool)
    # condition 2: every boolean is decided
    for i, (name, _G, _P) in enumerate(pairs):
        if not np.isfinite(c["pose_pred"][i]).all():
            continue
        assert _far(c["add"][i], diameter * 0.1) and _far(c["adds"][i], diameter * 0.1), name
        assert _far(c["proj2d"][i], 5.0) and _far(c["trans_cm"][i], 5.0) and _far(c["ang_deg"][i], 5.0), name
    # and the cases are what their names say
    hit = {nm: i for i, nm in enumerate(c["names"])}
    for key, arr in (("add", c["hit_add"]), ("adds", c["hit_adds"]), ("proj2d", c["hit_proj2d"])):
        assert arr[hit[key + "_inside"]] and not arr[hit[key + "_outside"]], key
    for key in ("trans", "ang"):
        assert c["hit_cmd5"][hit[key + "_inside"]] and not c["hit_cmd5"][hit[key + "_outside"]], key
    assert abs(c["ang_deg"][hit["rot180"]] - 180.0) < 1e-5
    assert not (c["hit_add"][-1] or c["hit_adds"][-1] or c["hit_proj2d"][-1] or c["hit_cmd5"][-1])
    return c


def mask_case(Evaluator):
    """seg logits / ground-truth masks through Evaluator.mask_iou, one image per call as the reference does."""
    rng = np.random.RandomState(31)
    H, W = 48, 64
    gts, segs = [], []
    base = np.zeros((H, W), np.int64)
    base[10:30, 12:42] = 1                                           # 600 pixels
    for extra in (0, 12, 13, 25):                                    # IoU 600 / (600 + 20 * extra): 1, 0.714, 0.698, 0.545
        pred = base.copy()
        pred[10:30, 42:42 + extra] = 1
        gts.append(base)
        segs.append(pred)
    gts.append((rng.rand(H, W) < 0.3).astype(np.int64))
    segs.append((rng.rand(H, W) < 0.3).astype(np.int64))
    gts.append(np.zeros((H, W), np.int64))                           # empty union: 0 / 0 = NaN, a miss
    segs.append(np.zeros((H, W), np.int64))
    ns = _namespace(None, 0.0)
    inter, union = [], []
    with np.errstate(all="ignore"):
        for g, p in zip(gts, segs):
            seg = torch.from_numpy(np.stack([1 - p, p]).astype(np.float32))[None]          # argmax over dim 1 gives p
            Evaluator.mask_iou(ns, {"seg": seg}, {"mask": torch.from_numpy(g)[None]})
            inter.append(int((p & g).sum()))
            union.append(int((p | g).sum()))
    c = dict(mask_pred=np.stack(segs).astype(np.uint8), mask_gt=np.stack(gts).astype(np.uint8),
             inter=np.array(inter, np.int64), union=np.array(union, np.int64), hit_ap=np.array(ns.mask_ap, bool))
    for i, u in zip(inter, union):
        assert u == 0 or _far(i / u, 0.7)
    assert c["hit_ap"].tolist() == [True, True, False, False, False, False]
    return c


def main():
    Evaluator, utils = load_reference()
    cases = {"metrics_n5841": pose_case(Evaluator, utils, 5841, 11, 0.15),
             "metrics_n777": pose_case(Evaluator, utils, 777, 12, 0.12),
             "metrics_masks": mask_case(Evaluator)}
    for name, c in cases.items():
        path = os.path.join(OUT, name + ".npz")
        if os.path.exists(path) and "--force" not in sys.argv:       # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v), equal_nan=np.asarray(v).dtype.kind == "f")
                                              for k, v in c.items())
            print(name, "exists,", "identical content" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, {k: (v.shape if hasattr(v, "shape") else v) for k, v in c.items()})


if __name__ == "__main__":
    main()
