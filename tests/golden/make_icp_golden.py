#!/usr/bin/env python
"""Generate tests/golden/icp_*.npz by running THE REFERENCE'S OWN ``ICPRefiner.refine`` on the CPU.

``lib/utils/icp/icp_utils.py`` and ``lib/utils/pysixd/transform.py`` are imported from where they lie under /root/reference
(never copied).  The reference renders through OpenGL, which does not exist here: ``lib.utils.renderer.opengl_utils`` is a stub
module and ``ICPRefiner.renderer`` an object whose ``render`` returns the numpy twin of the rasteriser's contract
(tests/vsd_twin.py::render_depth).  ``np.random`` is seeded before each ``refine`` and the indices the reference draws are
recorded, so that the twin (tests/icp_twin.py) and the device run on the same samples.  Both stages run as
``Evaluator.icp_refine`` runs them (lib/evaluators/tless_test/pvnet.py:143-158): ``depth_only`` with factor 5.0 on
``[R | t * 1000]``, then ``no_depth`` from that pose.

Stored per fixture: the seeds of the mesh and of the sensor images (the tests regenerate both, icp_twin.regenerate), the
poses in metres, the camera, the size; the drawn indices (int32); the reference's R, t and round count of each stage and its
final pose; the twin's stage poses, final pose and info rows; and ``deviation``, the largest element-wise |twin - reference|
over the fixture, in millimetres for t and on the entries of R.

Asserted while writing (a fixture that misses one is drawn again from another seed: change its seeds below):
  * the reference and the twin take the same number of rounds in every stage;
  * in no round of the twin does |prev - mean| lie within a factor 2 of the tolerance on either side;
  * n_real is not within 1 of n_syn / 20;
  * the rotation-limit decision equals the reference's ``rotation_from_matrix`` decision and the cosine is not within 1e-6 of
    the limit;
  * the twin equals the reference under the repository's tolerance rule (tests/tolerances.py), in millimetres for t and on
    the entries of R.

Run from the repository root in the build container:  python tests/golden/make_icp_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference/lib/utils"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import icp_twin as twin  # noqa: E402
from tests import tolerances as tol  # noqa: E402
from tests import vsd_twin as vt  # noqa: E402

N_MAX, TOLERANCE, LIMIT_DEG = 3000, 5e-7, 20.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    """icp_utils with ``lib.utils.renderer.opengl_utils`` stubbed; the names it imports are entered in sys.modules only while it
    loads, then whatever was there before is put back."""
    names = ("lib.utils", "lib.utils.renderer", "lib.utils.renderer.opengl_utils", "lib.utils.pysixd", "lib.utils.pysixd.transform")
    saved = {n: sys.modules.get(n) for n in names}
    try:
        for n in names[:4]:
            sys.modules[n] = types.ModuleType(n)
            sys.modules[n].__path__ = []
        transform = _load("lib.utils.pysixd.transform", os.path.join(REF, "pysixd", "transform.py"))
        sys.modules["lib.utils.renderer"].opengl_utils = sys.modules["lib.utils.renderer.opengl_utils"]
        sys.modules["lib.utils.pysixd"].transform = transform
        icp_utils = _load("ref_icp_utils", os.path.join(REF, "icp", "icp_utils.py"))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return icp_utils, transform


class TwinRenderer:
    def __init__(self, pts, faces):
        self.pts, self.faces = pts, faces

    def render(self, im_size, near, far, K, R, t):
        return vt.render_depth(self.pts, self.faces, np.concatenate([R, np.reshape(t, (3, 1))], 1), K, tuple(im_size), near, far)


def _near(P, dw, dt):
    return np.concatenate([vt.rodrigues(dw) @ P[:, :3], (P[:, 3] + np.asarray(dt)).reshape(3, 1)], 1)


def definitions():
    """name -> the inputs of a fixture (poses in metres, one row per pose; consecutive poses share an image)."""
    g0 = vt.pose([0.9, 0.4, -0.3], [-0.09, 0.02, 0.70])
    big = dict(mesh_seed=5, scene_seed=[151], size=(720, 540), K=vt.camera(1.0), occluder=True, mask_keep=[1.0],
               pose_gt=[g0], pose_est=[_near(g0, [0.04, -0.03, 0.05], [0.004, -0.003, 0.012])], draw_seed=1000)
    h0 = vt.pose([0.3, -0.8, 0.5], [-0.09, 0.01, 0.66])
    h1 = vt.pose([1.2, 0.2, -0.9], [0.09, -0.01, 0.74])
    h2 = vt.pose([-0.6, 0.5, 1.4], [-0.07, -0.02, 0.72])
    h3 = vt.pose([2.0, -0.4, 0.3], [0.08, 0.03, 0.68])
    half = dict(mesh_seed=6, scene_seed=[161, 162], size=(360, 270), K=vt.camera(0.5), occluder=False, mask_keep=[1.0] * 4,
                pose_gt=[h0, h1, h2, h3],
                pose_est=[_near(h0, [0.05, 0.02, -0.04], [0.003, 0.002, 0.010]), _near(h1, [-0.03, 0.04, 0.02], [-0.002, 0.003, -0.008]),
                          _near(h2, [0.02, -0.05, 0.03], [0.002, -0.002, 0.006]), _near(h3, [-0.04, -0.02, -0.03], [-0.003, 0.001, 0.009])],
                draw_seed=2100)               # 2000 missed a condition: a step of pose 2, stage 1 within a factor 2 of the tolerance
    e0 = vt.pose([0.5, 0.9, -0.2], [-0.08, 0.0, 0.70])
    away = vt.pose([0.1, 0.2, 0.3], [2.0, 0.0, 0.70])                                        # outside the image: empty render
    e2 = vt.pose([-0.9, 0.3, 0.7], [0.08, 0.01, 0.72])                                       # its mask keeps a few rows only
    edge = dict(mesh_seed=7, scene_seed=[171], size=(360, 270), K=vt.camera(0.5), occluder=False, mask_keep=[1.0, 1.0, 0.04],
                pose_gt=[e0, away, e2],
                pose_est=[_near(e0, [0.03, 0.03, 0.02], [0.002, 0.002, -0.007]), _near(away, [0.1, 0.0, 0.0], [0.1, 0.0, 0.0]),
                          _near(e2, [0.02, 0.0, -0.02], [0.001, -0.002, 0.005])],
                draw_seed=3000)
    return {"icp_720": big, "icp_360": half, "icp_edge": edge}


def make(name, d, ref, transform):
    c = dict(mesh_seed=d["mesh_seed"], scene_seed=np.array(d["scene_seed"]), size=np.array(d["size"]), K=d["K"],
             pose_est=np.array(d["pose_est"]), pose_gt=np.array(d["pose_gt"]), t_scale=1000.0, depth_scale=0.1,
             occluder=d["occluder"], mask_keep=np.array(d["mask_keep"]), n_max=N_MAX, tolerance=TOLERANCE, angle_limit_deg=LIMIT_DEG)
    r = twin.regenerate(name, c)
    P, K, size = len(c["pose_est"]), c["K"], r["size"]
    refiner = ref.ICPRefiner.__new__(ref.ICPRefiner)
    refiner.renderer, refiner.im_size = TwinRenderer(r["pts"], r["faces"]), size
    drawn, rounds_seen, angles = [], [], []
    real_choice, real_icp, real_rot = np.random.choice, ref.icp, transform.rotation_from_matrix

    def choice(a, n):
        out = real_choice(a, n)
        drawn.append(np.asarray(out))
        return out

    def icp(*a, **k):
        out = real_icp(*a, **k)
        rounds_seen.append(out[2] + 1)
        return out

    def rot(T):
        out = real_rot(T)
        angles.append(out[0])
        return out

    idx = np.zeros((2, 2, P, N_MAX), np.int32)
    ref_R, ref_t, ref_rounds = np.zeros((2, P, 3, 3)), np.zeros((2, P, 3)), np.zeros((2, P), np.int32)
    ref_pose, twin_stage, twin_pose = np.zeros((P, 3, 4)), np.zeros((2, P, 3, 4)), np.zeros((P, 3, 4))
    info = np.zeros((2, P, 5), np.int32)
    dev_t = dev_R = 0.0
    climit = twin.cos_limit(LIMIT_DEG)
    for p in range(P):
        z_img = vt.sensor_depth(r["raw"][p // r["per_image"]], c["depth_scale"])
        mask = r["mask"][p]
        depth = z_img.copy()
        depth[mask != 1] = 0                                                        # tless_test/pvnet.py:150
        R, t = c["pose_est"][p][:, :3].copy(), c["pose_est"][p][:, 3] * 1000.0        # :151-152
        stage_args = (dict(depth_only=True, max_mean_dist_factor=5.0), dict(no_depth=True))
        np.random.choice, ref.icp, transform.rotation_from_matrix = choice, icp, rot
        try:
            with np.errstate(all="ignore"):
                for s, kw in enumerate(stage_args):
                    del drawn[:], rounds_seen[:], angles[:]
                    np.random.seed(d["draw_seed"] + 10 * p + s)
                    R, t = refiner.refine(depth, R, t, K.copy(), **kw)                # :154-155
                    ref_R[s, p], ref_t[s, p] = R, t
                    if drawn:
                        idx[s, 1, p, :len(drawn[0])], idx[s, 0, p, :len(drawn[1])] = drawn[0], drawn[1]   # real is drawn first
                        ref_rounds[s, p] = rounds_seen[0]
                    if s == 1 and angles:
                        ref_limited = abs(angles[0]) > LIMIT_DEG * np.pi / 180.0
                    else:
                        ref_limited = None
                    if s == 1:
                        stage2_limited = ref_limited
        finally:
            np.random.choice, ref.icp, transform.rotation_from_matrix = real_choice, real_icp, real_rot
        ref_pose[p] = np.hstack((ref_R[1, p], ref_t[0, p].reshape(3, 1) / 1000.0))    # :156
        # the twin on the same samples
        traces = ([], [])
        samples = tuple((idx[s, 0, p], idx[s, 1, p]) for s in range(2))
        out, infos, stages = twin.icp_refine(c["pose_est"][p], z_img, mask, K, r["pts"], r["faces"], size, samples=samples,
                                             n_max=N_MAX, tolerance=TOLERANCE, angle_limit_deg=LIMIT_DEG, traces=traces)
        twin_pose[p] = out
        for s in range(2):
            i = infos[s]
            twin_stage[s, p] = stages[s]
            info[s, p] = [i["status"], i["n_syn"], i["n_real"], i["n"], i["rounds"]]
            assert i["rounds"] == ref_rounds[s, p], (name, p, s, i["rounds"], ref_rounds[s, p])
            for step in traces[s]:
                assert not (TOLERANCE / 2 <= step <= TOLERANCE * 2), (name, p, s, step)
            assert abs(i["n_real"] - i["n_syn"] / 20.0) > 1 or i["n_syn"] == 0, (name, p, s, i)
            if "cos" in i:
                assert abs(i["cos"] - climit) > 1e-6 and (i["cos"] < climit) == bool(stage2_limited), (name, p, i, stage2_limited)
            tol.assert_means_close(stages[s][:, 3], ref_t[s, p], what="%s pose %d stage %d t" % (name, p, s))
            tol.assert_means_close(stages[s][:, :3], ref_R[s, p], what="%s pose %d stage %d R" % (name, p, s))
            dev_t = max(dev_t, float(np.abs(stages[s][:, 3] - ref_t[s, p]).max()))
            dev_R = max(dev_R, float(np.abs(stages[s][:, :3] - ref_R[s, p]).max()))
        print("%s pose %d: status %s rounds %s n %s  |twin - ref| so far: t %.3g mm, R %.3g" %
              (name, p, info[:, p, 0].tolist(), info[:, p, 4].tolist(), info[:, p, 3].tolist(), dev_t, dev_R), flush=True)
    c.update(idx=idx, ref_R=ref_R, ref_t=ref_t, ref_rounds=ref_rounds, ref_pose=ref_pose, twin_stage=twin_stage,
             twin_pose=twin_pose, info=info, deviation=np.array([dev_t, dev_R]))
    return c


def main():
    ref, transform = load_reference()
    for name, d in definitions().items():
        if len(sys.argv) > 1 and not sys.argv[1].startswith("--") and sys.argv[1] != name:
            continue
        c = make(name, d, ref, transform)
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
