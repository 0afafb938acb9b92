#!/usr/bin/env python
"""Generate tests/golden/model_*.npz by running THE REFERENCE'S OWN farthest point sampling and diameter on the CPU.

``lib/csrc/fps/src/farthest_point_sampling.cpp`` is compiled where it lies under /root/reference with the flags of the
reference's ``lib/csrc/fps/setup.py`` (``-O2 -std=c++11 -fPIC``) into a temporary directory outside this tree, loaded with
ctypes, and the directory is removed afterwards: nothing compiled and no program text enters the repository.  Both entry
points are called: ``farthest_point_sampling_init_center`` and ``farthest_point_sampling``, whose first index is its
``rand() % pn`` and is stored as the ``start`` that reproduces the run.  ``calc_pts_diameter`` is imported from
``lib/utils/vsd/misc.py`` where it lies, with ``PIL`` stubbed when it is absent.

Stored per case (tests/model_twin.py::GOLDEN): the cloud's kind, size and seed -- the tests regenerate the cloud -- or the points
themselves when the cloud is tiny; ``sn``; ``idx_center``; ``idx_random`` and its ``start``; ``diameter`` of the cloud widened to
float64.  While writing it is asserted that the numpy twin reproduces every stored value exactly.

Run from the repository root in the build container:  python tests/golden/make_model_golden.py
"""
import ctypes
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import model_twin as twin  # noqa: E402


def load_reference_fps(tmp):
    so = os.path.join(tmp, "libref_fps.so")
    subprocess.check_call(["g++", "-shared", "-fPIC", "-O2", "-std=c++11", "-o", so,
                           os.path.join(REF, "lib/csrc/fps/src/farthest_point_sampling.cpp")])
    L = ctypes.CDLL(so)
    for f in (L.farthest_point_sampling, L.farthest_point_sampling_init_center):
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int], None
    return L


def load_reference_diameter():
    for name in ("PIL", "PIL.Image", "PIL.ImageDraw"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            parent, _, leaf = name.rpartition(".")
            if parent:
                setattr(sys.modules[parent], leaf, sys.modules[name])
    spec = importlib.util.spec_from_file_location("ref_vsd_misc", os.path.join(REF, "lib/utils/vsd/misc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calc_pts_diameter


def run(fn, pts, sn):
    """The call of the reference's fps_utils.py:9-18."""
    pts = np.ascontiguousarray(pts, np.float32)
    idxs = np.ascontiguousarray(np.zeros([sn], np.int32))
    fn(pts.ctypes.data, idxs.ctypes.data, pts.shape[0], sn)
    return idxs


def case(name, L, calc_pts_diameter):
    pts, sn = twin.golden_points(name)
    c = {"sn": np.int32(sn)}
    spec = twin.GOLDEN[name]
    if len(spec) == 2:
        c["points"] = pts
    else:
        c["kind"], c["n"], c["seed"] = np.array(spec[0]), np.int32(spec[1]), np.int32(spec[2])
    c["idx_center"] = run(L.farthest_point_sampling_init_center, pts, sn)
    c["idx_random"] = run(L.farthest_point_sampling, pts, sn)
    c["start"] = np.int32(c["idx_random"][0])
    c["diameter"] = np.float64(calc_pts_diameter(pts.astype(np.float64)))
    assert np.array_equal(twin.fps(pts, sn), c["idx_center"]), name
    assert np.array_equal(twin.fps(pts, sn, int(c["start"])), c["idx_random"]), name
    assert twin.diameter(pts).tobytes() == c["diameter"].tobytes(), name
    assert twin.diameter(pts.astype(np.float64)).tobytes() == c["diameter"].tobytes(), name
    return c


def main():
    tmp = tempfile.mkdtemp(prefix="model_golden_")
    try:
        L = load_reference_fps(tmp)
        calc = load_reference_diameter()
        cases = {"model_" + name: case(name, L, calc) for name in twin.GOLDEN}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert cases["model_abba"]["idx_center"].tolist() == [0, 1, 0, 0, 0, 0] and cases["model_one_point"]["idx_center"].tolist() == [0, 0, 0]
    assert cases["model_one_point"]["diameter"] == 0.0
    for name, c in cases.items():
        path = os.path.join(OUT, name + ".npz")
        if os.path.exists(path) and "--force" not in sys.argv:       # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v)) for k, v in c.items()
                                              if k not in ("idx_random", "start"))
            print(name, "exists,", "identical content but for the random start" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, {k: (v.shape if getattr(v, "shape", ()) else v) for k, v in c.items()})


if __name__ == "__main__":
    main()
