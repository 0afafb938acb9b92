"""The device pose with its start (include/pvnet_pose.h, clean_pvnet_amd.pose) -- what can be checked without a GPU: the C ABI
library exports what its header declares, refuses bad arguments before any launch, and the Python surface has the
reference's shapes.  The numbers are checked on the GPU in test_gpu_pose.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "pvnet_pose.h")
SO = os.path.join(ROOT, "clean-pvnet_amd", "libpvnet_pose.so")

_P = ctypes.c_void_p
_INIT_ARGS = [_P] * 4 + [ctypes.c_int] + [_P] * 2 + [ctypes.c_int] * 4 + [_P]
_POSE_ARGS = [_P] * 4 + [ctypes.c_int] + [_P] * 5 + [ctypes.c_int] * 5 + [ctypes.c_double, _P]


def _lib():
    L = ctypes.CDLL(SO)
    L.pvp_initial_pose_batched.argtypes = _INIT_ARGS
    L.pvp_pose_batched.argtypes = _POSE_ARGS
    return L


def test_header_names_equal_the_library_exports():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    names = set(re.findall(r"\b([a-z_0-9]+)\s*\(", txt)) - {"defined"}
    assert names == {"pvp_initial_pose_batched", "pvp_pose_batched"}
    L = ctypes.CDLL(SO)
    for n in names:
        assert hasattr(L, n)
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True)
    if nm.returncode == 0:                                  # every exported pvp_ symbol is declared
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("pvp_")}
        assert exported == names


def test_status_and_method_codes_match_the_header(pkg):
    from clean_pvnet_amd import pose
    defs = dict(re.findall(r"#define\s+(PVP_\w+)\s+(-?\d+)", open(HDR).read()))
    assert {k: int(v) for k, v in defs.items() if k.startswith("PVP_START_")} == {"PVP_START_P3P": pose.METHODS["p3p"],
                                                                                   "PVP_START_DLT": pose.METHODS["dlt"]}
    assert sorted(int(v) for k, v in defs.items() if k.startswith("PVP_STATUS_")) == sorted(pose.STATUS)


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    buf = (ctypes.c_double * 64)()
    ibuf = (ctypes.c_int * 4)()
    d, i = ctypes.cast(buf, _P), ctypes.cast(ibuf, _P)
    # NULL pointers (host pointers elsewhere: a launch would fault, so -1 proves none happened)
    assert L.pvp_initial_pose_batched(None, None, None, None, 0, None, None, 1, 9, 0, 0, None) == -1
    assert L.pvp_initial_pose_batched(d, d, None, d, 0, d, i, 1, 9, 0, 0, None) == -1        # P3P needs the weights
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, None, 1, 9, 0, 0, None) == -1        # no status
    assert L.pvp_pose_batched(None, None, None, None, 1, None, None, None, None, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_pose_batched(d, d, None, d, 0, d, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_pose_batched(d, d, d, d, 1, None, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    # out of range: method, pn, B
    assert L.pvp_initial_pose_batched(d, d, d, d, 2, d, i, 1, 9, 0, 0, None) == -1
    assert L.pvp_pose_batched(d, d, d, d, -1, d, None, None, i, None, 1, 9, 0, 0, 0, 0.0, None) == -1
    for pn in (3, 4097):
        assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, 1, pn, 0, 0, None) == -1
        assert L.pvp_pose_batched(d, d, d, d, 1, d, None, None, i, None, 1, pn, 0, 0, 0, 0.0, None) == -1
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, -1, 9, 0, 0, None) == -1
    # an empty batch is valid and launches nothing
    assert L.pvp_initial_pose_batched(d, d, d, d, 1, d, i, 0, 9, 0, 0, None) == 0
    assert L.pvp_pose_batched(d, d, None, d, 1, d, None, None, i, None, 0, 9, 0, 0, 0, 0.0, None) == 0


def test_python_signatures(pkg):
    from clean_pvnet_amd import pose
    from clean_pvnet_amd.un_pnp_utils import uncertainty_pnp_batched
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    E = inspect.Parameter.empty
    assert sig(pose.initial_pose_batched) == [("points_2d", E), ("points_3d", E), ("camera_matrix", E), ("weights_2d", None),
                                              ("method", "p3p")]
    assert sig(pose.pnp_batched) == [("points_3d", E), ("points_2d", E), ("camera_matrix", E)]
    assert sig(pose.pnp) == [("points_3d", E), ("points_2d", E), ("camera_matrix", E), ("method", 0)]
    assert sig(pose.solve_pose) == [("output", E), ("kpt_3d", E), ("K", E), ("un_pnp", False)]
    assert dict(sig(uncertainty_pnp_batched))["init_rt"] is None
    from lib.csrc.uncertainty_pnp import un_pnp_utils as drop_in
    for n in ("initial_pose_batched", "pnp_batched", "pnp", "solve_pose"):
        assert getattr(drop_in, n) is getattr(pose, n)


def test_pnp_supports_only_the_iterative_method(pkg):
    from clean_pvnet_amd.pose import pnp
    P = np.random.RandomState(0).uniform(-0.05, 0.05, (9, 3))
    for method in (1, 2, 6):                                   # SOLVEPNP_EPNP, _P3P, _UPNP
        with pytest.raises(NotImplementedError):
            pnp(P, np.zeros((9, 2)), np.eye(3), method=method)


def test_p3p_twin_has_no_solution_for_a_collinear_triple(pkg):
    """The rotation about the line of a collinear object triple is undetermined; the twin (and the device) reject it
    rather than return an arbitrary one."""
    from clean_pvnet_amd.un_pnp_utils import p3p_depths
    P = np.array([[0.0, 0.0, 0.0], [0.04, 0.01, -0.02], [0.028, 0.007, -0.014]])
    f = np.array([[0.1, 0.05, 1.0], [0.12, 0.02, 1.0], [0.11, 0.04, 1.0]])
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    assert p3p_depths(f, P) == []
