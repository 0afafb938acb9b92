"""Model metadata (include/pvnet_vote.h's last section, clean_pvnet_amd.model, lib.csrc.fps.fps_utils) without a GPU: the numpy
twin of the contracts (tests/model_twin.py) reproduces the reference's own results (tests/golden/model_*.npz), a binary64
evaluation of the same rule and scipy's ``cdist``; the entry points exist under ABI 8 in the seven libraries, check their
arguments before any launch and answer the workspace queries on the host; the wrapper refuses CPU tensors and validates
``sn``, ``n`` and ``start`` on the host.  The GPU tests (tests/test_gpu_model.py) then hold the device to the twin as bytes."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import capi
from tests import model_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE_FPS = "/root/reference/lib/csrc/fps/fps_utils.py"
SYMBOLS = {"pvv_fps_workspace_bytes", "pvv_fps", "pvv_model_workspace_bytes", "pvv_model_bounds", "pvv_model_diameter"}


# ------------------------------------------------------------------------------------------------ 1. the twin
@pytest.mark.parametrize("name", list(twin.GOLDEN))
def test_twin_reproduces_the_reference(name):
    g = np.load(os.path.join(GOLDEN, "model_%s.npz" % name))
    pts, sn = twin.golden_points(name)
    assert sn == int(g["sn"])
    if "points" in g:
        assert np.array_equal(pts, g["points"])
    else:
        assert (str(g["kind"]), int(g["n"]), int(g["seed"])) == twin.GOLDEN[name][:3]
    assert np.array_equal(twin.fps(pts, sn), g["idx_center"])
    assert int(g["idx_random"][0]) == int(g["start"])
    assert np.array_equal(twin.fps(pts, sn, int(g["start"])), g["idx_random"])
    assert twin.diameter(pts).tobytes() == g["diameter"].tobytes()
    assert twin.diameter(pts.astype(np.float64)).tobytes() == g["diameter"].tobytes()


def test_golden_holds_the_quirks():
    g = {name: np.load(os.path.join(GOLDEN, "model_%s.npz" % name)) for name in twin.GOLDEN}
    assert g["abba"]["idx_center"].tolist() == [0, 1, 0, 0, 0, 0]                   # index 0 repeats, chosen before or not
    assert g["one_point"]["idx_center"].tolist() == [0, 0, 0] and float(g["one_point"]["diameter"]) == 0.0
    assert int(g["sn_gt_n"]["sn"]) > int(g["sn_gt_n"]["n"])
    rep = g["repeated_n600"]["idx_center"]
    assert (rep[12:] == 0).all() and len(set(rep[:12].tolist())) == 12              # 12 distinct points, then the rule
    lat = twin.cloud("lattice", 1100, 3)
    assert len(np.unique(lat, axis=0)) < 300                                        # many equal points: ties are decided by index


@pytest.mark.parametrize("kind,n,sn", [("gauss", 400, 12), ("planar", 257, 9), ("gauss", 1500, 6)])
def test_twin_equals_a_binary64_evaluation_on_separated_clouds(kind, n, sn):
    """Multiples of 1/32 in a box of side < 16 (the centre: multiples of 1/64 within 8 of every point): every difference has at
    most 9 bits, every square 18 and every sum 20, all exact in float32, so float32 can change no order."""
    rng = np.random.RandomState(n)
    pts = (np.round(twin.cloud(kind, n, 77).astype(np.float64) * 40 * 32) / 32).astype(np.float32)
    assert (pts.max(0) - pts.min(0)).max() < 16
    for start in (None, 0, int(rng.randint(n))):
        assert np.array_equal(twin.fps(pts, sn, start), twin.fps_binary64(pts, sn, start))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_twin_diameter_equals_cdist(dtype):
    from scipy.spatial.distance import cdist
    for n, seed in ((1, 1), (2, 2), (333, 3), (1100, 4)):
        p = (np.random.RandomState(seed).randn(n, 3) * 0.05).astype(dtype)
        # cdist gives sqrt of the same sum in the same order for three coordinates; sqrt is monotonic, so the maxima agree
        assert twin.diameter(p) == cdist(p.astype(np.float64), p.astype(np.float64)).max()
    p = twin.planted(2 * twin.TILE + 17, 9, 3, 2 * twin.TILE + 5)
    d = p[3].astype(np.float64) - p[2 * twin.TILE + 5].astype(np.float64)
    assert twin.diameter(p) == np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) > 1.7   # the planted pair
    assert twin.diameter(np.ones((40, 3), dtype)) == 0.0


def test_twin_corners_follow_the_references_row_order():
    p = twin.cloud("gauss", 50, 5)
    c, (lo, hi) = twin.corners(p), twin.bounds(p)
    assert c.shape == (8, 3) and np.array_equal(c[0], lo) and np.array_equal(c[7], hi)
    assert np.array_equal(c[1], [lo[0], lo[1], hi[2]]) and np.array_equal(c[4], [hi[0], lo[1], lo[2]])
    assert np.array_equal(twin.center(p), (c.max(0) + c.min(0)) / 2)                # handle_custom_dataset.py:94


def test_case_table_holds_what_the_gpu_tests_need():
    assert set(twin.SIZES) >= {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2 * twin.TILE + 17}
    assert twin.sample_counts(65) == (1, 2, 8, 68) and twin.starts(65) == [None, 0, 32, 64] and twin.starts(1) == [None, 0]
    want = twin.reference("repeated", 257, None)
    assert len(want) == 260 and np.array_equal(want[:8], twin.fps(twin.cloud("repeated", 257, twin.kind_seed("repeated", 257)), 8))
    assert (want[6:] == 0).all()                                                    # six distinct points
    for n in twin.SIZES:                                                            # the shared reference covers every count of the table
        assert len(twin.reference("gauss", n, None)) == max(twin.sample_counts(n)) >= 8
    assert [p[0] for p in twin.plant_places(3 * twin.TILE + 17)] == ["ends", "last_partial_tile", "one_tile", "two_middle_tiles"]


# ------------------------------------------------------------------------------------------------ 2. the library
def test_header_declares_and_library_exports_the_entry_points():
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    raw = open(HEADER).read()
    assert "#define PVV_ABI_VERSION 8" in raw                                       # additive: the version did not move
    for cite in ("farthest_point_sampling.cpp", "misc.py:139-154", "handle_custom_dataset.py:19-40"):
        assert cite in raw
    section = raw[raw.index("Model metadata"):]
    assert SYMBOLS <= set(re.findall(r"\b(pvv_[a-z0-9_]+)\s*\(", section))           # a new last section


def test_no_eighth_library():
    import lib
    b = lib.load_build()
    assert len(b.HIP_LIBS) == 7 and list(b.HIP_LIBS)[-1] == "icp"
    assert os.path.exists(os.path.join(b.CSRC, "model.hpp")) and not os.path.exists(os.path.join(b.CSRC, "pvnet_model.hip"))


def test_workspace_queries_are_host_only_values():
    L = capi.load()
    AUTO, ONE, TILED = 0, 1, 2
    assert L.pvv_abi_version() == 8
    assert L.pvv_fps_workspace_bytes(8, 5841, 8, AUTO) == 256 == L.pvv_fps_workspace_bytes(8, 8192, 8, ONE)
    up = lambda v: (v + 255) // 256 * 256                                           # noqa: E731
    T = 98                                                                          # 100 000 points in tiles of 1024
    want = up(4 * 8 * 100000) + up(8 * 2 * 8 * T) + up(4 * 6 * 8 * T)               # min_dist, two key buffers, the tiles' boxes
    assert L.pvv_fps_workspace_bytes(8, 100000, 8, AUTO) == want == L.pvv_fps_workspace_bytes(8, 100000, 8, TILED)
    assert L.pvv_fps_workspace_bytes(1, 65, 3, TILED) == up(4 * 65) + 256 + 256 == 1024
    assert L.pvv_model_workspace_bytes(8, 100000) == up(8 * 6 * 8 * T) + 256
    for args, word in (((0, 10, 1, AUTO), b"positive"), ((1, 0, 1, AUTO), b"positive"), ((1, 10, 0, AUTO), b"sn must be positive"),
                       ((1, 10, 1, 3), b"unknown path"), ((1, 8193, 1, ONE), b"8192"), ((1, (1 << 20) + 1, 1, AUTO), b"2^20"),
                       ((65536, 10, 1, AUTO), b"split the batch"), ((8192, 1 << 20, 1, AUTO), b"2^22")):
        assert L.pvv_fps_workspace_bytes(*args) == 0 and word in L.pvv_last_error(), args
    assert L.pvv_model_workspace_bytes(1, (1 << 20) + 1) == 0 and b"2^20" in L.pvv_last_error()


def test_null_pointers_and_bad_sizes_return_minus_one_before_any_launch():
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    fps = lambda pts, ws, idx, B=1, N=10, sn=2, path=0, nbytes=1 << 20: L.pvv_fps(pts, None, None, B, N, sn, path, ws, nbytes, idx, None)  # noqa: E731
    assert fps(None, x, x) == -1 and b"NULL device pointer" in L.pvv_last_error()
    assert fps(x, x, None) == -1 and b"NULL device pointer" in L.pvv_last_error()
    assert fps(x, None, x) == -1 and b"NULL workspace" in L.pvv_last_error()
    assert fps(x, x + 8, x) == -1 and b"aligned" in L.pvv_last_error()
    assert fps(x, x, x, sn=0) == -1 and b"sn must be positive" in L.pvv_last_error()
    assert fps(x, x, x, N=0) == -1 and b"positive" in L.pvv_last_error()
    assert fps(x, x, x, path=7) == -1 and b"unknown path" in L.pvv_last_error()
    assert fps(x, x, x, N=9000, path=1) == -1 and b"8192" in L.pvv_last_error()
    assert fps(x, x, x, N=9000, path=2, nbytes=1000) == -2 and b"too small" in L.pvv_last_error()
    for f, out in ((L.pvv_model_bounds, (x, x)), (L.pvv_model_diameter, (x,))):
        assert f(None, 0, None, 1, 10, x, 1 << 20, *out, None) == -1 and b"NULL device pointer" in L.pvv_last_error()
        assert f(x, 0, None, 1, 10, x, 1 << 20, *((None,) * len(out)), None) == -1 and b"NULL device pointer" in L.pvv_last_error()
        assert f(x, 0, None, 1, 10, None, 1 << 20, *out, None) == -1 and b"NULL workspace" in L.pvv_last_error()
        assert f(x, 1, None, 0, 10, x, 1 << 20, *out, None) == -1 and b"positive" in L.pvv_last_error()
        assert f(x, 1, None, 1, 10, x, 16, *out, None) == -2 and b"too small" in L.pvv_last_error()
    assert L.pvv_model_diameter(x, 0, None, 8, 1 << 20, x, 1 << 30, x, None) == -1 and b"diameter: B * ceil" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 3. the wrapper
def test_module_imports(pkg):
    from clean_pvnet_amd import model
    assert all(callable(getattr(model, f)) for f in ("farthest_point_sampling", "bounds", "model_corners", "model_center", "diameter",
                                                     "model_meta"))
    assert (model.AUTO, model.ONE_BLOCK, model.TILED) == (0, 1, 2) and model.TILE == twin.TILE
    raw = open(HEADER).read()
    for name, value in (("PVV_FPS_ONE_BLOCK_MAX", model.ONE_BLOCK_MAX), ("PVV_MODEL_TILE", model.TILE)):
        assert re.search(r"#define %s %d\b" % (name, value), raw)
    params = inspect.signature(model.farthest_point_sampling).parameters
    assert list(params) == ["points", "sn", "init_center", "start", "n", "path"]
    assert params["init_center"].default is True and params["path"].default == model.AUTO


def test_cpu_tensors_are_refused(pkg):
    import torch
    from clean_pvnet_amd import model
    p = torch.zeros(2, 10, 3)
    for f in (lambda: model.farthest_point_sampling(p, 4), lambda: model.bounds(p), lambda: model.model_corners(p),
              lambda: model.model_center(p), lambda: model.diameter(p.double()), lambda: model.model_meta(p)):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor; there is no CPU fallback"):
            f()
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        model.farthest_point_sampling(np.zeros((10, 3), np.float32), 4)


def test_host_validation(pkg):
    """``sn``, ``n`` and ``start`` are checked on the host before anything reaches the device: meta tensors carry the shapes."""
    import torch
    from clean_pvnet_amd import model
    p = torch.empty(2, 10, 3, device="meta")
    real_need = model._native.need_cuda
    model._native.need_cuda = lambda *a: None
    try:
        fps = model.farthest_point_sampling
        with pytest.raises(ValueError, match="sn must be >= 1"):
            fps(p, 0)
        for bad in ([0, 10], [10, 11], [-1, 3], [5]):
            with pytest.raises(ValueError, match="n has|must lie in \\[1, N = 10\\]"):
                fps(p, 4, n=bad)
            with pytest.raises(ValueError, match="n has|must lie in \\[1, N = 10\\]"):
                model.diameter(p, n=bad)
            with pytest.raises(ValueError, match="n has|must lie in \\[1, N = 10\\]"):
                model.bounds(p, n=bad)
        with pytest.raises(TypeError, match="host sequence"):
            fps(p, 4, n=torch.tensor([3, 3]))
        with pytest.raises(ValueError, match="needs init_center=False"):
            fps(p, 4, start=0)
        for bad, n in ((10, None), (-1, None), ([0, 10], None), ([0, 5], [10, 5]), ([0], None)):
            with pytest.raises(ValueError, match="start has|every start must lie in \\[0, n_b\\)"):
                fps(p, 4, False, start=bad, n=n)
        with pytest.raises(ValueError, match="path must be"):
            fps(p, 4, path=5)
        with pytest.raises(RuntimeError, match="must be torch.float32"):
            fps(p.double(), 4)
        with pytest.raises(RuntimeError, match="float32 or torch.float64"):
            model.diameter(p.half())
        with pytest.raises(ValueError, match="\\[B, N, 3\\]"):
            fps(torch.empty(2, 10, 2, device="meta"), 4)
        with pytest.raises(ValueError, match="8192"):                               # the library's own refusal, through the host-only query
            fps(torch.empty(1, 9000, 3, device="meta"), 4, path=model.ONE_BLOCK)
    finally:
        model._native.need_cuda = real_need


def test_drop_in_path_has_the_references_signature(pkg):
    from lib.csrc.fps import fps_utils
    sig = inspect.signature(fps_utils.farthest_point_sampling)
    assert str(sig) == "(pts, sn, init_center=False)"
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fps_utils.farthest_point_sampling(np.zeros((5, 3)), 2, True)
    assert os.path.exists(os.path.join(ROOT, "lib", "csrc", "fps", "setup.py"))


@pytest.mark.skipif(not os.path.exists(REFERENCE_FPS), reason="the reference is not on this machine")
def test_drop_in_signature_equals_the_reference_files(pkg):
    import ast
    from lib.csrc.fps import fps_utils
    tree = ast.parse(open(REFERENCE_FPS).read())                                    # (its import of the cffi extension cannot run here)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "farthest_point_sampling")
    theirs = "(%s)" % ast.unparse(fn.args)
    assert str(inspect.signature(fps_utils.farthest_point_sampling)) == theirs
