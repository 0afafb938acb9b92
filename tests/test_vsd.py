"""The batched depth rasteriser and VSD (include/pvnet_vsd.h, clean_pvnet_amd.vsd) without a GPU: the numpy twin of the
rasteriser's contract against an independent ray caster, the twin's VSD arithmetic against fixtures made by the reference's
own functions (tests/golden/make_vsd_golden.py), the library's exports and its host-side argument checks.  The GPU tests
(tests/test_gpu_vsd.py) then hold the device to the twin bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import vsd_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VSDLIB = os.path.join(ROOT, "clean-pvnet_amd", "libpvnet_vsd.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("vsd_720", "vsd_360", "vsd_near")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_module_imports(pkg):
    from clean_pvnet_amd import vsd
    assert vsd.COSTS == {"step": 0, "tlinear": 1} and callable(vsd.render_depth) and callable(vsd.vsd)


# --------------------------------------------------------------------------------- 1. the twin against an independent renderer
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_rasteriser_against_the_ray_caster(name):
    """Coverage equal on every sample farther than 1/256 px from every projected edge of a near-clipped triangle (snapping
    moves a vertex by at most sqrt(2)/512 px), depth within 2**-23 relative there (float32 rounding), and those samples are
    at least 98 % of the covered ones -- a condition on the fixture, not a tolerance."""
    c = load(name)
    r = twin.regenerate(name, c)
    near, far = float(c["near"]), float(c["far"])
    poses = np.concatenate([twin.scaled(c["pose_est"], float(c["t_scale"])).reshape(-1, 3, 4),
                            twin.scaled(c["pose_gt"], float(c["t_scale"])).reshape(-1, 3, 4)])
    renders = np.concatenate([r["est"].reshape((-1,) + r["est"].shape[2:]), r["gt"].reshape((-1,) + r["gt"].shape[2:])])
    checked = 0
    for P, got in zip(poses, renders):
        want, band = twin.raycast_depth(r["pts"], r["faces"], P, c["K"], r["size"], near, far)
        cov_t, cov_r = got > 0, want > 0
        covered = int((cov_t | cov_r).sum())
        if covered == 0:
            assert not band.any() or not cov_t.any()
            continue
        excluded = int(((cov_t | cov_r) & band).sum())
        ok = ~band
        diff_cov = int((cov_t != cov_r)[ok].sum())
        both = ok & cov_t & cov_r
        rel = np.abs(got.astype(np.float64)[both] - want[both]) / want[both]
        print("%s: covered %d, excluded %d (%.2f %%), coverage differences %d, largest relative depth difference %.3g" %
              (name, covered, excluded, 100.0 * excluded / covered, diff_cov, rel.max() if rel.size else 0.0))
        assert excluded <= 0.02 * covered
        assert diff_cov == 0
        assert rel.size and rel.max() <= 2.0 ** -23
        checked += 1
    assert checked >= 2


def test_near_fixture_straddles_the_near_plane_and_mesh_mixes_sizes():
    c = load("vsd_near")
    pts, faces = twin.mesh(int(c["mesh_seed"]))
    Z = twin.eye_space(pts, twin.scaled(c["pose_gt"], float(c["t_scale"]))[0, 0])[:, 2]
    ins = Z[faces] >= float(c["near"])
    assert (ins.sum(1) == 1).any() and (ins.sum(1) == 2).any() and (ins.sum(1) == 0).any() and (ins.sum(1) == 3).any()
    assert len(faces) == 2 * 48 * 24 + 2
    e = pts[faces].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(e[:, 1] - e[:, 0], e[:, 2] - e[:, 0]), axis=1)
    assert area.max() > 10 * np.median(area)                             # the three long triangles of the apex


def test_twin_rasteriser_rules():
    """The fill rule on a shared edge, the half-pixel sample, depth of a fronto-parallel plane, and bad input."""
    K = np.array([[100.0, 0.0, 0.0], [0.0, 100.0, 0.0], [0.0, 0.0, 1.0]])
    P = twin.pose([0, 0, 0], [0, 0, 0])
    # a square [0.02, 0.06]^2 at Z = 2 -> pixels u, v in [1, 3]: samples 1.5 and 2.5 inside; split along a diagonal
    q = np.array([[0.02, 0.02, 2], [0.06, 0.02, 2], [0.06, 0.06, 2], [0.02, 0.06, 2]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    img = twin.render_depth(q, f, P, K, (5, 4), near=1.0, far=10.0)
    want = np.zeros((4, 5), np.float32)
    want[1:3, 1:3] = 2.0
    np.testing.assert_array_equal(img, want)
    one = twin.render_depth(q, f[:1], P, K, (5, 4), near=1.0, far=10.0) > 0
    two = twin.render_depth(q, f[1:], P, K, (5, 4), near=1.0, far=10.0) > 0
    assert not (one & two).any() and (one | two).sum() == 4              # every sample of the diagonal has one owner
    np.testing.assert_array_equal(twin.render_depth(q, f[:, ::-1], P, K, (5, 4), near=1.0, far=10.0), want)   # no culling
    # a square whose edges pass exactly through the samples (u, v in [1.5, 3.5]): left / top edges own, right / bottom do not
    q2 = np.array([[0.03, 0.03, 2], [0.07, 0.03, 2], [0.07, 0.07, 2], [0.03, 0.07, 2]], np.float32)
    img2 = twin.render_depth(q2, f, P, K, (5, 4), near=1.0, far=10.0)
    assert (img2 > 0).sum() == 4
    # outside [near, far], a bad face row, a non-finite pose
    assert not twin.render_depth(q, f, P, K, (5, 4), near=2.5, far=10.0).any()
    assert not twin.render_depth(q, f, P, K, (5, 4), near=0.5, far=1.5).any()
    bad = np.array([[0, 1, 2], [0, 2, 4], [-1, 2, 3]], np.int32)
    np.testing.assert_array_equal(twin.render_depth(q, bad, P, K, (5, 4), near=1.0, far=10.0) > 0, one)
    Pn = P.copy()
    Pn[1, 2] = np.nan
    assert not twin.render_depth(q, f, Pn, K, (5, 4), near=1.0, far=10.0).any()


# ------------------------------------------------------------------------------------- 2. the twin's VSD against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_vsd_reproduces_the_reference_fixture(name):
    """Masks bit for bit, counts equal, 'step' e bit for bit, 'tlinear' e within vsd_twin.tlinear_bound (derived in the
    twin's docstring from the two summation orders; nothing in it is measured)."""
    c = load(name)
    r = twin.regenerate(name, c)
    n, p = c["pose_est"].shape[:2]
    g = c["pose_gt"].shape[1]
    delta, tau = float(c["delta"]), float(c["tau"])
    for i in range(n):
        depth = twin.sensor_depth(r["raw"][i], float(c["depth_scale"]))
        for a in range(p):
            for b in range(g):
                step = twin.vsd_pair(r["est"][i, a], r["gt"][i, b], depth, c["K"], delta, tau, "step")
                np.testing.assert_array_equal(np.packbits(step["visib_gt"]), c["visib_gt_bits"][i, b])
                np.testing.assert_array_equal(np.packbits(step["visib_est"]), c["visib_est_bits"][i, a, b])
                assert [step["union"], step["inter"], step["cost"]] == c["counts"][i, a, b].tolist()
                assert step["e"] == c["e_step"][i, a, b], (name, i, a, b)
                tl = twin.vsd_pair(r["est"][i, a], r["gt"][i, b], depth, c["K"], delta, tau, "tlinear")
                want = float(c["e_tlinear"][i, a, b])
                bound = twin.tlinear_bound(want, tl["m"], float(c["cost_sum"][i, a, b]), tl["union"])
                print("%s[%d,%d,%d] tlinear got %.17g want %.17g |diff| %.3g bound %.3g" %
                      (name, i, a, b, tl["e"], want, abs(tl["e"] - want), bound))
                assert abs(tl["e"] - want) <= bound


def test_fixtures_hold_the_cases_the_checks_need():
    big, half, close = load("vsd_720"), load("vsd_360"), load("vsd_near")
    assert tuple(big["size"]) == (720, 540) and big["e_step"].shape == (1, 2, 2)
    assert big["e_step"][0, 0, 0] < 0.3 and big["e_step"][0, 1, 1] > 0.9                       # a hit, and a prediction far off
    assert half["e_step"].shape == (2, 2, 2) and half["counts"][1, 1, 1, 0] == 0 and half["e_step"][1, 1, 1] == 1.0
    assert close["counts"][0, 0, 0, 0] > 0
    for name, c in (("vsd_720", big), ("vsd_360", half), ("vsd_near", close)):
        for k in ("e_step", "e_tlinear"):
            assert (np.abs(c[k] - 0.3) > 1e-6 * 0.3).all()
        raw = twin.regenerate(name, c)["raw"]
        assert raw.dtype == np.uint16 and (raw == 0).any() and (raw > 0).any()
    assert twin.any_pair_hit(big["e_step"][0]) and not twin.any_pair_hit(big["e_step"][0, 1:])
    assert not twin.any_pair_hit(big["e_step"][0], gt_valid=[False, True])


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/utils/vsd/vsd_utils.py"),
                    reason="the reference tree exists only in the build container")
def test_vsd_fixtures_are_reproducible_from_the_reference():
    """tests/golden/make_vsd_golden.py, run here against the reference where it lies, regenerates every committed fixture
    with identical content (it never rewrites an existing file without --force)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_vsd_golden.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " exists," in l]
    assert len(lines) == len(FIXTURES) and all(l.endswith("identical content") for l in lines), out.stdout


# ------------------------------------------------------------------------------------------- 3. the library and its arguments
def test_vsd_library_exports_what_the_header_declares():
    txt = open(os.path.join(ROOT, "include", "pvnet_vsd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(pvs_[a-z_]+)\s*\(", txt))
    assert names == {"pvs_render_workspace_bytes", "pvs_render_depth_batched", "pvs_vsd_workspace_bytes", "pvs_vsd_batched"}
    L = ctypes.CDLL(VSDLIB)
    for n in names:
        assert hasattr(L, n)
    import shutil
    import subprocess
    nm = shutil.which("nm") or shutil.which("llvm-nm", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if nm:                                                       # and nothing else is exported
        out = subprocess.run([nm, "-D", "--defined-only", VSDLIB], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert {e for e in exported if not e.startswith("_")} == names, exported


def test_workspace_sizes_and_argument_errors():
    """Bad arguments are refused before anything is launched (no GPU is needed to be told so)."""
    L = ctypes.CDLL(VSDLIB)
    L.pvs_render_workspace_bytes.restype = ctypes.c_size_t
    L.pvs_vsd_workspace_bytes.restype = ctypes.c_size_t
    assert L.pvs_render_workspace_bytes(0, 100) == 0 and L.pvs_render_workspace_bytes(3, 0) == 0
    assert L.pvs_render_workspace_bytes(3, 100) == 3 * 100 * 32          # three binary64 and two int32 per (pose, vertex)
    assert L.pvs_vsd_workspace_bytes(2, 2, 2, 540, 720, 0) == 0          # 'step': integers only
    assert L.pvs_vsd_workspace_bytes(2, 2, 2, 540, 720, 1) == 8 * 8 * -(-540 * 720 // 256)
    assert L.pvs_vsd_workspace_bytes(0, 2, 2, 540, 720, 1) == 0
    render = L.pvs_render_depth_batched
    render.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 6 + [ctypes.c_double] * 2 + [ctypes.c_void_p]
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 100.0, 1e4, None) == 0      # no pose: nothing to do
    assert render(None, None, None, None, None, None, 2, 5, 4, 0, 64, 48, 100.0, 1e4, None) == -1     # null pointers
    assert render(None, None, None, None, None, None, -1, 5, 4, 0, 64, 48, 100.0, 1e4, None) == -1
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 0, 48, 100.0, 1e4, None) == -1      # empty image
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 16385, 100.0, 1e4, None) == -1  # beyond PVS_MAX_SIDE
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 0.0, 1e4, None) == -1       # near must be positive
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 100.0, 50.0, None) == -1    # far < near
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, float("nan"), 1e4, None) == -1
    vsd = L.pvs_vsd_batched
    vsd.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 +
                    [ctypes.c_void_p])
    args = lambda n, kind=0, cost=0, H=48, W=64: (None, None, None, kind, 0.1, None, 0, 15.0, 20.0, cost, None, None, None,   # noqa: E731
                                                  n, 2, 2, H, W, None)
    assert vsd(*args(0)) == 0
    assert vsd(*args(1)) == -1                                           # null pointers
    assert vsd(*args(0, kind=3)) == -1 and vsd(*args(0, cost=2)) == -1 and vsd(*args(0, H=0)) == -1
    assert vsd(*args(20000)) == -1                                       # more pairs than a grid dimension holds


def test_no_cpu_fallback(pkg):
    import torch
    from clean_pvnet_amd import vsd
    pts, faces = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)
    P, K = torch.eye(3, 4, dtype=torch.float64)[None], torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.render_depth(pts, faces, P, K, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.vsd(P[None], P[None], torch.zeros(1, 8, 8, dtype=torch.uint16), K, pts, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.VsdEvaluator(np.zeros((5, 3), np.float32), np.zeros((2, 3), np.int32), (8, 8), device="cpu")
