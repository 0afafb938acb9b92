"""The batched ICP refinement (include/pvnet_icp.h, clean_pvnet_amd.icp) without a GPU: the numpy twin of the contract against
fixtures made by the reference's own ``ICPRefiner.refine`` (tests/golden/make_icp_golden.py), the twin's rotation against an
SVD, the cases that leave a pose unchanged, the library's exports and its host-side argument checks.  The GPU tests
(tests/test_gpu_icp.py) then hold the device to the twin bit for bit."""
import os

import numpy as np
import pytest

from tests import capi
from tests import icp_twin as twin
from tests import tolerances as tol
from tests import vsd_twin as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("icp_720", "icp_360", "icp_edge")
SYMBOLS = {"pvi_workspace_bytes", "pvi_refine_batched"}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_module_imports(pkg):
    from clean_pvnet_amd import icp
    assert icp.STATUS == twin.STATUS and callable(icp.refine) and callable(icp.icp_refine) and callable(icp.IcpRefiner)


def test_build_table_has_the_icp_row(pkg):
    import lib
    b = lib.load_build()
    flags, inc = b.HIP_LIBS["icp"]
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags and inc == [b.INCLUDE]
    assert list(b.HIP_LIBS)[-1] == "icp" and len(b.HIP_LIBS) == 7           # with the pybind11 shim: the eighth native library


# ----------------------------------------------------------------------------------------- 1. the twin against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_reproduces_the_reference_fixture(name):
    """Rounds, status and counts exactly; the stage poses under the repository's one tolerance rule, in millimetres for t and
    on the entries of R; and the stored twin poses, which the GPU tests compare the device with, bit for bit."""
    c = load(name)
    r = twin.regenerate(name, c)
    worst_t = worst_R = 0.0
    for p in range(len(c["pose_est"])):
        z_img = vt.sensor_depth(r["raw"][p // r["per_image"]], float(c["depth_scale"]))
        samples = tuple((c["idx"][s, 0, p], c["idx"][s, 1, p]) for s in range(2))
        out, infos, stages = twin.icp_refine(c["pose_est"][p], z_img, r["mask"][p], c["K"], r["pts"], r["faces"], r["size"],
                                             samples=samples, n_max=int(c["n_max"]), tolerance=float(c["tolerance"]),
                                             angle_limit_deg=float(c["angle_limit_deg"]))
        for s in range(2):
            i = infos[s]
            assert [i["status"], i["n_syn"], i["n_real"], i["n"], i["rounds"]] == c["info"][s, p].tolist(), (name, p, s)
            assert i["rounds"] == c["ref_rounds"][s, p]
            tol.assert_means_close(stages[s][:, 3], c["ref_t"][s, p], what="%s pose %d stage %d t (mm)" % (name, p, s))
            tol.assert_means_close(stages[s][:, :3], c["ref_R"][s, p], what="%s pose %d stage %d R" % (name, p, s))
            worst_t = max(worst_t, float(np.abs(stages[s][:, 3] - c["ref_t"][s, p]).max()))
            worst_R = max(worst_R, float(np.abs(stages[s][:, :3] - c["ref_R"][s, p]).max()))
            np.testing.assert_array_equal(_bits(stages[s]), _bits(c["twin_stage"][s, p]))
        np.testing.assert_array_equal(_bits(out), _bits(c["twin_pose"][p]))
        tol.assert_means_close(out[:, 3] * 1000.0, c["ref_pose"][p][:, 3] * 1000.0)
        tol.assert_means_close(out[:, :3], c["ref_pose"][p][:, :3])
    print("%s: largest |twin - reference|: t %.3g mm, R %.3g (stored %s)" % (name, worst_t, worst_R, c["deviation"].tolist()))
    assert [worst_t, worst_R] == c["deviation"].tolist()


def test_fixtures_hold_the_cases_the_checks_need():
    big, half, edge = load("icp_720"), load("icp_360"), load("icp_edge")
    assert tuple(big["size"]) == (720, 540) and bool(big["occluder"]) and big["info"][:, 0, 0].tolist() == [0, 0]
    assert tuple(half["size"]) == (360, 270) and len(half["pose_est"]) == 4 and len(half["scene_seed"]) == 2
    assert (half["info"][:, :, 0] == twin.REFINED).all() and (half["info"][:, :, 4] > 1).all()
    assert edge["info"][:, :, 0].tolist() == [[twin.REFINED, twin.EMPTY_RENDER, twin.NOT_VISIBLE]] * 2
    for c in (big, half, edge):
        assert c["idx"].dtype == np.int32 and c["deviation"].max() < 1e-6         # far inside the tolerance rule
        assert (c["info"][..., 3] <= 3000).all()
    raw = twin.regenerate("icp_720", big)["raw"]
    assert raw.dtype == np.uint16 and (raw == 0).any()                            # holes


# ---------------------------------------------------------------------------------------------- 2. the twin's own arithmetic
def test_twin_rotation_equals_the_svd_with_the_reflection_fix():
    rng = np.random.RandomState(0)
    for k in range(40):
        A = rng.randn(50, 3) * [30.0, 20.0, 5.0]
        R0 = vt.rodrigues(rng.randn(3) * (0.05 if k % 2 else 1.5))
        B = A @ R0.T + rng.randn(50, 3) * 0.5
        if k % 5 == 0:
            B[:, 2] = -B[:, 2]                                                     # the SVD alone would give a reflection
        H = (A - A.mean(0)).T @ (B - B.mean(0))
        U, S, Vt = np.linalg.svd(H)
        R = Vt.T @ U.T
        if np.linalg.det(R) < 0:
            Vt[2, :] *= -1
            R = Vt.T @ U.T
        got = twin.rotation_of(H)
        assert np.abs(got - R).max() < 1e-12, (k, np.abs(got - R).max())
        assert abs(np.linalg.det(got) - 1.0) < 1e-14
    np.testing.assert_array_equal(twin.rotation_of(np.zeros((3, 3))), np.eye(3))


def test_twin_sums_and_draws():
    v = np.random.RandomState(1).randn(1000)
    assert abs(twin.stride_sum(v) - v.sum()) < 1e-10 and twin.stride_sum(v[:3]) == (v[0] + v[2]) + v[1]    # the tree
    assert twin.stride_sum(v[:258]) == twin.stride_sum(np.concatenate([v[:2] + v[256:258], v[2:256]]))          # the stride
    m = np.random.RandomState(2).randn(700, 3, 3)
    np.testing.assert_array_equal(twin.stride_sum(m)[1, 2], twin.stride_sum(m[:, 1, 2]))
    w = np.array([0, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 5], np.int64)                 # only the low 32 bits count
    assert twin.draw(w, 10).tolist() == [0, 5, 9, 0]


def _small_scene(seed=9):
    pts, faces = vt.mesh(seed)
    size, K = (240, 180), vt.camera(1.0 / 3.0)
    gt = vt.pose([0.7, -0.4, 0.2], [0.01, -0.005, 0.68])
    render = vt.render_depth(pts, faces, vt.scaled(gt, 1000.0), K, size)
    raw = vt.scene_depth(900 + seed, render[None], occluder=False)
    return pts, faces, size, K, gt, (render > 0).astype(np.uint8), vt.sensor_depth(raw)


def test_twin_reduces_the_translation_error_on_a_clean_scene():
    pts, faces, size, K, gt, mask, z_img = _small_scene()
    est = np.concatenate([vt.rodrigues([0.02, -0.03, 0.02]) @ gt[:, :3], (gt[:, 3] + [0.003, -0.002, 0.012]).reshape(3, 1)], 1)
    words = np.random.RandomState(4).randint(0, 2 ** 32, (2, 2, 400), dtype=np.int64)
    out, infos, _ = twin.icp_refine(est, z_img, mask, K, pts, faces, size, words=words, n_max=400)
    assert [i["status"] for i in infos] == [twin.REFINED, twin.REFINED] and infos[0]["n"] == 400
    before, after = np.linalg.norm(est[:, 3] - gt[:, 3]), np.linalg.norm(out[:, 3] - gt[:, 3])
    print("translation error %.2f mm -> %.2f mm, rounds %s" % (1e3 * before, 1e3 * after, [i["rounds"] for i in infos]))
    assert after < 0.5 * before


def test_twin_leaves_the_pose_unchanged_with_the_right_status():
    pts, faces, size, K, gt, mask, z_img = _small_scene()
    mm = vt.scaled(gt, 1000.0)
    idx = (np.zeros(100, np.int64), np.zeros(100, np.int64))
    kw = dict(mask=mask, n_max=100, samples=idx)
    away = vt.scaled(vt.pose([0.1, 0.2, 0.3], [2.0, 0.0, 0.7]), 1000.0)
    behind = mm.copy()
    behind[2, 3] = -680.0
    nan = mm.copy()
    nan[0, 1] = np.nan
    few = np.zeros_like(mask)
    few[np.nonzero(mask.any(1))[0][0]] = 1                                         # one row of the object
    for pose, kwargs, want in ((away, kw, twin.EMPTY_RENDER), (behind, kw, twin.BAD_POSE), (nan, kw, twin.BAD_POSE),
                               (mm, dict(kw, mask=few & mask), twin.NOT_VISIBLE),
                               (mm, dict(kw, min_mask_pixels=int(mask.sum()) + 1), twin.SMALL_MASK),
                               (mm, dict(kw, samples=(idx[0], idx[1] + 10 ** 6)), twin.BAD_INDEX),
                               (mm, dict(kw, samples=(idx[0] - 1, idx[1])), twin.BAD_INDEX)):
        out, info = twin.refine(z_img, pose, K, pts, faces, size, **kwargs)
        assert info["status"] == want and info["rounds"] == 0, (twin.STATUS[want], info)
        np.testing.assert_array_equal(_bits(out), _bits(pose))
    out, info = twin.refine(z_img, mm, K, pts, faces, size, **kw)                  # and the same input without a fault runs
    assert info["status"] == twin.REFINED and info["rounds"] >= 1
    # the two-stage recipe returns a pose in metres as it came when stage 1 refuses it
    out, infos, _ = twin.icp_refine(vt.scaled(behind, 1e-3), z_img, mask, K, pts, faces, size, samples=(idx, idx), n_max=100)
    np.testing.assert_array_equal(_bits(out), _bits(vt.scaled(behind, 1e-3)))
    assert [i["status"] for i in infos] == [twin.BAD_POSE, twin.BAD_POSE]


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/utils/icp/icp_utils.py"),
                    reason="the reference tree exists only in the build container")
def test_icp_fixtures_are_reproducible_from_the_reference():
    """tests/golden/make_icp_golden.py, run here against the reference where it lies, regenerates every committed fixture with
    identical content (it never rewrites an existing file without --force)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_icp_golden.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " exists," in l]
    assert len(lines) == len(FIXTURES) and all(l.endswith("identical content") for l in lines), out.stdout


# ------------------------------------------------------------------------------------------- 3. the library and its arguments
def test_icp_library_exports_what_the_header_declares():
    names = capi.declared("icp")
    assert names == SYMBOLS
    L = capi.load("icp")
    for n in names:
        assert hasattr(L, n)
    exported = capi.exported("icp")                              # and nothing else is exported
    assert {e for e in exported if not e.startswith("_")} == names, exported


def test_workspace_size_and_argument_errors():
    """Bad arguments are refused before anything is launched (no GPU is needed to be told so)."""
    L = capi.load("icp")
    assert L.pvi_workspace_bytes(0, 540, 720, 3000) == 0 and L.pvi_workspace_bytes(2, 0, 720, 3000) == 0
    assert L.pvi_workspace_bytes(2, 540, 720, 0) == 0 and L.pvi_workspace_bytes(2, 540, 720, 16385) == 0
    one, two = L.pvi_workspace_bytes(1, 540, 720, 3000), L.pvi_workspace_bytes(2, 540, 720, 3000)
    assert 0 < one < two <= 2 * one and two % 16 == 0
    assert one >= 3 * 3 * 3000 * 8 + 12 * 3000 * 12 + 1519 * (24 + 8)            # samples, slab partials, tile sums and counts
    f = L.pvi_refine_batched

    def call(P=0, kind=0, mkind=0, flags=0, n_max=3000, iters=200, tolerance=5e-7, H=48, W=64, per=1):
        return f(None, None, kind, 0.1, per, None, mkind, 1, 0, None, None, 0, None, None, None, flags, 2.0, n_max, iters,
                 tolerance, 0.94, None, None, None, P, H, W, None)

    assert call() == 0                                                   # no pose: nothing to do
    assert call(P=2) == -1                                               # null pointers
    assert call(P=-1) == -1 and call(kind=3) == -1 and call(mkind=3) == -1 and call(flags=4) == -1
    assert call(n_max=0) == -1 and call(n_max=16385) == -1 and call(iters=0) == -1 and call(H=0) == -1 and call(W=16385) == -1
    assert call(tolerance=float("nan")) == -1 and call(per=0) == -1


def test_no_cpu_fallback(pkg):
    import torch
    from clean_pvnet_amd import icp
    pts, faces = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)
    P, K = torch.eye(3, 4, dtype=torch.float64)[None], torch.eye(3, dtype=torch.float64)
    depth = torch.zeros(1, 8, 8, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="clean_pvnet_amd.icp: depth must be a CUDA tensor; there is no CPU fallback"):
        icp.refine(depth, P, K, pts, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        icp.icp_refine(P, depth, None, K, pts, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        icp.IcpRefiner(np.zeros((5, 3), np.float32), np.zeros((2, 3), np.int32), (8, 8), device="cpu")
