"""The batched pose scores (include/pvnet_metrics.h, clean_pvnet_amd.metrics) without a GPU: the library exports what its
header declares, there is no CPU fallback, the fixtures are reproducible from the reference's own evaluator, and the numpy
twin of the arithmetic contract (tests/metrics_twin.py) reproduces every fixture -- which is what lets the GPU tests use the
twin where the fixtures have no case."""
import os

import numpy as np
import pytest

from tests import capi
from tests import metrics_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
POSE_FIXTURES = ("metrics_n5841", "metrics_n777")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_metrics_library_exports_what_the_header_declares():
    names = capi.declared("metrics")
    assert names == {"pvm_adds_slabs", "pvm_workspace_bytes", "pvm_pose_metrics_batched", "pvm_mask_iou_batched"}
    L = capi.load("metrics")
    for n in names:
        assert hasattr(L, n)
    exported = capi.exported("metrics")                          # and nothing else is exported
    assert {e for e in exported if not e.startswith("_")} == names, exported


def test_workspace_size_and_slab_rule():
    L = capi.load("metrics")
    assert L.pvm_workspace_bytes(0, 5841, 0) == 0 and L.pvm_workspace_bytes(4, 0, 0) == 0
    s1, s64 = L.pvm_adds_slabs(1, 5841), L.pvm_adds_slabs(64, 5841)
    assert 6 * s1 >= 512 and 5841 // s1 >= 64                    # B = 1: at least two blocks per compute unit, slabs of >= 64 points
    assert 6 * 64 * s64 >= 512 and s64 <= 8                      # B = 64: a few slabs even out the load of the 384 query tiles
    assert L.pvm_adds_slabs(1024, 5841) == 1 and L.pvm_adds_slabs(1, 1) == 1
    small, large = L.pvm_workspace_bytes(2, 777, 1), L.pvm_workspace_bytes(2, 777, 5)
    assert large - small == 2 * 4 * 777 * 8                      # one 64-bit key per (image, slab, point)
    assert L.pvm_workspace_bytes(2, 777, 10 ** 6) == L.pvm_workspace_bytes(2, 777, 777)
    # bad arguments are refused before anything is launched (no GPU is needed to be told so)
    assert L.pvm_pose_metrics_batched(None, None, None, None, None, None, None, None, 0, 5, 0, 0, None) == 0
    assert L.pvm_pose_metrics_batched(None, None, None, None, None, None, None, None, 2, 5, 0, 0, None) == -1
    assert L.pvm_pose_metrics_batched(None, None, None, None, None, None, None, None, -1, 5, 0, 0, None) == -1


def test_no_cpu_fallback(pkg):
    import torch
    from clean_pvnet_amd import metrics
    P = torch.eye(3, 4, dtype=torch.float64)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.pose_metrics(P, P, torch.zeros(5, 3), torch.eye(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.mask_iou(torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.PoseEvaluator(np.zeros((5, 3), np.float32), 0.1, device="cpu")


@pytest.mark.parametrize("name", POSE_FIXTURES)
def test_twin_reproduces_the_reference_fixture(name):
    c = load(name)
    n, diameter = int(c["n"]), float(c["diameter"])
    model = twin.cloud(n, int(c["cloud_seed"]))
    assert model.shape == (n, 3) and (model[7] == model[3]).all()
    for i, case in enumerate(c["names"]):
        Pp, Pg = c["pose_pred"][i], c["pose_gt"][i]
        got = twin.pose_metrics(Pp, Pg, model, c["K"], symmetric=True)
        if not np.isfinite(Pp).all():
            assert all(np.isnan(got[k]) for k in ("add", "adds", "proj2d", "trans_cm", "ang_deg")) and not got["adds_idx"].any()
            for sym in (False, True):
                assert not any(twin.hits(got, diameter, sym).values())
            assert not (c["hit_add"][i] or c["hit_adds"][i] or c["hit_proj2d"][i] or c["hit_cmd5"][i])
            continue
        np.testing.assert_array_equal(got["adds_idx"], c["adds_idx"][i], err_msg=str(case))
        want = dict(got, **{k: float(c[k][i]) for k in ("add", "adds", "proj2d", "trans_cm", "ang_deg")})
        twin.assert_close(got, want, n, what="%s/%s" % (name, case))
        h, hs = twin.hits(got, diameter, False), twin.hits(got, diameter, True)
        assert (h["add"], hs["add"], h["proj2d"], h["cmd5"]) == (bool(c["hit_add"][i]), bool(c["hit_adds"][i]),
                                                                  bool(c["hit_proj2d"][i]), bool(c["hit_cmd5"][i])), case


def test_twin_search_equals_the_oracle(oracle):
    for n, seed in ((1, 1), (255, 2), (777, 3)):
        model = twin.cloud(n, seed)
        Pp, Pg = twin.pose([0.3, -0.2, 0.1], [0.01, 0.02, 0.8]), twin.pose([0.25, -0.2, 0.15], [0.012, 0.02, 0.81])
        a, b = twin.transform(model, Pp).astype(np.float32), twin.transform(model, Pg).astype(np.float32)
        np.testing.assert_array_equal(twin.nearest(a, b), oracle.find_nearest_point_idx(a, b))
    ref = twin.cloud(50, 4)
    assert twin.nearest(ref, ref[[3, 7]]).tolist() == [3, 3]       # exact duplicates: the lower index wins


def test_mask_fixture_matches_numpy():
    c = load("metrics_masks")
    p, g = c["mask_pred"].astype(np.int64), c["mask_gt"].astype(np.int64)
    np.testing.assert_array_equal((p & g).sum((1, 2)), c["inter"])
    np.testing.assert_array_equal((p | g).sum((1, 2)), c["union"])
    with np.errstate(all="ignore"):
        iou = c["inter"] / c["union"]
    np.testing.assert_array_equal(iou > 0.7, c["hit_ap"])
    assert np.isnan(iou[-1]) and c["union"][-1] == 0


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/evaluators/linemod/pvnet.py"),
                    reason="the reference tree exists only in the build container")
def test_metrics_fixtures_are_reproducible_from_the_reference():
    """tests/golden/make_metrics_golden.py, run here against the reference where it lies, regenerates every committed
    fixture with identical content (it never rewrites an existing file without --force)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_metrics_golden.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " exists," in l]
    assert len(lines) == 3 and all(l.endswith("identical content") for l in lines), out.stdout
