"""GPU: the HIP path against the committed golden fixtures produced by the reference's own Python glue
(tests/golden/make_golden.py).  Tolerance: tests/tolerances.py -- 1e-4 abs + 2e-6 rel, plus the reference's OWN measured
deviation from the exact (rational) least-squares solution of the same inlier set (its binary32 accumulation)."""

import numpy as np
import pytest
import torch

from tests import fixtures
from tests import tolerances as tol

pytestmark = pytest.mark.gpu


def gold(name, gpu):
    c = fixtures.load(name)
    t = {k: torch.from_numpy(v).to(gpu) for k, v in c.items() if isinstance(v, np.ndarray) and v.ndim > 0}
    return c, t


def test_v3_basic(oracle, pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3
    c, t = gold("v3_basic", gpu)
    out = ransac_voting_layer_v3(t["mask"], t["vertex"], int(c["hn"]), inlier_thresh=float(c["thresh"]), idxs=t["idxs"])
    exact = tol.exact_v3(oracle, c["mask"], c["vertex"], int(c["hn"]), float(c["thresh"]), c["idxs"])
    tol.assert_means_close(out.cpu().numpy(), exact)                                   # within the contract of the exact answer
    tol.assert_means_close(out.cpu().numpy(), c["out"], extra=np.abs(c["out"] - exact))
    assert (out[2] == 0).all()


def test_v3_subsample(oracle, pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3
    c, t = gold("v3_subsample", gpu)
    out = ransac_voting_layer_v3(t["mask"], t["vertex"], int(c["hn"]), inlier_thresh=float(c["thresh"]),
                                 max_num=int(c["max_num"]), idxs=t["idxs"], selection=t["selection"])
    exact = tol.exact_v3(oracle, c["mask"], c["vertex"], int(c["hn"]), float(c["thresh"]), c["idxs"], selection=c["selection"],
                         max_num=int(c["max_num"]))
    tol.assert_means_close(out.cpu().numpy(), exact)
    tol.assert_means_close(out.cpu().numpy(), c["out"], extra=np.abs(c["out"] - exact))
    assert np.abs(c["out"] - exact).max() > 1e-4        # the fixture where the reference's own rounding exceeds the contract


def test_v3_bytemask(oracle, pkg, gpu):
    """uint8 mask of 255s: foreground_num = sum of the byte values (P:126) decides the subsampling (P:135-138)."""
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3
    c, t = gold("v3_bytemask", gpu)
    out = ransac_voting_layer_v3(t["mask"], t["vertex"], int(c["hn"]), inlier_thresh=float(c["thresh"]),
                                 max_num=int(c["max_num"]), idxs=t["idxs"], selection=t["selection"])
    exact = tol.exact_v3(oracle, c["mask"], c["vertex"], int(c["hn"]), float(c["thresh"]), c["idxs"], selection=c["selection"],
                         max_num=int(c["max_num"]))
    tol.assert_means_close(out.cpu().numpy(), exact)
    tol.assert_means_close(out.cpu().numpy(), c["out"], extra=np.abs(c["out"] - exact))
    assert t["mask"].max().item() == 255            # the input is not subsampled in place (the reference does that to a uint8 mask)


def test_estimate_subsample(pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import estimate_voting_distribution_with_mean
    c, t = gold("estimate_subsample", gpu)
    mean, cov = estimate_voting_distribution_with_mean(t["mask"], t["vertex"], t["mean"], int(c["round_hyp_num"]),
                                                       int(c["min_hyp_num"]), max_num=int(c["max_num"]), idxs=t["idxs"],
                                                       selection=t["selection"])
    tol.assert_cov_close(cov.cpu().numpy(), c["cov"], rtol=tol.COV_RTOL_VS_REFERENCE_F32, what="cov vs the reference's float32 glue")


def test_v3_singular_reference_policy_is_default(oracle, pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3
    c, t = gold("v3_singular", gpu)
    out = ransac_voting_layer_v3(t["mask"], t["vertex"], int(c["hn"]), inlier_thresh=float(c["thresh"]), idxs=t["idxs"])
    exact = tol.exact_v3(oracle, c["mask"], c["vertex"], int(c["hn"]), float(c["thresh"]), c["idxs"])
    tol.assert_means_close(out.cpu().numpy(), exact)
    tol.assert_means_close(out.cpu().numpy(), c["out"], extra=np.abs(c["out"] - exact))


def test_v1_layer(oracle, pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer
    c, t = gold("v1_basic", gpu)
    out = ransac_voting_layer(t["mask"], t["vertex"], int(c["hn"]), inlier_thresh=float(c["thresh"]), idxs=t["idxs"])
    exact = tol.exact_v3(oracle, c["mask"], c["vertex"], int(c["hn"]), float(c["thresh"]), c["idxs"], singular="image_zero")
    tol.assert_means_close(out.cpu().numpy(), exact)                                   # within the contract of the exact answer (VERDICT r2 #2b)
    tol.assert_means_close(out.cpu().numpy(), c["out"], extra=np.abs(c["out"] - exact))


def test_estimate(pkg, gpu):
    from clean_pvnet_amd.ransac_voting_gpu import estimate_voting_distribution_with_mean
    c, t = gold("estimate_basic", gpu)
    mean, cov = estimate_voting_distribution_with_mean(t["mask"], t["vertex"], t["mean"], int(c["round_hyp_num"]),
                                                       int(c["min_hyp_num"]), idxs=t["idxs"])
    tol.assert_cov_close(cov.cpu().numpy(), c["cov"], rtol=tol.COV_RTOL_VS_REFERENCE_F32, what="cov vs the reference's float32 glue")
    assert mean is t["mean"]
