"""Pose from keypoints for a whole batch on the device, start included (``libpvnet_pose.so``, include/pvnet_pose.h).

The reference computes the pose per image on the host, after the keypoints were copied back:
  * by default ``pvnet_pose_utils.pnp(kpt_3d, kpt_2d, K)`` (lib/utils/pvnet/pvnet_pose_utils.py:5-38), i.e.
    ``cv2.solvePnP(..., SOLVEPNP_ITERATIVE)``: a DLT start, then Levenberg-Marquardt on the reprojection error;
  * with ``cfg.test.un_pnp`` ``un_pnp_utils.uncertainty_pnp`` (lib/csrc/uncertainty_pnp/un_pnp_utils.py:6-57): P3P on the
    four best-weighted keypoints, then the uncertainty-weighted refinement.
Here both run for the batch in one launch on the current stream, reading ``output['kpt_2d']`` (and ``var_weights``) where
``decode_keypoint`` left them: no copy to the host, no synchronisation.  The starts are the device forms of
``un_pnp_utils.initial_pose_p3p`` / ``initial_pose_dlt``; the refinement is the kernel of ``uncertainty_pnp_batched``.
A planar object model (OpenCV would take a homography start there) and fewer than six keypoints for the DLT have no start:
those images come back as NaN with their status.  There is no CPU fallback.
"""
import numpy as np

from . import _native

_lib = _native.bind("pose", "libpvnet_pose.so")

METHODS = {"p3p": 0, "dlt": 1}                    # PVP_START_P3P, PVP_START_DLT
# d_status codes (PVP_STATUS_*): >= 0 a start was found, < 0 the image's outputs are NaN
STATUS = {0: "p3p", 1: "dlt", 2: "dlt_fallback", -1: "no_start", -2: "planar", -3: "nonfinite"}


def _inputs(points_2d, points_3d, camera_matrix, weights_2d):
    import torch
    dev = points_2d.device
    assert dev.type == "cuda", "clean_pvnet_amd.pose needs CUDA tensors (no CPU path exists)"
    f64 = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float64).contiguous()   # noqa: E731
    p2, p3, Km, w2 = f64(points_2d), f64(points_3d), f64(camera_matrix), f64(weights_2d)
    b, pn = p2.shape[0], p2.shape[1]
    assert p2.shape == (b, pn, 2), p2.shape
    assert p3.shape in ((pn, 3), (b, pn, 3)) and Km.shape in ((3, 3), (b, 3, 3)), (p3.shape, Km.shape)
    assert w2 is None or w2.shape == (b, pn, 3), w2.shape
    if not 4 <= pn <= 4096:
        raise ValueError("pose: %d keypoints, supported are 4 to 4096" % pn)
    return dev, p2, p3, Km, w2, b, pn


def initial_pose_batched(points_2d, points_3d, camera_matrix, weights_2d=None, method="p3p"):
    """The start alone, for a batch, on the device (one launch on the current stream, nothing read back).
    :param points_2d:      [b,pn,2] CUDA tensor, any float dtype
    :param points_3d:      [pn,3] (one object model) or [b,pn,3]
    :param camera_matrix:  [3,3] or [b,3,3]
    :param weights_2d:     [b,pn,3] (wxx,wxy,wyy); "p3p" needs it (its key is wxx + wxy), "dlt" does not read it
    :param method:         "p3p" (``un_pnp_utils.initial_pose_p3p``, DLT fallback) or "dlt" (``initial_pose_dlt``)
    :return:               rt [b,6] float64 (angle-axis, translation; NaN without a start), status [b] int32 (``STATUS``)
    """
    import torch
    if method not in METHODS:
        raise ValueError("method must be one of %s" % sorted(METHODS))
    if method == "p3p" and weights_2d is None:
        raise ValueError("the P3P start ranks keypoints by their weights: pass weights_2d")
    dev, p2, p3, Km, w2, b, pn = _inputs(points_2d, points_3d, camera_matrix, weights_2d if method == "p3p" else None)
    rt = torch.empty(b, 6, dtype=torch.float64, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    if b == 0:
        return rt, status
    _lib.call("pvp_initial_pose_batched", dev, p2.data_ptr(), p3.data_ptr(), _native.ptr(w2), Km.data_ptr(),
              METHODS[method], rt.data_ptr(), status.data_ptr(), b, pn, int(p3.dim() == 3), int(Km.dim() == 3))
    return rt, status


def pose_batched(points_2d, points_3d, camera_matrix, weights_2d=None, method="dlt", max_iterations=0,
                 function_tolerance=0.0):
    """Start and refinement in one launch (``pvp_pose_batched``).  Without ``weights_2d`` the refinement is unweighted.
    :return: dict of device tensors: ``rt`` [b,6], ``Rt`` [b,3,4], ``init_rt`` [b,6], ``status`` [b] int32 and ``info``
             [b,4] (initial cost, final cost, iterations, termination; NaN where no refinement ran)."""
    import torch
    if method not in METHODS:
        raise ValueError("method must be one of %s" % sorted(METHODS))
    if method == "p3p" and weights_2d is None:
        raise ValueError("the P3P start ranks keypoints by their weights: pass weights_2d")
    dev, p2, p3, Km, w2, b, pn = _inputs(points_2d, points_3d, camera_matrix, weights_2d)
    out = {k: torch.empty(*s, dtype=torch.float64, device=dev) for k, s in
           (("rt", (b, 6)), ("Rt", (b, 3, 4)), ("init_rt", (b, 6)), ("info", (b, 4)))}
    out["status"] = torch.empty(b, dtype=torch.int32, device=dev)
    if b == 0:
        return out
    _lib.call("pvp_pose_batched", dev, p2.data_ptr(), p3.data_ptr(), _native.ptr(w2), Km.data_ptr(), METHODS[method],
              out["rt"].data_ptr(), out["Rt"].data_ptr(), out["init_rt"].data_ptr(), out["status"].data_ptr(),
              out["info"].data_ptr(), b, pn, int(p3.dim() == 3), int(Km.dim() == 3), int(max_iterations),
              float(function_tolerance))
    return out


def pnp_batched(points_3d, points_2d, camera_matrix):
    """The device form of ``pvnet_pose_utils.pnp`` for a batch (same argument order): DLT start, unweighted refinement.
    :param points_3d:      [pn,3] or [b,pn,3]
    :param points_2d:      [b,pn,2] CUDA tensor
    :param camera_matrix:  [3,3] or [b,3,3]
    :return:               Rt [b,3,4] float64 on the device; NaN for an image without a start (pn < 6, planar model)
    """
    return pose_batched(points_2d, points_3d, camera_matrix)["Rt"]


def pnp(points_3d, points_2d, camera_matrix, method=0):
    """Drop-in for ``pvnet_pose_utils.pnp`` (numpy in, [3,4] ``Rt`` out), computed on the GPU.  Only
    ``cv2.SOLVEPNP_ITERATIVE`` (0) is implemented, for non-planar models with >= 6 keypoints."""
    if method != 0:
        raise NotImplementedError("pnp: only SOLVEPNP_ITERATIVE (0) is implemented on the device, not method %r" % (method,))
    import torch
    assert points_3d.shape[0] == points_2d.shape[0], 'points 3D and points 2D must have same number of vertices'
    p2 = torch.as_tensor(np.ascontiguousarray(points_2d, np.float64).reshape(1, -1, 2), device="cuda")
    out = pose_batched(p2, np.ascontiguousarray(points_3d, np.float64), np.asarray(camera_matrix, np.float64))
    status = int(out["status"].item())
    if status < 0:
        raise ValueError("pnp: no pose (%s)" % STATUS[status])
    return out["Rt"][0].cpu().numpy()


def solve_pose(output, kpt_3d, K, un_pnp=False):
    """Sets ``output['pose']`` [b,3,4] float64 (and ``output['pose_status']`` [b] int32) from ``output['kpt_2d']``, on the
    device, without a host synchronisation.  The default is the evaluators' ``pnp(kpt_3d, kpt_2d, K)``
    (evaluators/linemod/pvnet.py:188); ``un_pnp`` is their ``uncertainty_pnp`` branch and reads ``output['var_weights']``
    (``decode_keypoint(..., un_pnp=True, weights=True)``).  ``kpt_3d`` [pn,3] or [b,pn,3] and ``K`` [3,3] or [b,3,3]: pass
    them as CUDA tensors -- numpy arrays are copied to the device first, which synchronises.
    :return: ``output``"""
    if un_pnp:
        out = pose_batched(output["kpt_2d"], kpt_3d, K, weights_2d=output["var_weights"], method="p3p")
    else:
        out = pose_batched(output["kpt_2d"], kpt_3d, K)
    output["pose"] = out["Rt"]
    output["pose_status"] = out["status"]
    return output
