"""From a mesh's vertices to the metadata every later stage consumes, on the device (``libpvnet_vote.so``, the last section of
include/pvnet_vote.h): the farthest-point keypoints ``fps_3d`` (the vote targets and the PnP model points), the bounding box
``corner_3d`` / ``center_3d`` and the diameter (the ADD threshold of every evaluator).

The reference does this on the host: ``tools/handle_custom_dataset.py:19-40, 94`` with ``lib/csrc/fps`` (plain C++) and the
O(N^2) Python loop ``calc_pts_diameter`` (lib/utils/vsd/misc.py:139-154).  Here a padded batch of clouds goes through HIP
kernels: the indices equal the reference's ``farthest_point_sampling.cpp`` and the diameter equals ``calc_pts_diameter`` bit for
bit (the numpy twin is tests/model_twin.py, the reference's own results are tests/golden/model_*.npz).  ``lib/csrc/fps/fps_utils.py``
is the reference's import path on top of this module.  CUDA tensors, the current stream, nothing read back, no CPU fallback.
"""
import numbers
import random

import torch

from . import _native

AUTO, ONE_BLOCK, TILED = 0, 1, 2     # PVV_FPS_*: ONE_BLOCK runs all rounds in one launch (N <= ONE_BLOCK_MAX), TILED one launch per round
ONE_BLOCK_MAX = 8192                 # PVV_FPS_ONE_BLOCK_MAX
TILE = 1024                          # PVV_MODEL_TILE
MAX_N = 1 << 20                      # PVV_MODEL_MAX_N

_lib = _native.bind("model", "libpvnet_vote.so", last_error="pvv_last_error")


def _clouds(points, dtypes):
    """``points`` as a contiguous [B, N, 3] tensor and whether it came as [N, 3]."""
    _native.check_tensors([("points", points)], dtypes, "model", {"points": " or ".join(str(d) for d in dtypes)})
    single = points.dim() == 2
    p = points[None] if single else points
    if p.dim() != 3 or p.shape[2] != 3 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError("clean_pvnet_amd.model: points must be [B, N, 3] or [N, 3] with B, N >= 1, got %s" % (tuple(points.shape),))
    return p.detach().contiguous(), single


def _lengths(n, B, N, dev):
    """The per-cloud lengths, validated on the host, as (list, int32 device tensor or None)."""
    if n is None:
        return [N] * B, None
    if isinstance(n, torch.Tensor):
        raise TypeError("clean_pvnet_amd.model: n must be a host sequence of ints (it is validated on the host), not a tensor")
    n = [int(v) for v in n]
    if len(n) != B:
        raise ValueError("clean_pvnet_amd.model: n has %d entries for %d clouds" % (len(n), B))
    if any(v < 1 or v > N for v in n):
        raise ValueError("clean_pvnet_amd.model: every entry of n must lie in [1, N = %d], got %s" % (N, n))
    return n, torch.tensor(n, dtype=torch.int32, device=dev)


def farthest_point_sampling(points, sn, init_center=True, start=None, n=None, path=AUTO):
    """The reference's farthest point sampling (lib/csrc/fps/src/farthest_point_sampling.cpp) for a padded batch.
    :param points:       [B, N, 3] float32 CUDA tensor; [N, 3] gives [sn]
    :param sn:           samples per cloud, >= 1; more than a cloud has points is legal (index 0 repeats, as in the reference)
    :param init_center:  True: the first sample is the point farthest from the bounding box's centre
    :param start:        the first sample: an int or a host sequence of B ints, each in [0, n_b); needs init_center=False.
                         With init_center=False and no start, one is drawn on the host (the reference's ``rand() % pn``)
    :param n:            host sequence of the B cloud lengths, each in [1, N]; None: every cloud has N points
    :param path:         AUTO, ONE_BLOCK or TILED: both forms give the same indices
    :return:             idx [B, sn] int32
    """
    p, single = _clouds(points, (torch.float32,))
    B, N = p.shape[0], p.shape[1]
    sn = int(sn)
    if sn < 1:
        raise ValueError("clean_pvnet_amd.model: sn must be >= 1, got %d" % sn)
    if path not in (AUTO, ONE_BLOCK, TILED):
        raise ValueError("clean_pvnet_amd.model: path must be AUTO, ONE_BLOCK or TILED")
    lens, d_n = _lengths(n, B, N, p.device)
    d_start = None
    if init_center:
        if start is not None:
            raise ValueError("clean_pvnet_amd.model: start replaces the random first sample: it needs init_center=False")
    else:
        if start is None:
            start = [random.randrange(v) for v in lens]
        elif isinstance(start, torch.Tensor):
            raise TypeError("clean_pvnet_amd.model: start must be an int or a host sequence of ints, not a tensor")
        start = [int(start)] * B if isinstance(start, numbers.Integral) else [int(v) for v in start]
        if len(start) != B:
            raise ValueError("clean_pvnet_amd.model: start has %d entries for %d clouds" % (len(start), B))
        if any(s < 0 or s >= v for s, v in zip(start, lens)):
            raise ValueError("clean_pvnet_amd.model: every start must lie in [0, n_b), got %s for lengths %s" % (start, lens))
        d_start = torch.tensor(start, dtype=torch.int32, device=p.device)
    ws, nbytes = _lib.workspace("pvv_fps_workspace_bytes", p.device, B, N, sn, path)
    idx = torch.empty(B, sn, dtype=torch.int32, device=p.device)
    _lib.call("pvv_fps", p.device, p.data_ptr(), _native.ptr(d_n), _native.ptr(d_start), B, N, sn, path, ws.data_ptr(), nbytes, idx.data_ptr())
    return idx[0] if single else idx


def bounds(points, n=None):
    """(lo [B,3], hi [B,3]): the coordinate-wise minima and maxima, in the dtype of ``points`` (float32 or float64)."""
    p, _ = _clouds(points, (torch.float32, torch.float64))
    B, N = p.shape[0], p.shape[1]
    _, d_n = _lengths(n, B, N, p.device)
    ws, nbytes = _lib.workspace("pvv_model_workspace_bytes", p.device, B, N)
    lo, hi = torch.empty(B, 3, dtype=p.dtype, device=p.device), torch.empty(B, 3, dtype=p.dtype, device=p.device)
    _lib.call("pvv_model_bounds", p.device, p.data_ptr(), int(p.dtype == torch.float64), _native.ptr(d_n), B, N, ws.data_ptr(), nbytes,
              lo.data_ptr(), hi.data_ptr())
    return lo, hi


def _corners(lo, hi):
    """tools/handle_custom_dataset.py:30-39: x is the slowest coordinate, min before max."""
    box = torch.stack([lo, hi], 1)                                                  # [B, 2, 3]
    sel = torch.tensor([[i >> 2 & 1, i >> 1 & 1, i & 1] for i in range(8)], device=lo.device)
    return torch.stack([box[:, sel[:, c], c] for c in range(3)], 2)                # [B, 8, 3]


def model_corners(points, n=None):
    """[B, 8, 3]: the corners of the bounding box in the row order of ``get_model_corners`` (handle_custom_dataset.py:26-40)."""
    return _corners(*bounds(points, n))


def model_center(points, n=None):
    """[B, 3]: ``(hi + lo) / 2`` (handle_custom_dataset.py:94)."""
    lo, hi = bounds(points, n)
    return (hi + lo) / 2


def diameter(points, n=None):
    """[B] float64: the largest distance between two points of each cloud, ``calc_pts_diameter`` (lib/utils/vsd/misc.py:139-154)
    bit for bit for float64 points; float32 points are widened exactly.  One launch over the pairs of 1024-point tiles."""
    p, _ = _clouds(points, (torch.float32, torch.float64))
    B, N = p.shape[0], p.shape[1]
    _, d_n = _lengths(n, B, N, p.device)
    ws, nbytes = _lib.workspace("pvv_model_workspace_bytes", p.device, B, N)
    out = torch.empty(B, dtype=torch.float64, device=p.device)
    _lib.call("pvv_model_diameter", p.device, p.data_ptr(), int(p.dtype == torch.float64), _native.ptr(d_n), B, N, ws.data_ptr(), nbytes,
              out.data_ptr())
    return out


def model_meta(points, sn=8, n=None):
    """What ``custom_to_coco`` (handle_custom_dataset.py:86-104) collects per model, for a batch, on one stream:
    ``fps_idx`` [B,sn] int32, ``fps_3d`` [B,sn,3], ``corner_3d`` [B,8,3], ``center_3d`` [B,3], ``diameter`` [B] float64."""
    p, _ = _clouds(points, (torch.float32,))
    idx = farthest_point_sampling(p, sn, True, n=n)
    lo, hi = bounds(p, n)
    return {"fps_idx": idx, "fps_3d": torch.gather(p, 1, idx.long()[:, :, None].expand(-1, -1, 3)),
            "corner_3d": _corners(lo, hi), "center_3d": (hi + lo) / 2, "diameter": diameter(p, n)}
