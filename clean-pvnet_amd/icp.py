"""ICP pose refinement for a whole batch on the device (``libpvnet_icp.so``, include/pvnet_icp.h).

The reference refines one image at a time on the host: ``Evaluator.icp_refine`` (lib/evaluators/linemod/pvnet.py:102-116,
tless_test/pvnet.py:143-158, custom/pvnet.py:75-86) calls ``ICPRefiner.refine`` twice (lib/utils/icp/icp_utils.py:134-176) --
an OpenGL depth render, two numpy point clouds, a radius filter, a draw of up to 3000 points from each and up to 200 rounds of
a scikit-learn nearest-neighbour search with an SVD fit (``icp``, :83-126).  Here ``refine`` is one such stage for ``P`` poses:
the renders come from ``vsd.render_depth``, the clouds are never written, the samples are picked by rank, and the rounds are
launches on the current stream that a converged pose leaves at once.  ``icp_refine`` is the evaluators' two-stage recipe;
its result feeds ``metrics.pose_metrics`` and ``vsd.vsd`` unchanged.  Nothing is read back.  There is no CPU fallback.
"""
import math

from . import _native
from . import vsd as _vsd

_lib = _native.bind("icp", "libpvnet_icp.so")

STATUS = ("refined", "empty_render", "not_visible", "rotation_limit", "bad_pose", "small_mask", "bad_index")   # PVI_REFINED ...
INFO = ("status", "n_syn", "n_real", "n", "rounds")                                                            # PVI_STATUS ...
MAX_SAMPLES = 16384                                                                                            # PVI_MAX_SAMPLES
_UNCHANGED_AT_ONCE = 4            # a status from PVI_BAD_POSE on ends icp_refine with the pose as it came


def _mask_arg(mask, P, H, W):
    """(tensor, PVI_MASK_* kind, poses per mask)."""
    import torch
    if mask is None:
        return None, 0, 1
    _native.need_cuda(mask, "mask", "icp")
    if mask.dtype == torch.bool:
        m, kind = mask.contiguous().view(torch.uint8), 1
    elif mask.dtype == torch.uint8:
        m, kind = mask.contiguous(), 1
    elif mask.dtype == torch.int64:
        m, kind = mask.contiguous(), 2
    else:
        raise TypeError("icp: mask has dtype %s, supported are uint8, bool and int64" % mask.dtype)
    assert m.dim() == 3 and tuple(m.shape[1:]) == (H, W) and m.shape[0] > 0 and P % m.shape[0] == 0, (m.shape, P, H, W)
    return m, kind, P // m.shape[0]


def refine(depth, pose, K, pts, faces, *, mask=None, depth_only=False, no_depth=False, max_mean_dist_factor=2.0, n_max=3000,
           max_iterations=200, tolerance=5e-7, angle_limit_deg=20.0, depth_scale=1.0, near=100., far=10000., samples=None,
           generator=None, return_info=False, min_mask_pixels=0):
    """One stage of ``ICPRefiner.refine`` (icp_utils.py:134-176) for ``P`` poses, on the device, nothing read back.
    :param depth:   [n,H,W] CUDA tensor, the sensor images, ``P`` a multiple of ``n``: pose ``p`` looks at image
                    ``p // (P // n)``.  uint16 scaled by ``depth_scale`` on the device, or float32 / float64 in model units
    :param pose:    [P,3,4] CUDA tensor [R | t], t in the units of ``pts``
    :param K:       [3,3] or [P,3,3]
    :param pts, faces:  the model, as for ``vsd.render_depth``
    :param mask:    [m,H,W] uint8, bool or int64 (``P`` a multiple of ``m``): the sensor pixels whose mask is not 1 are
                    dropped (tless_test/pvnet.py:150); a mask with fewer than ``min_mask_pixels`` ones leaves its pose unchanged
    :param depth_only, no_depth, max_mean_dist_factor:  as the reference's arguments
    :param samples: (idx_syn, idx_real), two [P,n_max] int32 CUDA tensors of point ranks to use instead of a draw
    :param generator:  a CUDA ``torch.Generator`` for the draw
    :return:        [P,3,4] float64; with ``return_info`` also a dict of [P] int32 tensors ``status`` (index into ``STATUS``),
                    ``n_syn``, ``n_real``, ``n`` and ``rounds``
    """
    import torch
    for t, what in ((depth, "depth"), (pose, "pose"), (K, "K"), (pts, "pts"), (faces, "faces")):
        _native.need_cuda(t, what, "icp")
    dt, kind = _vsd._test_image(depth, depth_scale)
    dev = pose.device
    ps = pose.to(dtype=torch.float64).contiguous()
    P = ps.shape[0]
    assert ps.shape == (P, 3, 4), ps.shape
    assert dt.dim() == 3 and dt.shape[0] > 0 and P % dt.shape[0] == 0, (dt.shape, P)
    H, W = int(dt.shape[1]), int(dt.shape[2])
    _vsd._check_size((W, H))
    Km = K.to(device=dev, dtype=torch.float64).contiguous()
    assert Km.shape in ((3, 3), (P, 3, 3)), Km.shape
    n_max, max_iterations = int(n_max), int(max_iterations)
    if not 0 < n_max <= MAX_SAMPLES:
        raise ValueError("icp: n_max must lie in [1, %d], got %r" % (MAX_SAMPLES, n_max))
    if max_iterations < 1:
        raise ValueError("icp: max_iterations must be at least 1, got %r" % (max_iterations,))
    m, mkind, per_mask = _mask_arg(mask, P, H, W)
    render = _vsd.render_depth(pts, faces, ps, Km, (W, H), near, far)
    idx_syn = idx_real = words = None
    if samples is not None:
        for s in samples:
            _native.need_cuda(s, "samples", "icp")
        idx_syn, idx_real = (s.to(device=dev, dtype=torch.int32).contiguous() for s in samples)
        assert idx_syn.shape == (P, n_max) and idx_real.shape == (P, n_max), (idx_syn.shape, idx_real.shape, n_max)
    else:
        words = torch.randint(0, 2 ** 32, (P, 2, n_max), dtype=torch.int64, device=dev, generator=generator)
    out = torch.empty(P, 3, 4, dtype=torch.float64, device=dev)
    info = torch.empty(P, len(INFO), dtype=torch.int32, device=dev)
    if P:
        flags = (1 if depth_only else 0) | (2 if no_depth else 0)
        ws, _ = _lib.workspace("pvi_workspace_bytes", dev, P, H, W, n_max)
        _lib.call("pvi_refine_batched", dev, render.data_ptr(), dt.data_ptr(), kind, float(depth_scale), P // dt.shape[0],
                  _native.ptr(m), mkind, per_mask, int(min_mask_pixels), ps.data_ptr(), Km.data_ptr(), int(Km.dim() == 3),
                  _native.ptr(idx_syn), _native.ptr(idx_real), _native.ptr(words), flags, float(max_mean_dist_factor), n_max,
                  max_iterations, float(tolerance), math.cos(float(angle_limit_deg) * math.pi / 180.), out.data_ptr(),
                  info.data_ptr(), ws.data_ptr(), P, H, W)
    if return_info:
        return out, {k: info[:, i] for i, k in enumerate(INFO)}
    return out


def icp_refine(pose, depth, mask, K, pts, faces, *, t_scale=1000., min_mask_pixels=0, depth_scale=0.1, samples=None,
               generator=None, return_info=False, **kw):
    """The evaluators' two-stage recipe (``Evaluator.icp_refine``, tless_test/pvnet.py:143-158) for ``P`` poses in metres:
    stage 1 ``depth_only`` with factor 5.0 on ``[R | t * t_scale]``, stage 2 ``no_depth`` with factor 2.0 from stage 1's pose
    with a fresh render; the result is ``[R2 | t1 / t_scale]``, [P,3,4] float64.  A pose with a non-finite entry or
    ``t_z <= 0``, or whose mask has fewer than ``min_mask_pixels`` ones (20 in the T-LESS evaluator), comes back as it was.
    :param samples:  ((idx_syn, idx_real) of stage 1, (idx_syn, idx_real) of stage 2) instead of the draws
    :param kw:       ``n_max``, ``max_iterations``, ``tolerance``, ``angle_limit_deg``, ``near``, ``far`` of ``refine``
    :return:         the poses; with ``return_info`` also the two info dicts of the stages
    """
    import torch
    _native.need_cuda(pose, "pose", "icp")
    p0 = pose.to(dtype=torch.float64)
    mm = torch.cat([p0[:, :, :3], p0[:, :, 3:] * float(t_scale)], 2)
    s1, s2 = samples if samples is not None else (None, None)
    common = dict(mask=mask, depth_scale=depth_scale, min_mask_pixels=min_mask_pixels, generator=generator, return_info=True, **kw)
    r1, i1 = refine(depth, mm, K, pts, faces, depth_only=True, max_mean_dist_factor=5.0, samples=s1, **common)
    r2, i2 = refine(depth, r1, K, pts, faces, no_depth=True, max_mean_dist_factor=2.0, samples=s2, **common)
    # a tensor divisor: torch turns a division by a Python scalar into a multiplication by its reciprocal on the device,
    # which is not the reference's `t / 1000` in the last bit
    out = torch.cat([r2[:, :, :3], r1[:, :, 3:] / torch.full((), float(t_scale), dtype=torch.float64, device=r1.device)], 2)
    out = torch.where((i1["status"] >= _UNCHANGED_AT_ONCE)[:, None, None], p0, out)
    if return_info:
        return out, (i1, i2)
    return out


class IcpRefiner:
    """``ICPRefiner`` (icp_utils.py:129-176) with the model held on the device; ``defaults`` are keyword arguments of
    ``refine`` / ``icp_refine`` applied to every call."""

    def __init__(self, pts, faces, size, device="cuda", **defaults):
        import torch
        self.pts = torch.as_tensor(pts).to(device=device, dtype=torch.float32).contiguous()
        if self.pts.device.type != "cuda":
            raise RuntimeError("clean_pvnet_amd.icp: IcpRefiner needs a CUDA device; there is no CPU fallback")
        self.faces = torch.as_tensor(faces).to(device=device, dtype=torch.int32).contiguous()
        self.size = _vsd._check_size(size)
        self.defaults = defaults

    def _check(self, depth):
        assert tuple(depth.shape[1:]) == (self.size[1], self.size[0]), (depth.shape, self.size)

    def refine(self, depth, pose, K, **kw):
        self._check(depth)
        return refine(depth, pose, K, self.pts, self.faces, **{**self.defaults, **kw})

    def icp_refine(self, pose, depth, mask, K, **kw):
        self._check(depth)
        return icp_refine(pose, depth, mask, K, self.pts, self.faces, **{**self.defaults, **kw})
