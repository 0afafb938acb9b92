"""Depth renders and the Visible Surface Discrepancy for a whole batch on the device (``libpvnet_vsd.so``,
include/pvnet_vsd.h).

The reference scores VSD one pose pair at a time on the host: ``Evaluator.vsd_metric``
(lib/evaluators/tless_test/pvnet.py:66-105) renders the model through an OpenGL context once per predicted and once per
ground-truth pose (lib/utils/renderer/opengl_utils.py:405-492), then runs ``depth_im_to_dist_im``, the two visibility masks
and ``vsd`` (lib/utils/vsd/) in numpy on every pair.  Here ``render_depth`` rasterises a triangle mesh at every pose of a
batch in HIP, ``vsd`` turns the renders and the sensor images into the error of every (prediction, ground truth) pair of every
image (``vsd_from_depth`` is its second half, for renders the caller already holds), and ``VsdEvaluator`` applies the
reference's any-pair rule and counts the hits on the device; nothing is read back before ``summarize()``.  Every call runs
on the current stream in a workspace from the caching allocator.  There is no CPU fallback.
"""
from . import _native

_lib = _native.bind("vsd", "libpvnet_vsd.so")

COSTS = {"step": 0, "tlinear": 1}                                    # PVS_COST_*
COUNTS = ("union", "inter", "cost")                                  # PVS_UNION, PVS_INTER, PVS_COST
MAX_SIDE = 16384                                                     # PVS_MAX_SIDE


def _check_size(size):
    W, H = int(size[0]), int(size[1])
    if not (0 < W <= MAX_SIDE and 0 < H <= MAX_SIDE):
        raise ValueError("size = (W, H) must lie in [1, %d], got %r" % (MAX_SIDE, (W, H)))
    return W, H


def render_depth(pts, faces, pose, K, size, near=100., far=10000.):
    """Depth images of a triangle mesh at ``P`` poses, on the device, nothing read back (replaces
    ``DepthRender.render(im_size, 100, 10000, K, R, t)``, opengl_utils.py:405-492).
    :param pts:    [N,3] CUDA tensor, the model's vertices (taken as float32)
    :param faces:  [F,3] CUDA tensor of vertex indices (taken as int32); a row with an index outside [0, N) is skipped
    :param pose:   [P,3,4] CUDA tensor [R | t], t in the units of ``pts``; a row with a non-finite value gives an empty image
    :param K:      [3,3] or [P,3,3] CUDA tensor
    :param size:   (W, H)
    :return:       [P,H,W] float32: the eye-space Z of the nearest surface within [near, far], 0 = background.  Pixel (x, y)
                   is sampled at (x + 0.5, y + 0.5); the exact contract is in include/pvnet_vsd.h.
    """
    import torch
    for t, what in ((pts, "pts"), (faces, "faces"), (pose, "pose"), (K, "K")):
        _native.need_cuda(t, what, "vsd")
    W, H = _check_size(size)
    if not (float(near) > 0.0 and float(far) >= float(near)):
        raise ValueError("0 < near <= far is required, got near=%r far=%r" % (near, far))
    dev = pose.device
    md = pts.to(device=dev, dtype=torch.float32).contiguous()
    fc = faces.to(device=dev, dtype=torch.int32).contiguous()
    ps = pose.to(dtype=torch.float64).contiguous()
    Km = K.to(device=dev, dtype=torch.float64).contiguous()
    P = ps.shape[0]
    assert ps.shape == (P, 3, 4), ps.shape
    assert md.dim() == 2 and md.shape[1] == 3 and md.shape[0] > 0, md.shape
    assert fc.dim() == 2 and fc.shape[1] == 3, fc.shape
    assert Km.shape in ((3, 3), (P, 3, 3)), Km.shape
    depth = torch.empty(P, H, W, dtype=torch.float32, device=dev)
    if P:
        ws, _ = _lib.workspace("pvs_render_workspace_bytes", dev, P, md.shape[0])
        _lib.call("pvs_render_depth_batched", dev, md.data_ptr(), fc.data_ptr() if fc.shape[0] else None, ps.data_ptr(),
                  Km.data_ptr(), depth.data_ptr(), ws.data_ptr(), P, md.shape[0], fc.shape[0], int(Km.dim() == 3), W, H,
                  float(near), float(far))
    return depth


_TEST_KINDS = None


def _test_image(depth_test, depth_scale):
    """The sensor image as (tensor, PVS_TEST_* kind)."""
    import torch
    global _TEST_KINDS
    if _TEST_KINDS is None:
        _TEST_KINDS = {torch.uint16: 0, torch.float32: 1, torch.float64: 2}
    _native.need_cuda(depth_test, "depth_test", "vsd")
    if depth_test.dtype not in _TEST_KINDS:
        raise TypeError("vsd: depth_test has dtype %s, supported are uint16, float32 and float64" % depth_test.dtype)
    kind = _TEST_KINDS[depth_test.dtype]
    if kind != 0 and float(depth_scale) != 1.0:
        raise ValueError("vsd: a floating-point depth_test is taken in model units; pass depth_scale=1")
    return depth_test.contiguous(), kind


def vsd(pose_est, pose_gt, depth_test, K, pts, faces, *, delta=15., tau=20., cost="step", depth_scale=0.1, t_scale=1000.,
        near=100., far=10000., gt_valid=None, return_images=False):
    """The VSD error of every (prediction, ground truth) pair of every image, on the device, nothing read back
    (``Evaluator.vsd_metric``, tless_test/pvnet.py:66-105, without its early return).  Every pose is rendered once.
    :param pose_est:    [n,p,3,4] CUDA tensor, the predictions of each image
    :param pose_gt:     [n,g,3,4] the ground-truth poses of each image
    :param depth_test:  [n,H,W] the sensor images: uint16 scaled by ``depth_scale`` on the device, or float32 /
                        float64 already in model units with ``depth_scale=1``
    :param K:           [3,3] or [n,3,3]
    :param pts, faces:  the model, as for ``render_depth``
    :param delta, tau, cost:  ``tless_config.vsd_delta``, ``vsd_tau``, ``vsd_cost`` ('step' or 'tlinear')
    :param t_scale:     the translations are multiplied by it before rendering (the evaluator's ``* 1000``, :84, :91)
    :param gt_valid:    [n,g] bool CUDA tensor: ``e`` is NaN for the pairs of an unset slot (padding of images with fewer
                        instances), so any comparison with it is a miss
    :param return_images:  also return a dict with ``depth_est`` [n,p,H,W], ``depth_gt`` [n,g,H,W] and the per-pair
                        ``union``, ``inter``, ``cost`` counts [n,p,g] int64
    :return:            e [n,p,g] float64
    """
    import torch
    for t, what in ((pose_est, "pose_est"), (pose_gt, "pose_gt"), (K, "K"), (depth_test, "depth_test")):
        _native.need_cuda(t, what, "vsd")
    dev = pose_est.device
    n, p = pose_est.shape[:2]
    g = pose_gt.shape[1]
    assert pose_est.shape == (n, p, 3, 4) and pose_gt.shape == (n, g, 3, 4), (pose_est.shape, pose_gt.shape)
    assert depth_test.dim() == 3 and depth_test.shape[0] == n, depth_test.shape
    H, W = int(depth_test.shape[1]), int(depth_test.shape[2])
    Km = K.to(device=dev, dtype=torch.float64).contiguous()
    assert Km.shape in ((3, 3), (n, 3, 3)), Km.shape
    # the sensor image, cost, gt_valid and the image size are checked by render_depth and vsd_from_depth
    # one render per pose: the n*p predictions, then the n*g ground truths
    poses = torch.cat([pose_est.to(torch.float64).reshape(n * p, 3, 4), pose_gt.to(device=dev, dtype=torch.float64).reshape(n * g, 3, 4)])
    poses = torch.cat([poses[:, :, :3], poses[:, :, 3:] * float(t_scale)], 2)
    if Km.dim() == 3:
        Kp = torch.cat([Km.repeat_interleave(p, 0), Km.repeat_interleave(g, 0)])
    else:
        Kp = Km
    depth = render_depth(pts, faces, poses, Kp, (W, H), near, far)
    depth_est, depth_gt = depth[:n * p].view(n, p, H, W), depth[n * p:].view(n, g, H, W)
    e, counts = vsd_from_depth(depth_est, depth_gt, depth_test, Km, delta=delta, tau=tau, cost=cost, depth_scale=depth_scale,
                               gt_valid=gt_valid, return_counts=True)
    if return_images:
        images = {"depth_est": depth_est, "depth_gt": depth_gt}
        images.update(counts)
        return e, images
    return e


def vsd_from_depth(depth_est, depth_gt, depth_test, K, *, delta=15., tau=20., cost="step", depth_scale=0.1, gt_valid=None,
                   return_counts=False):
    """The second half of ``vsd``: the error of every pair from depth images the caller already holds (renders of
    ``render_depth`` or of any other renderer with its conventions: eye-space Z in model units, 0 = background).
    :param depth_est:   [n,p,H,W] float32 CUDA tensor, the renders of the predictions of each image
    :param depth_gt:    [n,g,H,W] float32, the renders of the ground-truth poses
    :param depth_test, K, delta, tau, cost, depth_scale, gt_valid:  as for ``vsd``
    :param return_counts:  also return a dict with the per-pair ``union``, ``inter``, ``cost`` counts [n,p,g] int64
    :return:            e [n,p,g] float64
    """
    import torch
    for t, what in ((depth_est, "depth_est"), (depth_gt, "depth_gt"), (K, "K")):
        _native.need_cuda(t, what, "vsd")
    if cost not in COSTS:
        raise ValueError("vsd: cost must be 'step' or 'tlinear', got %r" % (cost,))
    dt, kind = _test_image(depth_test, depth_scale)
    for t, what in ((depth_est, "depth_est"), (depth_gt, "depth_gt")):
        if t.dtype != torch.float32:
            raise TypeError("vsd: %s has dtype %s, the renders are float32" % (what, t.dtype))
    assert depth_est.dim() == 4 and depth_gt.dim() == 4, (depth_est.shape, depth_gt.shape)
    dev = depth_est.device
    n, p, H, W = (int(v) for v in depth_est.shape)
    g = int(depth_gt.shape[1])
    assert tuple(depth_gt.shape) == (n, g, H, W), (depth_est.shape, depth_gt.shape)
    assert tuple(dt.shape) == (n, H, W), dt.shape
    _check_size((W, H))
    Km = K.to(device=dev, dtype=torch.float64).contiguous()
    assert Km.shape in ((3, 3), (n, 3, 3)), Km.shape
    if gt_valid is not None:
        _native.need_cuda(gt_valid, "gt_valid", "vsd")
        assert gt_valid.shape == (n, g), gt_valid.shape
    depth_est, depth_gt = depth_est.contiguous(), depth_gt.contiguous()
    counts = torch.empty(n, p, g, 3, dtype=torch.int64, device=dev)
    e = torch.empty(n, p, g, dtype=torch.float64, device=dev)
    if n * p * g:
        ws, _ = _lib.workspace("pvs_vsd_workspace_bytes", dev, n, p, g, H, W, COSTS[cost])
        _lib.call("pvs_vsd_batched", dev, depth_est.data_ptr(), depth_gt.data_ptr(), dt.data_ptr(), kind,
                  float(depth_scale), Km.data_ptr(), int(Km.dim() == 3), float(delta), float(tau), COSTS[cost],
                  counts.data_ptr(), e.data_ptr(), ws.data_ptr(), n, p, g, H, W)
    if gt_valid is not None:
        e = torch.where((gt_valid != 0)[:, None, :], e, torch.full_like(e, float("nan")))
    if return_counts:
        return e, {k: counts[..., i] for i, k in enumerate(COUNTS)}
    return e


class VsdEvaluator:
    """``Evaluator.vsd_metric`` with its bookkeeping (tless_test/pvnet.py:66-105, :258-267) on the device: an image is a hit
    when any of its (prediction, ground truth) pairs has ``e < error_thresh``.  ``evaluate`` adds the hits of a batch to
    int64 counters without a synchronisation; ``summarize`` is the one place that reads back.  ``last`` holds ``e`` [n,p,g]
    and the per-image hits of the latest ``evaluate`` as device tensors."""

    def __init__(self, pts, faces, size, error_thresh=0.3, delta=15., tau=20., cost="step", depth_scale=0.1, t_scale=1000.,
                 near=100., far=10000., device="cuda"):
        import torch
        self.pts = torch.as_tensor(pts).to(device=device, dtype=torch.float32).contiguous()
        if self.pts.device.type != "cuda":
            raise RuntimeError("clean_pvnet_amd.vsd: VsdEvaluator needs a CUDA device; there is no CPU fallback")
        self.faces = torch.as_tensor(faces).to(device=device, dtype=torch.int32).contiguous()
        self.size = _check_size(size)
        if cost not in COSTS:
            raise ValueError("VsdEvaluator: cost must be 'step' or 'tlinear', got %r" % (cost,))
        self.error_thresh = float(error_thresh)
        self.params = dict(delta=float(delta), tau=float(tau), cost=cost, depth_scale=float(depth_scale), t_scale=float(t_scale),
                           near=float(near), far=float(far))
        self._counts = torch.zeros(2, dtype=torch.int64, device=self.pts.device)       # hits, images
        self.last = None

    def evaluate(self, pose_est, pose_gt, depth_test, K, gt_valid=None):
        """``pose_est`` [n,p,3,4] against ``pose_gt`` [n,g,3,4] on the sensor images ``depth_test`` [n,H,W] with the camera
        ``K`` ([3,3] or [n,3,3]); ``gt_valid`` [n,g] masks padded ground-truth slots.  Everything is a CUDA tensor.
        Returns the per-image hits [n] bool.  A pose without a finite value renders nothing and is a miss."""
        import torch
        assert tuple(depth_test.shape[1:]) == (self.size[1], self.size[0]), (depth_test.shape, self.size)
        e = vsd(pose_est, pose_gt, depth_test, K, self.pts, self.faces, gt_valid=gt_valid, **self.params)
        hits = (e < self.error_thresh).flatten(1).any(1)                               # a comparison with NaN is a miss
        n_img = torch.full((), e.shape[0], dtype=torch.int64, device=e.device)
        self._counts += torch.stack([hits.sum(), n_img])
        self.last = {"e": e, "hits": hits}
        return hits

    def summarize(self, n_images=None):
        """``summarize_vsd`` (:258-267): the hit rate since the last call, then the counters start again.  ``n_images``
        overrides the denominator (the T-LESS evaluator divides by ``len(gt_img_ids)``, images without a detection
        included).  The mean of no images is NaN."""
        hits, seen = [int(v) for v in self._counts.cpu().tolist()]
        self._counts.zero_()
        n = seen if n_images is None else int(n_images)
        return {"vsd": hits / n if n else float("nan")}
