"""``lib.csrc.fps.fps_utils`` -- the module ``tools/handle_custom_dataset.py:4`` imports to pick the ``fps_3d`` keypoints of a
custom object.  The reference's signature and return value (lib/csrc/fps/fps_utils.py): numpy in, the sampled points
``pts[idxs]`` as float32 out; the sampling itself runs on the device (``clean_pvnet_amd.model``) and gives the indices of the
reference's ``farthest_point_sampling.cpp``.  With ``init_center=False`` the first sample is random, as in the reference."""
import numpy as np

from lib import _register_clean_pvnet_amd

_register_clean_pvnet_amd()
from clean_pvnet_amd import model as _model  # noqa: E402


def farthest_point_sampling(pts, sn, init_center=False):
    import torch
    pn, _ = pts.shape
    assert(pts.shape[1] == 3)
    if not torch.cuda.is_available():
        raise RuntimeError("lib.csrc.fps.fps_utils: farthest_point_sampling runs on the GPU; there is no CPU fallback")
    pts = np.ascontiguousarray(pts, np.float32)
    idxs = _model.farthest_point_sampling(torch.from_numpy(pts).cuda(), sn, bool(init_center)).cpu().numpy()
    return pts[idxs]
