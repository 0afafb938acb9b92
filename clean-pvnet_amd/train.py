"""PVNet's vote targets and training loss on the device (``libpvnet_vote.so``, the last section of include/pvnet_vote.h).

The reference builds the target field on a CPU core per sample (``compute_vertex``, lib/utils/pvnet/pvnet_data_utils.py:30-44,
called at lib/datasets/*/pvnet.py:53: 22 MB per 480x640 image at K = 9, then copied to the device) and computes the loss in
torch ops with autograd (``NetworkWrapper.forward``, lib/train/trainers/pvnet.py:25-34).  Here ``compute_vertex`` is one
launch for a batch, and ``pvnet_loss`` is fused: the forward pass reads the network output once, the backward pass reads it
once and writes the gradient once, and with ``kpt_2d`` the target field never exists -- it is recomputed per pixel from the
mask and the keypoints.  The target equals the reference's bit for bit, the vote loss's gradient equals torch's CPU autograd
bit for bit, every sum is binary64 in a fixed order (tests/train_twin.py is the contract in numpy, tests/golden/train_*.npz
the reference's own results).  CUDA float32 tensors, the current stream, nothing read back, no CPU fallback.
"""
import torch
from torch import nn

from . import _native
from ._loss import FusedLoss

MAX_K, MAX_C = 64, 16                # PVV_TRAIN_MAX_K, PVV_TRAIN_MAX_C
MASK_KINDS = {torch.uint8: 0, torch.bool: 0, torch.int32: 1, torch.int64: 2}     # PVV_MASK_U8, PVV_MASK_I32, PVV_MASK_I64

_lib = _native.bind("train", "libpvnet_vote.so", last_error="pvv_last_error")

_F32 = (torch.float32,)
_DTYPES = {"vertex_pred": _F32, "seg_pred": _F32, "vertex": _F32, "mask": tuple(MASK_KINDS), "kpt_2d": (torch.float32, torch.float64)}


def _check(named, mask, kpt_2d):
    """Device, then dtype, of every tensor; shapes come after."""
    named = named + [("mask", mask)] + ([("kpt_2d", kpt_2d)] if kpt_2d is not None else [])
    _native.check_tensors(named, _DTYPES, "train", {"mask": "uint8, bool, int32 or int64"})


def _mask_kpt_shapes(mask, kpt_2d):
    if mask.dim() != 3:
        raise ValueError("clean_pvnet_amd.train: mask must be [B, H, W], got %s" % (tuple(mask.shape),))
    B, H, W = mask.shape
    if kpt_2d is not None and (kpt_2d.dim() != 3 or kpt_2d.shape[0] != B or kpt_2d.shape[2] != 2):
        raise ValueError("clean_pvnet_amd.train: kpt_2d must be [B = %d, K, 2], got %s" % (B, tuple(kpt_2d.shape)))
    return B, H, W


def compute_vertex(mask, kpt_2d):
    """The reference's ``compute_vertex`` (pvnet_data_utils.py:30-44) for a batch, as its loader stores it (``transpose(2, 0, 1)``).
    :param mask:    [B,H,W] uint8, bool, int32 or int64 CUDA tensor; the pixels with ``mask == 1`` get a target
    :param kpt_2d:  [B,K,2] float32 or float64, (x, y)
    :return:        [B,2K,H,W] float32: channel 2k the x and 2k+1 the y component of the unit vector to keypoint k, +0 elsewhere
    ``mask`` [H,W] with ``kpt_2d`` [K,2] gives [2K,H,W]."""
    _check([], mask, kpt_2d)
    single = mask.dim() == 2 and kpt_2d.dim() == 2
    m, kp = (mask[None], kpt_2d[None]) if single else (mask, kpt_2d)
    B, H, W = _mask_kpt_shapes(m, kp)
    K = kp.shape[1]
    m, kp = m.contiguous(), kp.detach().contiguous()
    out = torch.empty(B, 2 * K, H, W, dtype=torch.float32, device=m.device)
    if out.numel() == 0:
        return out[0] if single else out
    _lib.call("pvv_vertex_target", m.device, m.data_ptr(), MASK_KINDS[m.dtype], kp.data_ptr(), int(kp.dtype == torch.float64), B, K, H, W,
              out.data_ptr())
    return out[0] if single else out


def _problem(vertex_pred, seg_pred, mask, kpt_2d, vertex):
    """The checked arguments of both entry points: (tensors kept alive, the leading ctypes arguments, sizes)."""
    if (kpt_2d is None) == (vertex is None):
        raise ValueError("clean_pvnet_amd.train: exactly one of kpt_2d and vertex must be given")
    named = [("vertex_pred", vertex_pred), ("seg_pred", seg_pred)] + ([("vertex", vertex)] if vertex is not None else [])
    _check(named, mask, kpt_2d)
    for what, t in [("vertex", vertex), ("kpt_2d", kpt_2d)]:
        if t is not None and t.requires_grad:
            raise RuntimeError("clean_pvnet_amd.train: %s requires grad; gradients go to vertex_pred and seg_pred only" % what)
    B, H, W = _mask_kpt_shapes(mask, kpt_2d)
    if vertex_pred.dim() != 4 or vertex_pred.shape[0] != B or tuple(vertex_pred.shape[2:]) != (H, W) or vertex_pred.shape[1] % 2:
        raise ValueError("clean_pvnet_amd.train: vertex_pred must be [B = %d, 2K, %d, %d], got %s" % (B, H, W, tuple(vertex_pred.shape)))
    K = vertex_pred.shape[1] // 2
    if seg_pred.dim() != 4 or seg_pred.shape[0] != B or tuple(seg_pred.shape[2:]) != (H, W):
        raise ValueError("clean_pvnet_amd.train: seg_pred must be [B = %d, C, %d, %d], got %s" % (B, H, W, tuple(seg_pred.shape)))
    C = seg_pred.shape[1]
    if kpt_2d is not None and kpt_2d.shape[1] != K:
        raise ValueError("clean_pvnet_amd.train: kpt_2d has %d keypoints, vertex_pred %d" % (kpt_2d.shape[1], K))
    if vertex is not None and tuple(vertex.shape) != (B, 2 * K, H, W):
        raise ValueError("clean_pvnet_amd.train: vertex must be [%d, %d, %d, %d], got %s" % (B, 2 * K, H, W, tuple(vertex.shape)))
    if not 1 <= K <= MAX_K or not 1 <= C <= MAX_C:
        raise ValueError("clean_pvnet_amd.train: K must lie in [1, %d] and C in [1, %d], got K = %d, C = %d" % (MAX_K, MAX_C, K, C))
    if B == 0 or H * W == 0:
        raise ValueError("clean_pvnet_amd.train: an empty batch has no loss")
    vp, vp_stride = _native.per_image(vertex_pred.detach(), "vertex_pred", 2 * K, H, W)
    sp, sp_stride = _native.per_image(seg_pred.detach(), "seg_pred", C, H, W)
    tg, tg_stride = (None, 0) if vertex is None else _native.per_image(vertex, "vertex", 2 * K, H, W)
    m = mask.contiguous()
    kp = None if kpt_2d is None else kpt_2d.contiguous()
    args = (vp.data_ptr(), vp_stride, sp.data_ptr(), sp_stride, m.data_ptr(), MASK_KINDS[m.dtype], _native.ptr(kp),
            int(kp is not None and kp.dtype == torch.float64), _native.ptr(tg), tg_stride, B, K, C, H, W)
    return (vp, sp, m, kp, tg), args, (B, K, C, H, W)


class _PVNetLoss(FusedLoss):
    lib, workspace_query, state_len = _lib, "pvv_pvnet_loss_workspace_bytes", 2
    forward_symbol, backward_symbol = "pvv_pvnet_loss_forward", "pvv_pvnet_loss_backward"

    problem = staticmethod(lambda *inputs: _problem(*inputs))
    workspace_sizes = staticmethod(lambda B, K, C, H, W: (B, H, W))
    grad_shapes = staticmethod(lambda B, K, C, H, W: ((B, 2 * K, H, W), (B, C, H, W)))


def pvnet_loss(vertex_pred, seg_pred, mask, *, kpt_2d=None, vertex=None):
    """The two losses of the reference's ``NetworkWrapper.forward`` (lib/train/trainers/pvnet.py:25-34), fused.
    :param vertex_pred: [B,2K,H,W] float32 CUDA tensor, ``output['vertex']``; a channel slice of a larger tensor is read in place
    :param seg_pred:    [B,C,H,W] float32, ``output['seg']``; likewise
    :param mask:        [B,H,W] uint8, bool, int32 or int64: the vote weight and the segmentation label
    :param kpt_2d:      [B,K,2] float32 or float64 -- the target is recomputed per pixel, no field exists -- or
    :param vertex:      [B,2K,H,W] float32, ``batch['vertex']``; exactly one of the two
    :return:            (vote_loss, seg_loss), 0-dim float32 tensors on the device
    Gradients go to ``vertex_pred`` and ``seg_pred`` only, once (no double backward).  A label outside [0, C) makes both
    losses and both gradients NaN instead of faulting; the contract is in include/pvnet_vote.h."""
    return _PVNetLoss.apply(vertex_pred, seg_pred, mask, kpt_2d, vertex)


class PVNetLoss(nn.Module):
    """``pvnet_loss`` as a module: ``forward(vertex_pred, seg_pred, mask, kpt_2d=None, vertex=None) -> (vote_loss, seg_loss)``."""

    def forward(self, vertex_pred, seg_pred, mask, kpt_2d=None, vertex=None):
        return pvnet_loss(vertex_pred, seg_pred, mask, kpt_2d=kpt_2d, vertex=vertex)


class NetworkWrapper(nn.Module):
    """The reference's ``NetworkWrapper`` (lib/train/trainers/pvnet.py:6-39) over the fused loss: the same ``forward(batch)``
    contract and the same keys.  The target is ``batch['vertex']`` when the loader still ships it, otherwise it is
    recomputed from ``batch['kpt_2d']`` [B,K,2]."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.crit = PVNetLoss()

    def forward(self, batch):
        output = self.net(batch['inp'])

        if 'pose_test' in batch['meta'].keys():
            loss = torch.tensor(0).to(batch['inp'].device)
            return output, loss, {}, {}

        if 'vertex' in batch:
            vote_loss, seg_loss = self.crit(output['vertex'], output['seg'], batch['mask'], vertex=batch['vertex'])
        else:
            vote_loss, seg_loss = self.crit(output['vertex'], output['seg'], batch['mask'], kpt_2d=batch['kpt_2d'])
        loss = vote_loss + seg_loss
        scalar_stats = {'vote_loss': vote_loss, 'seg_loss': seg_loss, 'loss': loss}
        image_stats = {}

        return output, loss, scalar_stats, image_stats
