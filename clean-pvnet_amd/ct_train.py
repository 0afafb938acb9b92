"""The detector's heat-map targets and training loss on the device (``libpvnet_vote.so``, the section "Detector training" of
include/pvnet_vote.h).

The reference builds the targets per sample on a CPU core (``prepare_detection``, lib/datasets/tless_train/ct.py:46-66, with
``gaussian_radius`` and ``draw_umich_gaussian`` of lib/utils/data_utils.py:10-65; ``ct_collator``, lib/datasets/collate_batch.py:6-32,
pads them) and computes the loss in about twenty map-sized torch ops with autograd (``NetworkWrapper.forward``,
lib/train/trainers/ct.py:14-31, over lib/utils/net_utils.py:9-49, 195-246).  Here ``ct_targets`` is two launches for a batch, and
``ct_loss`` is fused: the forward pass reads logits and targets once, the backward pass reads them once and writes the gradient
once.  Radii, indices and boxes equal the reference's bit for bit, the wh gradient equals torch's CPU autograd bit for bit, every
sum is binary64 in a fixed order (tests/ct_train_twin.py is the contract in numpy, tests/golden/ct_train_*.npz the reference's own
results).  CUDA float32 tensors, the current stream, nothing read back, no CPU fallback.
"""
import torch
from torch import nn

from . import _native
from ._loss import FusedLoss

MAX_N = 512                          # PVV_CT_TRAIN_MAX_N
BOX_KINDS = {torch.float32: 0, torch.int32: 1, torch.int64: 2}        # PVV_BOX_F32, PVV_BOX_I32, PVV_BOX_I64
_INTS = (torch.int32, torch.int64)

_lib = _native.bind("ct_train", "libpvnet_vote.so", last_error="pvv_last_error")


def ct_targets(boxes, cls, num, num_classes, height, width):
    """The reference's ``prepare_detection`` (lib/datasets/tless_train/ct.py:46-66) for every object of a batch and its
    ``ct_collator`` (lib/datasets/collate_batch.py:6-32), in one call.
    :param boxes:       [B,N,4] float32, int32 or int64 CUDA tensor: (x_min, y_min, x_max, y_max) on the output map
    :param cls:         [B,N] int64 or int32: the class of each box
    :param num:         [B] int64 or int32: the first ``num[b]`` rows of image b are objects
    :param num_classes: C; ``height``, ``width``: H, W of the output map
    :return:            ``ct_hm`` [B,C,H,W] float32, ``wh`` [B,N,2] float32, ``ct_cls`` [B,N] int64, ``ct_ind`` [B,N] int64,
                        ``ct_01`` [B,N] float32, ``ct_num`` [B] int64
    A box with ``x_max <= x_min`` or ``y_max <= y_min``, a class outside [0, C) or a centre outside the map draws nothing and is
    dropped; the survivors are packed to the front in their order and everything after ``ct_num[b]`` is zero.  The collator pads
    to the batch's largest ``ct_num``; that number lives on the device, so the width here is N.  Both losses are unchanged by
    the zero-weight padding: a padded row has ``ct_01 == 0``, so it adds +0 to the wh sum and to its divisor, and the heat map
    does not know the rows."""
    _native.check_tensors([("boxes", boxes), ("cls", cls), ("num", num)], {"boxes": tuple(BOX_KINDS), "cls": _INTS, "num": _INTS}, "ct_train")
    if boxes.dim() != 3 or boxes.shape[2] != 4:
        raise ValueError("clean_pvnet_amd.ct_train: boxes must be [B, N, 4], got %s" % (tuple(boxes.shape),))
    B, N = boxes.shape[:2]
    if tuple(cls.shape) != (B, N):
        raise ValueError("clean_pvnet_amd.ct_train: cls must be [B = %d, N = %d], got %s" % (B, N, tuple(cls.shape)))
    if tuple(num.shape) != (B,):
        raise ValueError("clean_pvnet_amd.ct_train: num must be [B = %d], got %s" % (B, tuple(num.shape)))
    C, H, W = int(num_classes), int(height), int(width)
    if B < 1 or not 1 <= N <= MAX_N or C < 1 or H < 1 or W < 1:
        raise ValueError("clean_pvnet_amd.ct_train: B, C, H, W must be positive and N in [1, %d], got B = %d, N = %d, C = %d, H = %d, W = %d"
                         % (MAX_N, B, N, C, H, W))
    bx, cl, nm = boxes.detach().contiguous(), cls.contiguous(), num.contiguous()
    dev = bx.device
    ct_hm = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
    wh = torch.empty(B, N, 2, dtype=torch.float32, device=dev)
    ct_cls = torch.empty(B, N, dtype=torch.int64, device=dev)
    ct_ind = torch.empty(B, N, dtype=torch.int64, device=dev)
    ct_01 = torch.empty(B, N, dtype=torch.float32, device=dev)
    ct_num = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("pvv_ct_targets", dev, bx.data_ptr(), BOX_KINDS[bx.dtype], cl.data_ptr(), int(cl.dtype == torch.int64), nm.data_ptr(),
              int(nm.dtype == torch.int64), B, N, C, H, W, ct_hm.data_ptr(), wh.data_ptr(), ct_cls.data_ptr(), ct_ind.data_ptr(),
              ct_01.data_ptr(), ct_num.data_ptr())
    return ct_hm, wh, ct_cls, ct_ind, ct_01, ct_num


def _problem(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01):
    """The checked arguments of both entry points: (tensors kept alive, the leading ctypes arguments, sizes)."""
    named = [("ct_hm_pred", ct_hm_pred), ("wh_pred", wh_pred), ("ct_hm", ct_hm), ("wh", wh), ("ct_ind", ct_ind), ("ct_01", ct_01)]
    f32 = (torch.float32,)
    _native.check_tensors(named, {"ct_hm_pred": f32, "wh_pred": f32, "ct_hm": f32, "wh": f32, "ct_ind": _INTS, "ct_01": f32}, "ct_train")
    for what, t in named[2:]:
        if t.requires_grad:
            raise RuntimeError("clean_pvnet_amd.ct_train: %s requires grad; gradients go to ct_hm_pred and wh_pred only" % what)
    if ct_hm_pred.dim() != 4:
        raise ValueError("clean_pvnet_amd.ct_train: ct_hm_pred must be [B, C, H, W], got %s" % (tuple(ct_hm_pred.shape),))
    B, C, H, W = ct_hm_pred.shape
    if tuple(wh_pred.shape) != (B, 2, H, W):
        raise ValueError("clean_pvnet_amd.ct_train: wh_pred must be [%d, 2, %d, %d], got %s" % (B, H, W, tuple(wh_pred.shape)))
    if tuple(ct_hm.shape) != (B, C, H, W):
        raise ValueError("clean_pvnet_amd.ct_train: ct_hm must be [%d, %d, %d, %d], got %s" % (B, C, H, W, tuple(ct_hm.shape)))
    if wh.dim() != 3 or wh.shape[0] != B or wh.shape[2] != 2:
        raise ValueError("clean_pvnet_amd.ct_train: wh must be [B = %d, N, 2], got %s" % (B, tuple(wh.shape)))
    N = wh.shape[1]
    for what, t in (("ct_ind", ct_ind), ("ct_01", ct_01)):
        if tuple(t.shape) != (B, N):
            raise ValueError("clean_pvnet_amd.ct_train: %s must be [B = %d, N = %d], got %s" % (what, B, N, tuple(t.shape)))
    if not 1 <= N <= MAX_N:
        raise ValueError("clean_pvnet_amd.ct_train: N must lie in [1, %d], got %d" % (MAX_N, N))
    if B == 0 or C * H * W == 0:
        raise ValueError("clean_pvnet_amd.ct_train: an empty batch has no loss")
    hp, hp_stride = _native.per_image(ct_hm_pred.detach(), "ct_hm_pred", C, H, W)
    wp, wp_stride = _native.per_image(wh_pred.detach(), "wh_pred", 2, H, W)
    hm, hm_stride = _native.per_image(ct_hm, "ct_hm", C, H, W)
    tg, ind, w01 = wh.contiguous(), ct_ind.contiguous(), ct_01.contiguous()
    args = (hp.data_ptr(), hp_stride, wp.data_ptr(), wp_stride, hm.data_ptr(), hm_stride, tg.data_ptr(), ind.data_ptr(),
            int(ind.dtype == torch.int64), w01.data_ptr(), B, N, C, H, W)
    return (hp, wp, hm, tg, ind, w01), args, (B, N, C, H, W)


class _CtLoss(FusedLoss):
    lib, workspace_query, state_len = _lib, "pvv_ct_loss_workspace_bytes", 4
    forward_symbol, backward_symbol = "pvv_ct_loss_forward", "pvv_ct_loss_backward"
    problem = staticmethod(lambda *inputs: _problem(*inputs))
    workspace_sizes = staticmethod(lambda B, N, C, H, W: (B, C, H, W))
    grad_shapes = staticmethod(lambda B, N, C, H, W: ((B, C, H, W), (B, 2, H, W)))


def ct_loss(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01):
    """The two losses of the reference's ``NetworkWrapper.forward`` (lib/train/trainers/ct.py:20-26), fused.
    :param ct_hm_pred:  [B,C,H,W] float32 CUDA tensor, ``output['ct_hm']``: the logits -- the sigmoid and its clamp
                        (lib/utils/net_utils.py:9-11) are inside; a channel slice of a larger tensor is read in place
    :param wh_pred:     [B,2,H,W] float32, ``output['wh']``; likewise
    :param ct_hm:       [B,C,H,W] float32, ``batch['ct_hm']``: exactly 1 marks a positive
    :param wh:          [B,N,2] float32, ``ct_ind`` [B,N] int64 or int32, ``ct_01`` [B,N] float32: ``batch['wh']``, ``['ct_ind']``, ``['ct_01']``
    :return:            (ct_loss, wh_loss), 0-dim float32 tensors on the device
    Gradients go to ``ct_hm_pred`` and ``wh_pred`` only, once (no double backward).  A ``ct_ind`` outside [0, H*W) at a position
    of weight != 0 makes the wh loss and its gradient NaN instead of faulting; the contract is in include/pvnet_vote.h."""
    return _CtLoss.apply(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01)


class CtLoss(nn.Module):
    """``ct_loss`` as a module: ``forward(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01) -> (ct_loss, wh_loss)``."""

    def forward(self, ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01):
        return ct_loss(ct_hm_pred, wh_pred, ct_hm, wh, ct_ind, ct_01)


class NetworkWrapper(nn.Module):
    """The reference's ``NetworkWrapper`` (lib/train/trainers/ct.py:5-31) over the fused loss: the same ``forward(batch)``
    contract and the same keys.  The targets are ``batch['ct_hm']``, ``['wh']``, ``['ct_ind']``, ``['ct_01']`` when the loader
    ships them; otherwise they are made from ``batch['boxes']`` [B,N,4], ``batch['cls']`` [B,N] and ``batch['num']`` [B]."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.crit = CtLoss()

    def forward(self, batch):
        output = self.net(batch['inp'])

        if 'ct_hm' in batch:
            ct_hm, wh, ct_ind, ct_01 = batch['ct_hm'], batch['wh'], batch['ct_ind'], batch['ct_01']
        else:
            C, H, W = output['ct_hm'].shape[1:]
            ct_hm, wh, _, ct_ind, ct_01, _ = ct_targets(batch['boxes'], batch['cls'], batch['num'], C, H, W)
        ct_loss, wh_loss = self.crit(output['ct_hm'], output['wh'], ct_hm, wh, ct_ind, ct_01)
        loss = ct_loss + 0.1 * wh_loss
        scalar_stats = {'ct_loss': ct_loss, 'wh_loss': wh_loss, 'loss': loss}
        image_stats = {}

        return output, loss, scalar_stats, image_stats
