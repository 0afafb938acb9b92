"""DCNv2 modulated deformable convolution, forward, on the device (``libpvnet_vote.so``, the last section of
include/pvnet_vote.h).

Every ``DeformConv`` of the reference's detector (lib/networks/ct/dla_dcn.py:346-358) is a ``DCN`` of lib/networks/dcn_v2.py,
whose extension is CUDA against THC and does not build with a current torch.  ``dcn_v2_conv`` here has that module's signature
(dcn_v2.py:54, 88-94) and ``DCNv2`` / ``DCN`` its parameter names, so a reference checkpoint's state dict loads unchanged;
``lib/csrc/dcn_v2/_ext.py`` is the extension's surface for the reference's own module.  One fused launch per call: the columns
are sampled into LDS and never written out.  The result equals the numpy twin (tests/dcn_twin.py) bit for bit (-0 == +0);
parity with the reference's compiled kernels is unpinned.  Forward only: inference, as ``ct_pvnet`` runs
the detector (lib/networks/ct_pvnet/res.py:71).  CUDA float32 tensors, the current stream, nothing read back, no CPU fallback.
"""
import math

import torch
from torch import nn

from . import _native

_lib = _native.bind("dcn", "libpvnet_vote.so", last_error="pvv_last_error")

MAX_COLUMNS = 1 << 28              # elements ``columns`` agrees to write


def _pair(v):
    if isinstance(v, (tuple, list)):
        a, b = v
        return int(a), int(b)
    return int(v), int(v)


def _out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


def _check(named, forward_only=True):
    _native.check_tensors(named, (torch.float32,), "dcn")
    if forward_only and torch.is_grad_enabled() and any(t.requires_grad for _, t in named):
        raise RuntimeError("clean_pvnet_amd.dcn: forward only -- there is no backward pass; call under torch.no_grad() "
                           "or with tensors that do not require grad")


def _problem(input, offset, mask, kernel, stride, padding, dilation, dg):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, _pair(stride), _pair(padding), _pair(dilation)
    dg = int(dg)
    if input.dim() != 4:
        raise RuntimeError("clean_pvnet_amd.dcn: input must be [B, C, H, W], got %s" % (tuple(input.shape),))
    B, C, H, W = input.shape
    Ho, Wo = _out_size(H, kh, sh, ph, dh), _out_size(W, kw, sw, pw, dw)
    if offset.shape[0] != B or mask.shape[0] != B:
        raise RuntimeError("clean_pvnet_amd.dcn: input, offset and mask differ in batch size")
    off, off_stride = _native.per_image(offset, "offset", 2 * dg * kh * kw, Ho, Wo, module="dcn")
    msk, msk_stride = _native.per_image(mask, "mask", dg * kh * kw, Ho, Wo, module="dcn")
    return (B, C, H, W, Ho, Wo), off, off_stride, msk, msk_stride, (kh, kw, sh, sw, ph, pw, dh, dw, dg)


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """The reference's ``dcn_v2_conv`` (dcn_v2.py:54), forward.
    :param input:   [B,C,H,W] float32 CUDA tensor
    :param offset:  [B, 2*dg*kh*kw, Ho, Wo]; per (group, tap) the row offset, then the column offset
    :param mask:    [B, dg*kh*kw, Ho, Wo]
    :param weight:  [M,C,kh,kw]
    :param bias:    [M] or None
    :return:        [B,M,Ho,Wo] float32
    ``offset`` and ``mask`` may be views (channel slices of one tensor): they are read by their strides.  The contract is in
    include/pvnet_vote.h: the reference's column element, then per output one float32 ``fmaf`` chain over k from the bias."""
    named = [("input", input), ("offset", offset), ("mask", mask), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    _check(named)
    if weight.dim() != 4 or weight.shape[1] != input.shape[1]:
        raise RuntimeError("clean_pvnet_amd.dcn: weight must be [M, C = %d, kh, kw], got %s" % (input.shape[1], tuple(weight.shape)))
    M, kernel = weight.shape[0], (int(weight.shape[2]), int(weight.shape[3]))
    if bias is not None and tuple(bias.shape) != (M,):
        raise RuntimeError("clean_pvnet_amd.dcn: bias must be [%d], got %s" % (M, tuple(bias.shape)))
    (B, C, H, W, Ho, Wo), off, off_stride, msk, msk_stride, geo = _problem(input, offset, mask, kernel, stride, padding, dilation,
                                                                          deformable_groups)
    x, wt = input.detach().contiguous(), weight.detach().contiguous()
    bs = None if bias is None else bias.detach().contiguous()
    out = torch.empty(B, M, max(Ho, 0), max(Wo, 0), dtype=torch.float32, device=x.device)
    if B == 0 or M == 0:
        return out
    _lib.call("pvv_dcn_forward", x.device, x.data_ptr(), wt.data_ptr(), _native.ptr(bs), off.data_ptr(), off_stride,
              msk.data_ptr(), msk_stride, B, C, H, W, M, *geo, out.data_ptr())
    return out


def columns(input, offset, mask, kernel_size, stride, padding, dilation, deformable_groups):
    """The column tensor [B, C*kh*kw, Ho*Wo] the convolution sums over (``pvv_dcn_columns``): the same device function as
    ``dcn_v2_conv`` samples with, written out so that a test can tell sampling from accumulation."""
    _check([("input", input), ("offset", offset), ("mask", mask)], forward_only=False)
    kernel = _pair(kernel_size)
    (B, C, H, W, Ho, Wo), off, off_stride, msk, msk_stride, geo = _problem(input, offset, mask, kernel, stride, padding, dilation,
                                                                          deformable_groups)
    K, P = C * kernel[0] * kernel[1], max(Ho, 0) * max(Wo, 0)
    if B * K * P > MAX_COLUMNS:
        raise ValueError("clean_pvnet_amd.dcn: columns of %d elements; at most 2^28 are written" % (B * K * P))
    x = input.detach().contiguous()
    col = torch.empty(B, K, P, dtype=torch.float32, device=x.device)
    if col.numel() == 0:
        return col
    _lib.call("pvv_dcn_columns", x.device, x.data_ptr(), off.data_ptr(), off_stride, msk.data_ptr(), msk_stride,
              B, C, H, W, *geo, col.data_ptr())
    return col


class DCNv2(nn.Module):
    """The reference's ``DCNv2`` (dcn_v2.py:57-94): ``weight`` [M,C,kh,kw] and ``bias`` [M]; offsets and mask come from the caller."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
            self.bias.zero_()

    def forward(self, input, offset, mask):
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert offset.shape[1] == 2 * taps and mask.shape[1] == taps, (offset.shape, mask.shape)
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)


class DCN(DCNv2):
    """The reference's ``DCN`` (dcn_v2.py:97-128): ``conv_offset_mask`` makes offsets and mask from the input itself.  Its first
    two thirds of channels are the offsets as they lie (what the reference's ``chunk`` and ``cat`` put together again) and are
    passed as a view; the last third goes through the sigmoid."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        self.conv_offset_mask = nn.Conv2d(self.in_channels, 3 * taps, kernel_size=self.kernel_size, stride=self.stride,
                                          padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        with torch.no_grad():
            self.conv_offset_mask.weight.zero_()
            self.conv_offset_mask.bias.zero_()

    def forward(self, input):
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        out = self.conv_offset_mask(input)
        return dcn_v2_conv(input, out[:, :2 * taps], torch.sigmoid(out[:, 2 * taps:]), self.weight, self.bias, self.stride,
                           self.padding, self.dilation, self.deformable_groups)
