"""``lib.csrc.dcn_v2._ext`` -- the extension module ``lib/networks/dcn_v2.py:13`` imports, served by ``clean_pvnet_amd.dcn``.

``dcn_v2_forward`` takes the argument order of dcn_v2.py:25-31, so the reference's own ``DCNv2`` / ``DCN`` run on it unchanged.
Scope is the forward pass of the modulated deformable convolution (inference; the detector is frozen when ``ct_pvnet`` runs):
the backward pass and deformable PSROI pooling are not provided and say so when called.
"""
from lib import _register_clean_pvnet_amd

_register_clean_pvnet_amd()
from clean_pvnet_amd import dcn as _dcn  # noqa: E402

_SCOPE = ("lib.csrc.dcn_v2._ext.%s: not implemented -- this port covers the forward pass of the modulated deformable "
          "convolution only (inference); the backward pass and deformable PSROI pooling are out of its scope")


def dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                   deformable_group):
    if tuple(weight.shape[2:]) != (kernel_h, kernel_w):
        raise RuntimeError("lib.csrc.dcn_v2._ext.dcn_v2_forward: weight is %s, the kernel %d x %d"
                           % (tuple(weight.shape), kernel_h, kernel_w))
    return _dcn.dcn_v2_conv(input, offset, mask, weight, bias, (stride_h, stride_w), (pad_h, pad_w), (dilation_h, dilation_w),
                            deformable_group)


def dcn_v2_backward(*args, **kwargs):
    raise NotImplementedError(_SCOPE % "dcn_v2_backward")


def dcn_v2_psroi_pooling_forward(*args, **kwargs):
    raise NotImplementedError(_SCOPE % "dcn_v2_psroi_pooling_forward")


def dcn_v2_psroi_pooling_backward(*args, **kwargs):
    raise NotImplementedError(_SCOPE % "dcn_v2_psroi_pooling_backward")
