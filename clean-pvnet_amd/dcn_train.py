"""DCNv2 modulated deformable convolution with its backward pass on the device (``libpvnet_vote.so``, "Modulated deformable
convolution, backward" of include/pvnet_vote.h): what training the detector through its ``DeformConv`` layers
(lib/networks/ct/dla_dcn.py:346-358) needs.

``dcn_v2_conv`` has the signature of ``clean_pvnet_amd.dcn.dcn_v2_conv`` and is a ``torch.autograd.Function`` underneath: the
forward is that module's fused launch, unchanged, and saves input, offset, mask and weight -- no column tensor; the backward
(``dcn_v2_backward``) samples the columns again on the chip.  Every gradient is the same bits on every run: the two GEMM-shaped
reductions are ``fmaf`` chains in a fixed order, the scatter into ``grad_input`` adds integers, and
the numpy twin (tests/dcn_train_twin.py) gives the same bits.  ``DCNv2`` / ``DCN`` subclass the forward-only modules, so a
reference checkpoint loads unchanged; ``convert`` swaps them into a model.  ``clean_pvnet_amd.dcn`` and
``lib.csrc.dcn_v2._ext`` keep refusing a backward pass: they are the inference surface, and this module is the training one.
CUDA float32 tensors, the current stream, nothing read back, no CPU fallback, no silent cast.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _native, dcn

_lib = _native.bind("dcn_train", "libpvnet_vote.so", last_error="pvv_last_error")

SLAB = 512                         # PVV_DCN_SLAB: pixels of one grad_weight chain


def _named(input, offset, mask, weight, bias):
    return [("input", input), ("offset", offset), ("mask", mask), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])


def _backward(input, offset, mask, weight, grad_output, stride, padding, dilation, deformable_groups, need, chunk_images=None):
    M, kernel = weight.shape[0], (int(weight.shape[2]), int(weight.shape[3]))
    (B, C, H, W, Ho, Wo), off, off_stride, msk, msk_stride, geo = dcn._problem(input, offset, mask, kernel, stride, padding, dilation,
                                                                              deformable_groups)
    if tuple(grad_output.shape) != (B, M, Ho, Wo):
        raise RuntimeError("clean_pvnet_amd.dcn_train: grad_output must be [%d, %d, %d, %d], got %s"
                           % (B, M, Ho, Wo, tuple(grad_output.shape)))
    x, wt, go = input.detach().contiguous(), weight.detach().contiguous(), grad_output.detach().contiguous()
    shapes = (x.shape, (B,) + tuple(offset.shape[1:]), (B,) + tuple(mask.shape[1:]), wt.shape, (M,))
    grads = [torch.empty(tuple(s), dtype=torch.float32, device=x.device) if n else None for n, s in zip(need, shapes)]
    if not any(need):
        return tuple(grads)
    if B == 0 or M == 0 or Ho <= 0 or Wo <= 0:
        return tuple(None if g is None else g.zero_() for g in grads)
    ws, nbytes = _lib.workspace("pvv_dcn_backward_workspace_bytes", x.device, B, C, H, W, M, *geo,
                                0 if chunk_images is None else int(chunk_images), refused=lambda n: n < 0, error=RuntimeError)
    _lib.call("pvv_dcn_backward", x.device, x.data_ptr(), wt.data_ptr(), off.data_ptr(), off_stride, msk.data_ptr(),
              msk_stride, go.data_ptr(), B, C, H, W, M, *geo, *(_native.ptr(g) for g in grads), ws.data_ptr(), nbytes)
    return tuple(grads)


def dcn_v2_backward(input, offset, mask, weight, bias, grad_output, stride, padding, dilation, deformable_groups,
                    need=(True,) * 5, _chunk_images=None):
    """The five gradients of ``dcn_v2_conv`` for the upstream gradient ``grad_output`` [B,M,Ho,Wo]:
    ``(grad_input, grad_offset, grad_mask, grad_weight, grad_bias)``, ``None`` where ``need`` is false (and for a ``bias`` of
    ``None``); the launches nobody needs are skipped.  ``offset`` and ``mask`` may be views, as in the forward; ``grad_output``
    is made contiguous if it is not.  ``_chunk_images`` is for tests: images per chunk of the workspace (default: what fits
    256 MiB) -- the result does not depend on it."""
    dcn._check(_named(input, offset, mask, weight, bias) + [("grad_output", grad_output)], forward_only=False)
    if weight.dim() != 4 or input.dim() != 4 or weight.shape[1] != input.shape[1]:
        raise RuntimeError("clean_pvnet_amd.dcn_train: weight must be [M, C, kh, kw] and input [B, C, H, W], got %s and %s"
                           % (tuple(weight.shape), tuple(input.shape)))
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise RuntimeError("clean_pvnet_amd.dcn_train: bias must be [%d], got %s" % (weight.shape[0], tuple(bias.shape)))
    need = tuple(bool(n) for n in need)
    if len(need) != 5:
        raise ValueError("clean_pvnet_amd.dcn_train: need has five entries")
    return _backward(input, offset, mask, weight, grad_output, stride, padding, dilation, deformable_groups,
                     need[:4] + (need[4] and bias is not None,), _chunk_images)


class _DCNv2Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
        ctx.geometry = (stride, padding, dilation, deformable_groups)
        ctx.save_for_backward(input, offset, mask, weight)                 # (no column tensor: the backward samples again)
        return dcn.dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        dcn._check([("grad_output", grad_output)], forward_only=False)
        grads = _backward(*ctx.saved_tensors, grad_output, *ctx.geometry, need=tuple(ctx.needs_input_grad[:5]))
        return grads + (None,) * 4


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """``clean_pvnet_amd.dcn.dcn_v2_conv`` -- same arguments, same bytes -- that autograd can go through."""
    dcn._check(_named(input, offset, mask, weight, bias), forward_only=False)
    return _DCNv2Function.apply(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)


class DCNv2(dcn.DCNv2):
    """``clean_pvnet_amd.dcn.DCNv2`` with a backward pass: the same parameters under the same names."""

    def forward(self, input, offset, mask):
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        assert offset.shape[1] == 2 * taps and mask.shape[1] == taps, (offset.shape, mask.shape)
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)


class DCN(dcn.DCN):
    """``clean_pvnet_amd.dcn.DCN`` with a backward pass: offsets and mask are passed as views, and their gradients flow back
    into ``conv_offset_mask`` through torch's own slicing and sigmoid."""

    def forward(self, input):
        taps = self.deformable_groups * self.kernel_size[0] * self.kernel_size[1]
        out = self.conv_offset_mask(input)
        return dcn_v2_conv(input, out[:, :2 * taps], torch.sigmoid(out[:, 2 * taps:]), self.weight, self.bias, self.stride,
                           self.padding, self.dilation, self.deformable_groups)


def _counterparts():
    """(class to replace, its trainable counterpart), the more derived first."""
    pairs = [(dcn.DCN, DCN), (dcn.DCNv2, DCNv2)]
    try:
        from lib.networks import dcn_v2 as reference            # the reference's own module, where a checkout provides it
        pairs += [(reference.DCN, DCN), (reference.DCNv2, DCNv2)]
    except Exception:                                           # not importable: nothing of it can be inside a model
        pass
    return pairs


def _trainable(module, pairs):
    if isinstance(module, (DCN, DCNv2)):
        return module
    for old, new in pairs:
        if isinstance(module, old):
            twin = new.__new__(new)
            twin.__dict__.update(module.__dict__)               # the same parameter, buffer and submodule tables: shared, not copied
            return twin
    return module


def convert(module):
    """``module`` with every ``dcn.DCN`` / ``dcn.DCNv2`` inside it (and the reference's ``lib/networks/dcn_v2`` classes when
    importable) replaced by its trainable counterpart, which shares the parameters.  Returns the model: ``module`` itself, or
    its counterpart when ``module`` is such a layer."""
    pairs = _counterparts()
    for parent in module.modules():
        for name, child in list(parent._modules.items()):
            if child is not None:
                parent._modules[name] = _trainable(child, pairs)
    return _trainable(module, pairs)
