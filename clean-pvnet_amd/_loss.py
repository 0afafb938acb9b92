"""The autograd function the two fused losses share (``train.pvnet_loss``, ``ct_train.ct_loss``): two losses out of one forward
launch, two gradients out of one backward launch that recomputes what it needs from the inputs and a small state tensor.
"""
import torch
from torch.autograd.function import once_differentiable


class FusedLoss(torch.autograd.Function):
    """A subclass supplies
        ``lib``                    its module's ``_native.Library``
        ``problem(*inputs)``       the checked arguments of both entry points: (tensors kept alive, the leading ctypes arguments, sizes)
        ``workspace_query``, ``forward_symbol``, ``backward_symbol``
        ``workspace_sizes(*sizes)``  the arguments of the workspace query
        ``state_len``              int64 words of the state the forward pass leaves for the backward pass
        ``grad_shapes(*sizes)``    the shapes of the two gradients: float32, for the first two inputs
    and gets ``apply(*inputs) -> (loss_0, loss_1)``, 0-dim float32 tensors on the device of the first input."""

    @classmethod
    def forward(cls, ctx, *inputs):
        keep, args, sizes = cls.problem(*inputs)
        dev = inputs[0].device
        ws, nbytes = cls.lib.workspace(cls.workspace_query, dev, *cls.workspace_sizes(*sizes))
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        state = torch.empty(cls.state_len, dtype=torch.int64, device=dev)
        cls.lib.call(cls.forward_symbol, dev, *args, ws.data_ptr(), nbytes, losses.data_ptr(), state.data_ptr())
        ctx.keep, ctx.args, ctx.sizes, ctx.state, ctx.others = keep, args, sizes, state, len(inputs) - 2
        return losses[0], losses[1]

    @classmethod
    @once_differentiable
    def backward(cls, ctx, go_0, go_1):
        dev = ctx.state.device
        zero = None
        if go_0 is None or go_1 is None:                           # an unused loss: its upstream gradient counts as zero
            zero = torch.zeros((), dtype=torch.float32, device=dev)
        go = torch.stack([zero if go_0 is None else go_0.to(torch.float32), zero if go_1 is None else go_1.to(torch.float32)])
        grad_0, grad_1 = (torch.empty(shape, dtype=torch.float32, device=dev) for shape in cls.grad_shapes(*ctx.sizes))
        cls.lib.call(cls.backward_symbol, dev, *ctx.args, ctx.state.data_ptr(), go.data_ptr(), grad_0.data_ptr(), grad_1.data_ptr())
        return (grad_0, grad_1) + (None,) * ctx.others
