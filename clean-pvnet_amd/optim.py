"""The clipped optimizer step of every parameter in one launch (``libpvnet_vote.so``, the section "Optimizer step" of
include/pvnet_vote.h).

The reference ends every iteration with ``zero_grad()``, ``clip_grad_value_(..., 40)`` and ``optimizer.step()``
(lib/train/trainers/trainer.py:42-45), and its ``make_optimizer`` (lib/train/optimizer.py:12-27) puts every parameter in a param
group of its own, so even torch's ``foreach`` / ``fused`` steps run once per tensor: over a thousand small launches for PVNet's
ResNet-18.  Here ``optim_step`` is one launch for all tensors: a table with one row per tensor (four pointers, ``numel``, the
float32 scalars) and a prefix of chunk starts is built on the host per step, uploaded, and every block of the launch works on one
chunk of ``CHUNK`` elements of one tensor.  ``Adam``, ``RAdam`` and ``SGD`` are ``torch.optim.Optimizer`` subclasses over it with the
state names and ``state_dict`` layout of the classes they replace, ``make_optimizer`` is the reference's factory.

The arithmetic is float32 in the order the header states (tests/optim_twin.py is the contract in numpy and the device equals it
byte for byte); the scalars are computed here in binary64 by the reference's own expressions and rounded to float32 once.  The one
deviation: the clamped gradient is used and not written back to ``p.grad`` (``clip_grad_value_`` writes it; calling it first is
still fine, clamping twice is the identity).  CUDA float32 tensors, the current stream, nothing read back, no CPU fallback.
"""
import math

import numpy as np
import torch

from . import _native

CHUNK = 8192                                     # PVV_OPTIM_CHUNK: elements one block works on
KINDS = {"adam": 0, "radam": 1, "sgd": 2}        # PVV_OPTIM_ADAM, PVV_OPTIM_RADAM, PVV_OPTIM_SGD
CLIP, ZERO_GRAD = 1, 2                           # PVV_OPTIM_CLIP, PVV_OPTIM_ZERO_GRAD
ROW_ADAPTIVE, ROW_DECAY, ROW_NO_UPDATE, ROW_FIRST = 1, 2, 4, 8      # PVV_OPTIM_ROW_*
ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("flags", "<i4"), ("reserved", "<i4"),
                ("s", "<f4", (8,))])             # pvv_optim_row
assert ROW.itemsize == 80

_lib = _native.bind("optim", "libpvnet_vote.so", last_error="pvv_last_error")
if _lib.pvv_optim_chunk() != CHUNK:
    raise ImportError("clean_pvnet_amd.optim: libpvnet_vote.so was built with PVV_OPTIM_CHUNK = %d, this module expects %d; rebuild"
                      % (_lib.pvv_optim_chunk(), CHUNK))


# ---------------------------------------------------------------------------------------------------------------- host side
def radam_rectification(step, beta1, beta2, degenerated_to_sgd=True):
    """``(N_sma, step_size)`` of the reference's RAdam at ``step`` (lib/utils/optimizer/radam.py:68-80), in Python floats."""
    beta2_t = beta2 ** step
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** step)
    elif degenerated_to_sgd:
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        step_size = -1
    return N_sma, step_size


def row_scalars(kind, step, lr, weight_decay, betas, eps, momentum, degenerated_to_sgd=True):
    """``(s, flags)`` of one row: the scalars in binary64, in the header's order (the table rounds them to float32 once), and the
    ``ROW_*`` bits.  ``step`` is the tensor's step count after this step (1 on its first)."""
    if kind == "adam":
        beta1, beta2 = betas
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        return (weight_decay, 1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, eps, -step_size), 0
    if kind == "radam":
        beta1, beta2 = betas
        N_sma, step_size = radam_rectification(step, beta1, beta2, degenerated_to_sgd)
        flags = (ROW_ADAPTIVE if N_sma >= 5 else 0 if step_size > 0 else ROW_NO_UPDATE) | (ROW_DECAY if weight_decay != 0 else 0)
        return (beta1, 1 - beta1, beta2, 1 - beta2, eps, -weight_decay * lr, -step_size * lr), flags
    return (weight_decay, momentum, -lr), (ROW_FIRST if step == 1 else 0)


def build_table(kind, pointers, numels, scalars):
    """The table of one call as host arrays: ``(rows, chunk_start)``.
    :param pointers: per tensor ``(p, g, m, v)`` as integers (``v`` is 0 for sgd)
    :param numels:   per tensor, every one >= 1
    :param scalars:  per tensor ``(s, flags)`` of ``row_scalars``
    ``rows`` is a ``ROW`` array; ``chunk_start`` is int32 [n + 1]: 0, then the running sum of ``ceil(numel / CHUNK)``."""
    n = len(numels)
    rows = np.zeros(n, ROW)
    numel = np.asarray(numels, np.int64).reshape(n)
    if n and int(numel.min()) < 1:
        raise ValueError("clean_pvnet_amd.optim: every row of the table needs numel >= 1")
    chunk_start = np.zeros(n + 1, np.int64)
    np.cumsum((numel + (CHUNK - 1)) // CHUNK, out=chunk_start[1:])
    if int(chunk_start[-1]) >= 2 ** 31:
        raise ValueError("clean_pvnet_amd.optim: %d chunks of %d elements; the launch holds fewer than 2^31" % (int(chunk_start[-1]), CHUNK))
    if n:
        ptr = np.asarray(pointers, np.uint64).reshape(n, 4)
        rows["p"], rows["g"], rows["m"], rows["v"] = ptr[:, 0], ptr[:, 1], ptr[:, 2], ptr[:, 3]
        rows["numel"] = numel
        seen, which, distinct = {}, [], []                       # most rows share one (s, flags): convert each once
        for sf in scalars:
            k = seen.get(id(sf))
            if k is None:
                k = seen[id(sf)] = len(distinct)
                distinct.append(sf)
            which.append(k)
        s32, flags = np.zeros((len(distinct), 8), np.float32), np.zeros(len(distinct), np.int32)
        for k, (values, bits) in enumerate(distinct):
            s32[k, :len(values)], flags[k] = values, bits         # binary64 -> float32, once
        rows["s"], rows["flags"] = s32[which], flags[which]
    return rows, chunk_start.astype(np.int32)


def _per_tensor(value, n, what, pair=False):
    """``value`` broadcast to ``n`` tensors: a number (a pair of numbers with ``pair``) or a sequence of ``n`` of them."""
    if isinstance(value, torch.Tensor) and value.dim() == 0:
        value = value.item()
    one = (isinstance(value, (tuple, list)) and len(value) == 2 and not isinstance(value[0], (tuple, list))) if pair \
        else not isinstance(value, (tuple, list, np.ndarray))
    if one:
        return [value] * n
    if len(value) != n:
        raise ValueError("clean_pvnet_amd.optim: %s has %d entries for %d tensors" % (what, len(value), n))
    return list(value)


def _check(lists):
    """The device of the call.  One pass says whether every tensor is as it must be; ``_refuse`` says what is wrong, if not."""
    params = lists[0][1]
    if not params and all(not ts for _, ts in lists):
        return None
    f32, strided = torch.float32, torch.strided
    try:
        dev = params[0].device
        fine = dev.type == "cuda" and all(len(ts) == len(params) for _, ts in lists) and all(
            t.dtype is f32 and t.layout is strided and t.device == dev and t.shape == p.shape and t.is_contiguous()
            for _, ts in lists for t, p in zip(ts, params))
    except (AttributeError, IndexError):                             # something that is no tensor; no parameter at all
        fine = False
    if not fine:
        _refuse(lists)
    return dev


def _refuse(lists):
    """dtype, shape and layout of every tensor, then the devices: one CUDA device for all.  Raises for the first offender."""
    n = len(lists[0][1])
    for what, ts in lists:
        if len(ts) != n:
            raise ValueError("clean_pvnet_amd.optim: %s has %d tensors, params has %d" % (what, len(ts), n))
        for i, t in enumerate(ts):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError("clean_pvnet_amd.optim: %s[%d] must be a tensor, got %s" % (what, i, type(t).__name__))
            if t.dtype != torch.float32:
                raise RuntimeError("clean_pvnet_amd.optim: %s[%d] must be float32, got %s" % (what, i, t.dtype))
            if t.layout != torch.strided:
                raise RuntimeError("clean_pvnet_amd.optim: %s[%d] must be a dense tensor, got %s" % (what, i, t.layout))
    params = lists[0][1]
    for what, ts in lists[1:]:
        for i, t in enumerate(ts):
            if t.shape != params[i].shape:
                raise ValueError("clean_pvnet_amd.optim: %s[%d] must have the shape of params[%d], %s, got %s"
                                 % (what, i, i, tuple(params[i].shape), tuple(t.shape)))
    for what, ts in lists:
        for i, t in enumerate(ts):
            if not t.is_contiguous():
                raise ValueError("clean_pvnet_amd.optim: %s[%d] must be contiguous (shape %s, strides %s)"
                                 % (what, i, tuple(t.shape), tuple(t.stride())))
    dev = params[0].device if n else None
    for what, ts in lists:
        for i, t in enumerate(ts):
            if t.device != dev:
                raise RuntimeError("clean_pvnet_amd.optim: %s[%d] is on %s, params[0] on %s; all tensors must be on one device"
                                   % (what, i, t.device, dev))
    _native.need_cuda(params[0], "params[0] (and every other tensor)", "optim")
    raise RuntimeError("clean_pvnet_amd.optim: the tensors were refused and nothing is wrong with them")      # not reached


def optim_step(kind, params, grads, exp_avg, exp_avg_sq=None, *, steps, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8,
               momentum=0.9, clip_value=None, zero_grad=False, degenerated_to_sgd=True):
    """One optimizer step of every tensor of ``params``, in place, in one launch.
    :param kind:         ``'adam'`` (torch.optim.Adam: no amsgrad, L2 decay), ``'radam'`` (the reference's RAdam) or ``'sgd'``
                         (torch.optim.SGD with momentum, L2 decay)
    :param params:       list of CUDA float32 tensors, contiguous, all on one device; ``grads``, ``exp_avg``, ``exp_avg_sq`` likewise,
                         each of its parameter's shape.  ``exp_avg`` is the momentum buffer of sgd, which takes no ``exp_avg_sq``
    :param steps:        the step count of each tensor after this step (1 on its first: sgd then sets its buffer to the gradient
                         without reading it).  ``steps``, ``lr``, ``weight_decay``, ``betas``, ``eps``, ``momentum`` are one value for
                         all tensors or a sequence with one per tensor
    :param clip_value:   ``c``: every gradient element is clamped to [-c, c] as it is read (a NaN stays NaN); ``p.grad`` keeps its
                         values.  None: no clamp
    :param zero_grad:    store +0 to every gradient element after reading it
    A tensor with ``numel() == 0`` is skipped.  Anything else is a RuntimeError or ValueError that names the tensor."""
    if kind not in KINDS:
        raise ValueError("clean_pvnet_amd.optim: kind must be one of %s, got %r" % (", ".join(sorted(KINDS)), kind))
    params, grads, exp_avg = list(params), list(grads), list(exp_avg)
    lists = [("params", params), ("grads", grads), ("exp_avg", exp_avg)]
    if kind == "sgd":
        if exp_avg_sq is not None:
            raise ValueError("clean_pvnet_amd.optim: sgd takes no exp_avg_sq")
    else:
        if exp_avg_sq is None:
            raise ValueError("clean_pvnet_amd.optim: %s needs exp_avg_sq" % kind)
        exp_avg_sq = list(exp_avg_sq)
        lists.append(("exp_avg_sq", exp_avg_sq))
    dev = _check(lists)
    n = len(params)
    steps, lr, wd = _per_tensor(steps, n, "steps"), _per_tensor(lr, n, "lr"), _per_tensor(weight_decay, n, "weight_decay")
    betas, eps, mu = _per_tensor(betas, n, "betas", pair=True), _per_tensor(eps, n, "eps"), _per_tensor(momentum, n, "momentum")
    keys = [(steps[i], lr[i], wd[i], betas[i][0], betas[i][1], eps[i], mu[i]) for i in range(n)]
    _launch(kind, lists, keys, clip_value, zero_grad, degenerated_to_sgd, dev)


def _launch(kind, lists, keys, clip_value, zero_grad, degenerated_to_sgd, dev=None):
    """The table and the launch.  ``lists`` is [(name, tensors)] for params, grads, exp_avg (and exp_avg_sq), checked here unless
    the caller has (``dev``); ``keys`` per tensor is (step, lr, weight_decay, beta1, beta2, eps, momentum), and rows with equal
    keys share their scalars."""
    if dev is None:
        dev = _check(lists)
    flags = ZERO_GRAD if zero_grad else 0
    if clip_value is not None:
        if not float(clip_value) >= 0:
            raise ValueError("clean_pvnet_amd.optim: clip_value must be >= 0 or None, got %r" % (clip_value,))
        flags |= CLIP
    second = [None] * len(keys) if kind == "sgd" else lists[3][1]
    pointers, numels, scalars, memo = [], [], [], {}
    for i, (p, g, m, v) in enumerate(zip(lists[0][1], lists[1][1], lists[2][1], second)):
        n = p.numel()
        if n == 0:
            continue
        key = keys[i]
        sf = memo.get(key)
        if sf is None:
            step = _step_value(key[0])
            if step < 1:
                raise ValueError("clean_pvnet_amd.optim: steps[%d] must be >= 1 (the count after this step), got %d" % (i, step))
            step_lr, wd, beta1, beta2, eps, mu = (float(x) for x in key[1:])
            sf = memo[key] = row_scalars(kind, step, step_lr, wd, (beta1, beta2), eps, mu, degenerated_to_sgd)
        scalars.append(sf)
        pointers.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), 0 if v is None else v.data_ptr()))
        numels.append(n)
    if not numels:
        return
    rows, chunk_start = build_table(kind, pointers, numels, scalars)
    table = _native.upload(np.concatenate([rows.view(np.uint8), chunk_start.view(np.uint8)]), dev)      # 80 n bytes, then the prefix
    _lib.call("pvv_optim_step", dev, KINDS[kind], table.data_ptr(), table.data_ptr() + rows.nbytes, len(numels),
              int(chunk_start[-1]), float(clip_value) if clip_value is not None else 0.0, flags)


# ---------------------------------------------------------------------------------------------------------------- the classes
def _step_value(step):
    return int(step.item()) if isinstance(step, torch.Tensor) else int(step)


class _Fused(torch.optim.Optimizer):
    """What the three classes share: ``step`` gathers every parameter with a gradient and makes one ``optim_step`` call."""
    kind = None

    def _state_of(self, p, group):
        """(step count after this step, first moment, second moment) of ``p``, the state made on its first step."""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = state["step"]
        state["step"] = step = (step if type(step) is int else _step_value(step)) + 1
        return step, state["exp_avg"], state["exp_avg_sq"]

    def load_state_dict(self, state_dict):
        """``step`` comes as an int (the reference's RAdam, this module) or as torch's scalar tensor; it is kept as an int."""
        super().load_state_dict(state_dict)
        for state in self.state.values():
            if "step" in state:
                state["step"] = _step_value(state["step"])

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, grads, first, second, keys = [], [], [], [], []
        for group in self.param_groups:
            beta1, beta2 = group["betas"] if "betas" in group else (0.0, 0.0)
            hyper = (group["lr"], group["weight_decay"], beta1, beta2, group.get("eps", 0.0), group.get("momentum", 0.0))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("clean_pvnet_amd.optim: %s does not support sparse gradients" % type(self).__name__)
                step, m, v = self._state_of(p, group)
                params.append(p)
                grads.append(g)
                first.append(m)
                second.append(v)
                keys.append((step,) + hyper)
        lists = [("params", params), ("grads", grads), ("exp_avg", first)]
        if self.kind != "sgd":
            lists.append(("exp_avg_sq", second))
        _launch(self.kind, lists, keys, self.clip_value, zero_grad, getattr(self, "degenerated_to_sgd", True))
        return loss


def _check_hyper(lr, eps=0.0, betas=(0.0, 0.0), weight_decay=0.0, momentum=0.0, clip_value=None):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
    if not 0.0 <= weight_decay:
        raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
    if not 0.0 <= momentum:
        raise ValueError("Invalid momentum value: {}".format(momentum))
    if clip_value is not None and not 0.0 <= clip_value:
        raise ValueError("Invalid clip_value: {}".format(clip_value))


class Adam(_Fused):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad, L2 decay) with ``clip_value``: the whole step is
    one launch.  ``self.state[p]`` holds ``step`` (an int; ``state_dict()`` writes it as torch's float32 scalar tensor), ``exp_avg``,
    ``exp_avg_sq``; the param groups carry torch's keys, so ``state_dict()`` loads into ``torch.optim.Adam`` and back."""
    kind = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, clip_value=None):
        _check_hyper(lr, eps, betas, weight_decay, clip_value=clip_value)
        self.clip_value = clip_value
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))

    def _state_of(self, p, group):
        if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
            raise RuntimeError("clean_pvnet_amd.optim: Adam has no amsgrad, maximize or decoupled_weight_decay form")
        return super()._state_of(p, group)

    def state_dict(self):
        """``step`` leaves as torch's float32 scalar tensor: ``torch.optim.Adam`` advances it in place and would not advance an int."""
        out = super().state_dict()
        out["state"] = {k: {**s, "step": torch.tensor(float(_step_value(s["step"])), dtype=torch.float32)} if "step" in s else s
                        for k, s in out["state"].items()}
        return out


class RAdam(_Fused):
    """The reference's ``RAdam`` (lib/utils/optimizer/radam.py:6-95) with ``clip_value``: the whole step is one launch.
    ``self.state[p]`` holds ``step`` (an int, as there), ``exp_avg``, ``exp_avg_sq``; the groups carry its ``buffer`` key for the
    interchange only: ``N_sma`` and ``step_size`` are recomputed per step by the same expressions."""
    kind = "radam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True, *, clip_value=None):
        _check_hyper(lr, eps, betas, clip_value=clip_value)
        self.degenerated_to_sgd, self.clip_value = degenerated_to_sgd, clip_value
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, buffer=[[None, None, None] for _ in range(10)]))



class SGD(_Fused):
    """``torch.optim.SGD(params, lr, momentum, weight_decay=...)`` (no dampening, no nesterov, L2 decay) with ``clip_value``: the
    whole step is one launch.  ``self.state[p]`` holds ``momentum_buffer``, as there; a parameter without one is on its first
    step, where the buffer becomes the gradient."""
    kind = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, clip_value=None):
        _check_hyper(lr, weight_decay=weight_decay, momentum=momentum, clip_value=clip_value)
        if dampening != 0 or nesterov:
            raise ValueError("clean_pvnet_amd.optim: SGD has no dampening and no nesterov form")
        self.clip_value = clip_value
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))

    def _state_of(self, p, group):
        if group.get("dampening") or group.get("nesterov") or group.get("maximize"):
            raise RuntimeError("clean_pvnet_amd.optim: SGD has no dampening, nesterov or maximize form")
        state = self.state[p]
        if state.get("momentum_buffer") is None:
            state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)     # written, not read, on step 1
            return 1, state["momentum_buffer"], None
        return 2, state["momentum_buffer"], None


_CLASSES = {"adam": Adam, "radam": RAdam, "sgd": SGD}
CLIP_VALUE = 40.0                                # the trainer's clip_grad_value_ line (lib/train/trainers/trainer.py:44)


def make_optimizer(cfg, net):
    """The reference's ``make_optimizer`` (lib/train/optimizer.py:12-27) over the classes above, with ``clip_value=40.0``:
    ``cfg.train.optim`` names the class, every trainable parameter of ``net`` becomes a param group of its own with
    ``cfg.train.lr`` and ``cfg.train.weight_decay``; a name with 'adam' in it takes the weight decay as its default too, sgd takes
    momentum 0.9 (and the decay through its groups)."""
    name, lr, wd = cfg.train.optim, cfg.train.lr, cfg.train.weight_decay
    if name not in _CLASSES:
        raise KeyError("clean_pvnet_amd.optim: cfg.train.optim must be one of %s, got %r" % (", ".join(sorted(_CLASSES)), name))
    groups = [{"params": [p], "lr": lr, "weight_decay": wd} for _, p in net.named_parameters() if p.requires_grad]
    if "adam" in name:
        return _CLASSES[name](groups, lr, weight_decay=wd, clip_value=CLIP_VALUE)
    return _CLASSES[name](groups, lr, momentum=0.9, clip_value=CLIP_VALUE)
