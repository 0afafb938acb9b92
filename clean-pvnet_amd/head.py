"""PVNet's full-resolution output head on the device (``libpvnet_vote.so``, "PVNet output head" in include/pvnet_vote.h).

The tail of the reference's ``Resnet18.forward`` (lib/networks/pvnet/resnet18.py:53-59, 90-94) -- ``up2storaw``, the ``cat`` with the
image and ``convraw``: Conv3x3 without bias, BatchNorm2d, LeakyReLU(0.1), Conv1x1 with bias -- is six map-sized torch ops at full
resolution.  ``pvnet_head`` is one launch that reads ``fm`` and the image and writes the ``seg_dim + ver_dim`` output channels,
with no full-resolution intermediate in memory; ``PVNetHead`` holds ``convraw`` under the reference's parameter names, so the
``convraw.*`` entries of a reference checkpoint load unchanged.  The result equals the numpy twin (tests/head_twin.py) bit for bit
(-0 == +0); parity with torch's own upsample kernel and with MIOpen's convolution is unpinned.  ``compute="bfloat16"`` is the opt-in matrix-core mode
(``PVV_HEAD_COMPUTE_BF16`` in ``pvv_head_forward``'s ``out_kind``): operands rounded to bfloat16, float32 accumulation in an unpinned order, held to the bound of
tests/head_bf16_twin.py.  Forward
only, BatchNorm in eval mode: inference.  CUDA float32 tensors, the current stream, nothing read back, no CPU fallback.

``pvnet_stage`` is the stage mode of the same entry point (``PVV_HEAD_STAGE``): one of the three decoder steps before the head
(resnet18.py:31-51, 81-89) -- upsample or none, ``cat`` with the skip tensor, Conv3x3, BatchNorm, LeakyReLU -- in one launch for
any number of input channels and up to 128 output channels.  ``PVNetDecoder`` holds ``conv8s``, ``conv4s``, ``conv2s`` and
``convraw`` under the reference's names and takes the backbone's outputs to ``{'seg', 'vertex'}`` in four launches; its stages
equal tests/decoder_twin.py bit for bit.  ``compute="bfloat16"`` of ``pvnet_stage``
(``stage_compute`` of the decoder) is the stages' own opt-in matrix-core mode, ``PVV_HEAD_STAGE_BF16``, held to the bound
of tests/decoder_bf16_twin.py.
"""
import torch
from torch import nn

from . import _native

_lib = _native.bind("head", "libpvnet_vote.so", last_error="pvv_last_error")

MAX_UPSAMPLE = 1 << 28             # elements ``upsample2x`` agrees to write
MAX_M = 64                         # output channels of either convolution
MAX_STAGE_M = 128                  # output channels of a decoder stage (PVV_HEAD_STAGE_MAX_M)
STAGE, SAME_RES = 0x400, 0x800     # or-ed into out_kind: PVV_HEAD_STAGE, PVV_HEAD_SAME_RES
STAGE_BF16 = 0x2000                # or-ed into out_kind beside STAGE: PVV_HEAD_STAGE_BF16, the stage's bfloat16 mode
OUT_KINDS = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
COMPUTE_MODES = {"float32": 0, "bfloat16": 0x100}                   # or-ed into out_kind; 0x100: PVV_HEAD_COMPUTE_BF16


def _check(named):
    _native.check_tensors(named, (torch.float32,), "head")
    if torch.is_grad_enabled() and any(t.requires_grad for _, t in named):
        raise RuntimeError("clean_pvnet_amd.head: forward only -- there is no backward pass; call under torch.no_grad() "
                           "or with tensors that do not require grad")


def _compute(compute):
    if not isinstance(compute, str) or compute not in COMPUTE_MODES:
        raise ValueError("clean_pvnet_amd.head: compute must be one of %s, got %r" % (", ".join(map(repr, COMPUTE_MODES)), compute))
    return COMPUTE_MODES[compute]


def _fm(fm):
    if fm.dim() != 4 or fm.shape[1] < 1:
        raise RuntimeError("clean_pvnet_amd.head: fm must be [B, C2 >= 1, h, w], got %s" % (tuple(fm.shape),))
    B, C2, h, w = (int(v) for v in fm.shape)
    t, stride = _native.per_image(fm.detach(), "fm", C2, h, w)
    return (B, C2, h, w), t, stride


def pvnet_head(fm, x, weight1, scale, shift, weight2, bias2, *, negative_slope=0.1, out_dtype=torch.float32,
               compute="float32"):
    """``convraw(cat([up2storaw(fm), x], 1))`` with the BatchNorm folded into ``scale`` and ``shift`` (``fold_bn``).
    :param fm:       [B,C2,h,w] float32 CUDA tensor, the half-resolution feature map
    :param x:        [B,C0,2h,2w], the image; C0 may be 0
    :param weight1:  [M1, C2+C0, 3, 3], ``fm``'s channels first; [M1] ``scale`` and ``shift``
    :param weight2:  [M2, M1] or [M2, M1, 1, 1]; ``bias2`` [M2]; M1, M2 <= 64
    :return:         [B,M2,2h,2w] of ``out_dtype``: float32, or float16 / bfloat16 rounded to nearest even at the store
    ``fm`` and ``x`` may be views (channel slices of larger tensors): they are read by their image strides.  The contract is in
    include/pvnet_vote.h: torch's float32 align_corners source index and blend, zero padding ring, one ``fmaf`` chain per output
    over k = channel*9 + tap from +0, ``fmaf(acc, scale, shift)``, the leaky slope, one ``fmaf`` chain over M1 from the bias.
    :param compute:  ``"float32"`` (that contract, that kernel), or ``"bfloat16"``, the matrix-core mode of
                     ``PVV_HEAD_COMPUTE_BF16``: every operand of the two convolutions is rounded once to bfloat16 and the
                     products are accumulated in float32 in an order that is not pinned: tests/head_bf16_twin.py bounds it."""
    mode = _compute(compute)
    named = [("fm", fm), ("x", x), ("weight1", weight1), ("scale", scale), ("shift", shift), ("weight2", weight2), ("bias2", bias2)]
    _check(named)
    if out_dtype not in OUT_KINDS:
        raise RuntimeError("clean_pvnet_amd.head: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    (B, C2, h, w), f, f_stride = _fm(fm)
    H, W = 2 * h, 2 * w
    if x.dim() != 4 or x.shape[0] != B:
        raise RuntimeError("clean_pvnet_amd.head: x must be [B = %d, C0, %d, %d], got %s" % (B, H, W, tuple(x.shape)))
    C0 = int(x.shape[1])
    xi, x_stride = _native.per_image(x.detach(), "x", C0, H, W, module="head")
    if weight1.dim() != 4 or tuple(weight1.shape[1:]) != (C2 + C0, 3, 3):
        raise RuntimeError("clean_pvnet_amd.head: weight1 must be [M1, C2 + C0 = %d, 3, 3], got %s" % (C2 + C0, tuple(weight1.shape)))
    M1, M2 = int(weight1.shape[0]), int(weight2.shape[0])
    if tuple(weight2.shape) not in ((M2, M1), (M2, M1, 1, 1)):
        raise RuntimeError("clean_pvnet_amd.head: weight2 must be [M2, M1 = %d] or [M2, %d, 1, 1], got %s" % (M1, M1, tuple(weight2.shape)))
    if tuple(scale.shape) != (M1,) or tuple(shift.shape) != (M1,) or tuple(bias2.shape) != (M2,):
        raise RuntimeError("clean_pvnet_amd.head: scale and shift must be [%d] and bias2 [%d], got %s, %s, %s"
                           % (M1, M2, tuple(scale.shape), tuple(shift.shape), tuple(bias2.shape)))
    if not (1 <= M1 <= MAX_M and 1 <= M2 <= MAX_M):
        raise ValueError("clean_pvnet_amd.head: M1 and M2 must lie in [1, %d], got %d and %d" % (MAX_M, M1, M2))
    out = torch.empty(B, M2, H, W, dtype=out_dtype, device=fm.device)
    if out.numel() == 0:
        return out
    w1, sc, sh, w2, b2 = (t.detach().contiguous() for t in (weight1, scale, shift, weight2, bias2))
    _lib.call("pvv_head_forward", fm.device, f.data_ptr(), f_stride, xi.data_ptr() if C0 else None, x_stride, w1.data_ptr(),
              sc.data_ptr(), sh.data_ptr(), w2.data_ptr(), b2.data_ptr(), B, C2, C0, h, w, H, W, M1, M2, float(negative_slope),
              OUT_KINDS[out_dtype] | mode, out.data_ptr())
    return out


def upsample2x(fm):
    """``nn.UpsamplingBilinear2d(scale_factor=2)`` by the contract's float32 formula (``pvv_head_upsample``): [B,C2,2h,2w], the
    same device function as ``pvnet_head`` blends with, written out so that a test can tell the upsample from the convolutions."""
    _native.check_tensors([("fm", fm)], (torch.float32,), "head")
    if fm.dim() == 4 and 4 * fm.numel() > MAX_UPSAMPLE:
        raise ValueError("clean_pvnet_amd.head: an upsampled tensor of %d elements; at most 2^28 are written" % (4 * fm.numel()))
    (B, C2, h, w), f, f_stride = _fm(fm)
    u = torch.empty(B, C2, 2 * h, 2 * w, dtype=torch.float32, device=fm.device)
    if u.numel() == 0:
        return u
    _lib.call("pvv_head_upsample", fm.device, f.data_ptr(), f_stride, B, C2, h, w, 2 * h, 2 * w, u.data_ptr())
    return u


def fold_bn(bn):
    """(scale, shift) float32 [M] of an eval-mode ``BatchNorm2d``, on its device: in binary64 scale = weight / sqrt(running_var +
    eps) and shift = bias - running_mean * scale from the unrounded scale, each rounded once.  A BatchNorm without affine
    parameters or running statistics is refused."""
    if not isinstance(bn, nn.modules.batchnorm._BatchNorm):
        raise TypeError("clean_pvnet_amd.head: fold_bn takes a BatchNorm module, got %s" % type(bn).__name__)
    if bn.weight is None or bn.bias is None:
        raise ValueError("clean_pvnet_amd.head: fold_bn needs a BatchNorm with affine parameters (affine=True)")
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError("clean_pvnet_amd.head: fold_bn needs a BatchNorm with running statistics (track_running_stats=True)")
    with torch.no_grad():
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        shift = bn.bias.double() - bn.running_mean.double() * scale
        return scale.float(), shift.float()


def cached_fold(cache, slot, bn):
    """``fold_bn(bn)`` kept in ``cache[slot]``: computed once and again whenever one of the BatchNorm's tensors changes
    (``_version`` counts the in-place writes; a loaded or moved tensor is another object)."""
    if bn.weight is None or bn.running_mean is None:
        return fold_bn(bn)                                          # raises
    tensors = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    key = tuple((id(t), t._version, t.device) for t in tensors) + (bn.eps,)
    if cache.get(slot) is None or cache[slot][0] != key:
        cache[slot] = (key, fold_bn(bn))
    return cache[slot][1]


def pvnet_stage(a, skip, weight, scale, shift, *, upsample=True, negative_slope=0.1, out_dtype=torch.float32,
                compute="float32"):
    """One decoder stage, ``LeakyReLU(BatchNorm(Conv3x3(cat([up(a), skip], 1))))`` with the BatchNorm folded into ``scale`` and
    ``shift`` (``fold_bn``), in one launch: ``pvv_head_forward`` with ``PVV_HEAD_STAGE``.
    :param a:        [B,C2,h,w] float32 CUDA tensor: the coarser feature map (``upsample=True``: ``UpsamplingBilinear2d(2)``
                     by the head's float32 formula), or one at the output's resolution (``upsample=False``: ``conv8s``)
    :param skip:     [B,C0,H,W] with H, W = 2h, 2w (h, w without the upsample); C0 may be 0
    :param weight:   [M, C2+C0, 3, 3], ``a``'s channels first; [M] ``scale`` and ``shift``; M <= 128, any C2 + C0
    :return:         [B,M,H,W] of ``out_dtype``: float32, or float16 / bfloat16 rounded to nearest even at the store
    ``a`` and ``skip`` may be views (channel slices of larger tensors): they are read by their image strides.  The contract
    is the head's up to the activation (include/pvnet_vote.h, "PVNet decoder stage").
    :param compute:  ``"float32"`` (that contract, that kernel), or ``"bfloat16"``, the matrix-core mode of
                     ``PVV_HEAD_STAGE_BF16``: ``cat([up(a), skip])`` and ``weight`` are rounded once to bfloat16 inside the
                     launch and the products are accumulated in float32 in an order that is not pinned:
                     tests/decoder_bf16_twin.py bounds it.  ``a``, ``skip`` and ``weight`` stay float32 tensors."""
    mode = STAGE_BF16 if _compute(compute) else 0
    named = [("a", a), ("skip", skip), ("weight", weight), ("scale", scale), ("shift", shift)]
    _check(named)
    if out_dtype not in OUT_KINDS:
        raise RuntimeError("clean_pvnet_amd.head: out_dtype must be float32, float16 or bfloat16, got %s" % (out_dtype,))
    if a.dim() != 4 or a.shape[1] < 1:
        raise RuntimeError("clean_pvnet_amd.head: a must be [B, C2 >= 1, h, w], got %s" % (tuple(a.shape),))
    B, C2, h, w = (int(v) for v in a.shape)
    H, W = (2 * h, 2 * w) if upsample else (h, w)
    if skip.dim() != 4 or skip.shape[0] != B:
        raise RuntimeError("clean_pvnet_amd.head: skip must be [B = %d, C0, %d, %d], got %s" % (B, H, W, tuple(skip.shape)))
    if tuple(skip.shape[2:]) != (H, W):
        raise RuntimeError("clean_pvnet_amd.head: skip must be %d x %d, %s a's %d x %d, got %d x %d -- a skip tensor of another "
                           "size needs the reference's resample of fm (the fm.shape[2]==136 branch, resnet18.py:83-84), which "
                           "is not supported" % (H, W, "twice" if upsample else "as", h, w, skip.shape[2], skip.shape[3]))
    C0 = int(skip.shape[1])
    f, f_stride = _native.per_image(a.detach(), "a", C2, h, w)
    xi, x_stride = _native.per_image(skip.detach(), "skip", C0, H, W)
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (C2 + C0, 3, 3):
        raise RuntimeError("clean_pvnet_amd.head: weight must be [M, C2 + C0 = %d, 3, 3], got %s" % (C2 + C0, tuple(weight.shape)))
    M = int(weight.shape[0])
    if tuple(scale.shape) != (M,) or tuple(shift.shape) != (M,):
        raise RuntimeError("clean_pvnet_amd.head: scale and shift must be [%d], got %s, %s" % (M, tuple(scale.shape), tuple(shift.shape)))
    if not 1 <= M <= MAX_STAGE_M:
        raise ValueError("clean_pvnet_amd.head: a stage's M must lie in [1, %d], got %d" % (MAX_STAGE_M, M))
    out = torch.empty(B, M, H, W, dtype=out_dtype, device=a.device)
    if out.numel() == 0:
        return out
    w1, sc, sh = (t.detach().contiguous() for t in (weight, scale, shift))
    _lib.call("pvv_head_forward", a.device, f.data_ptr(), f_stride, xi.data_ptr() if C0 else None, x_stride, w1.data_ptr(),
              sc.data_ptr(), sh.data_ptr(), None, None, B, C2, C0, h, w, H, W, M, 1, float(negative_slope),
              OUT_KINDS[out_dtype] | STAGE | (0 if upsample else SAME_RES) | mode, out.data_ptr())
    return out


class PVNetHead(nn.Module):
    """``up2storaw`` and ``convraw`` of the reference's ``Resnet18`` (resnet18.py:53-59) as one module: ``self.convraw`` has the
    reference's layers and names, ``forward(fm, x)`` is resnet18.py:90-96 up to the dict, through ``pvnet_head``.  ``compute`` is
    ``pvnet_head``'s mode, an attribute that may be set between calls; the parameters stay float32 in every mode."""

    def __init__(self, ver_dim, seg_dim, s2dim=32, raw_dim=32, image_dim=3, compute="float32"):
        super().__init__()
        _compute(compute)
        self.ver_dim, self.seg_dim, self.compute = ver_dim, seg_dim, compute
        self.convraw = nn.Sequential(
            nn.Conv2d(image_dim + s2dim, raw_dim, 3, 1, 1, bias=False),
            nn.BatchNorm2d(raw_dim),
            nn.LeakyReLU(0.1, True),
            nn.Conv2d(raw_dim, seg_dim + ver_dim, 1, 1)
        )
        self._folded = {}

    @classmethod
    def from_state_dict(cls, sd, seg_dim=2, prefix="convraw.", image_dim=3, compute="float32"):
        """A head sized from the ``<prefix>*`` tensors of a state dict (a whole ``Resnet18`` checkpoint will do), loaded with
        them, in eval mode.  ``seg_dim`` of the output channels are the segmentation's (2 in PVNet), the rest the vertex field's."""
        w1, w2 = sd[prefix + "0.weight"], sd[prefix + "3.weight"]
        m = cls(int(w2.shape[0]) - seg_dim, seg_dim, s2dim=int(w1.shape[1]) - image_dim, raw_dim=int(w1.shape[0]), image_dim=image_dim,
                compute=compute)
        m.load_state_dict({"convraw." + k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
        return m.eval()

    def folded(self):
        """``fold_bn`` of the BatchNorm, computed once and again whenever one of its tensors changes (``_version`` counts the
        in-place writes; a loaded or moved tensor is another object)."""
        return cached_fold(self._folded, "convraw", self.convraw[1])

    def forward(self, fm, x):
        if self.training:
            raise RuntimeError("clean_pvnet_amd.head: forward only -- the BatchNorm is folded from its running statistics; "
                               "call .eval() first")
        conv1, act, conv2 = self.convraw[0], self.convraw[2], self.convraw[3]
        named = [("fm", fm), ("x", x), ("weight1", conv1.weight), ("weight2", conv2.weight), ("bias2", conv2.bias)]
        _check(named)
        scale, shift = self.folded()
        out = pvnet_head(fm, x, conv1.weight, scale, shift, conv2.weight, conv2.bias, negative_slope=act.negative_slope,
                         compute=self.compute)
        return {"seg": out[:, :self.seg_dim], "vertex": out[:, self.seg_dim:]}


class PVNetDecoder(nn.Module):
    """The decoder of the reference's ``Resnet18`` (resnet18.py:31-59, 81-96): ``conv8s``, ``conv4s``, ``conv2s`` and
    ``convraw`` with the reference's layers and names, so the matching entries of a ``Resnet18`` checkpoint load unchanged.
    ``forward(x, x2s, x4s, x8s, xfc)`` takes the image and the backbone's outputs to ``{'seg', 'vertex'}`` in four launches:
    three ``pvnet_stage`` calls and ``pvnet_head``.  ``compute`` is the head's mode only; ``stage_compute`` is the three
    stages' (``pvnet_stage``'s ``compute``: ``"float32"``, or ``"bfloat16"``, held to tests/decoder_bf16_twin.py's bound).
    Both are attributes that may be set between calls; the parameters stay float32 in every mode.  The
    reference's resample of a 136-row map to 135 x 180 (resnet18.py:83-84) is not supported: the skip tensors must have
    twice the size of the map below them."""
    STAGES = ("conv8s", "conv4s", "conv2s")

    def __init__(self, ver_dim, seg_dim, fcdim=256, s8dim=128, s4dim=64, s2dim=32, raw_dim=32, compute="float32",
                 stage_compute="float32"):
        super().__init__()
        _compute(compute), _compute(stage_compute)
        self.ver_dim, self.seg_dim, self.compute, self.stage_compute = ver_dim, seg_dim, compute, stage_compute

        def stage(cin, cout):
            return nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.LeakyReLU(0.1, True))
        self.conv8s = stage(128 + fcdim, s8dim)
        self.conv4s = stage(64 + s8dim, s4dim)
        self.conv2s = stage(64 + s4dim, s2dim)
        self.convraw = nn.Sequential(
            nn.Conv2d(3 + s2dim, raw_dim, 3, 1, 1, bias=False),
            nn.BatchNorm2d(raw_dim),
            nn.LeakyReLU(0.1, True),
            nn.Conv2d(raw_dim, seg_dim + ver_dim, 1, 1)
        )
        self._folded = {}

    @classmethod
    def from_state_dict(cls, sd, seg_dim=2, compute="float32", stage_compute="float32"):
        """A decoder sized from the ``conv8s.*``, ``conv4s.*``, ``conv2s.*`` and ``convraw.*`` tensors of a state dict (a
        whole ``Resnet18`` checkpoint will do), loaded with them, in eval mode."""
        w8, w4, w2, wr, wo = (sd[k] for k in ("conv8s.0.weight", "conv4s.0.weight", "conv2s.0.weight", "convraw.0.weight",
                                              "convraw.3.weight"))
        m = cls(int(wo.shape[0]) - seg_dim, seg_dim, fcdim=int(w8.shape[1]) - 128, s8dim=int(w8.shape[0]), s4dim=int(w4.shape[0]),
                s2dim=int(w2.shape[0]), raw_dim=int(wr.shape[0]), compute=compute, stage_compute=stage_compute)
        m.load_state_dict({k: v for k, v in sd.items() if k.split(".")[0] in cls.STAGES + ("convraw",)})
        return m.eval()

    @classmethod
    def from_module(cls, net, compute="float32", stage_compute="float32"):
        """A decoder that shares ``net.conv8s``, ``net.conv4s``, ``net.conv2s`` and ``net.convraw`` -- the four ``Sequential``s
        of a reference network -- without copying them: it follows the network's parameters and its train / eval mode."""
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        _compute(compute), _compute(stage_compute)
        m.ver_dim, m.seg_dim, m.compute, m.stage_compute = net.ver_dim, net.seg_dim, compute, stage_compute
        for name in cls.STAGES + ("convraw",):
            setattr(m, name, getattr(net, name))
        m._folded = {}
        m.train(net.training)
        return m

    def folded(self, name):
        """``fold_bn`` of ``<name>``'s BatchNorm, cached by ``PVNetHead.folded``'s rule."""
        return cached_fold(self._folded, name, getattr(self, name)[1])

    def forward(self, x, x2s, x4s, x8s, xfc):
        if self.training or any(getattr(self, name).training for name in self.STAGES + ("convraw",)):
            raise RuntimeError("clean_pvnet_amd.head: forward only -- the BatchNorms are folded from their running statistics; "
                               "call .eval() first")
        convs = [getattr(self, name)[0].weight for name in self.STAGES]
        raw1, act, raw2 = self.convraw[0], self.convraw[2], self.convraw[3]
        _check([("x", x), ("x2s", x2s), ("x4s", x4s), ("x8s", x8s), ("xfc", xfc)]
               + [(name + ".weight", w) for name, w in zip(self.STAGES, convs)]
               + [("convraw.weight1", raw1.weight), ("convraw.weight2", raw2.weight), ("convraw.bias2", raw2.bias)])
        fm = xfc
        for name, w, skip in zip(self.STAGES, convs, (x8s, x4s, x2s)):
            scale, shift = self.folded(name)
            fm = pvnet_stage(fm, skip, w, scale, shift, upsample=name != "conv8s",
                             negative_slope=getattr(self, name)[2].negative_slope, compute=self.stage_compute)
        scale, shift = self.folded("convraw")
        out = pvnet_head(fm, x, raw1.weight, scale, shift, raw2.weight, raw2.bias, negative_slope=act.negative_slope,
                         compute=self.compute)
        return {"seg": out[:, :self.seg_dim], "vertex": out[:, self.seg_dim:]}
