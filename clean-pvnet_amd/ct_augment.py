"""The T-LESS detector's training batch and its input preparation for a batch on the device (``libpvnet_vote.so``, the section
"Detector augmentation" of include/pvnet_vote.h).

The reference produces a detector sample on a CPU core: ``cut_and_paste`` puts six object cut-outs on a background
(lib/utils/tless/tless_utils.py:86-97), ``augment`` warps the 540 x 720 canvas to 416 x 512 with a drawn scale and centre, runs
``data_utils.color_aug`` and normalises (tless_utils.py:18-63, lib/utils/data_utils.py:123-156, 172-210), ``Dataset.get_bbox``
warps a float mask per instance to the output map and takes its bounding rectangle (lib/datasets/tless/ct.py:58-70), and a float32
image is copied to the device.  Here the uint8 background and cut-outs go to the device once and ``ct_compose`` -> ``ct_augment``
-> ``ct_train.ct_targets`` hand ``ct_train.NetworkWrapper`` its batch on one stream; ``ct_augment(train=False, label=None)`` is the
detector's input preparation at inference (``augment(img, 'test')``).

The kernels hold no random number generator and evaluate no transcendental: ``draws`` returns a host table (``COLUMNS``), and
what depends only on the draws and the sizes -- scale, border, centre with their ``//`` and float32 steps, the closed form of
``get_affine_transform`` and its inverse, the rounded alphas, the lighting vector -- is computed here in binary64 and uploaded as
one small block per call.  What depends on pixels stays on the device: the instance boxes, the placements, the paste, the warp,
the grey mean, the boxes on the output map.  Each function equals its numpy twin (tests/ct_augment_twin.py) byte for byte; the
control flow and the colour arithmetic are the reference's own (tests/golden/ct_augment_*.npz); parity of the resampling with
OpenCV is unpinned.  Deviations: an instance with an empty mask or beyond ``num[b]`` is skipped and an
instance larger than the canvas is placed at 0 with its outside dropped, where the reference raises.  CUDA tensors in and out,
the current stream, nothing read back, no state, no CPU fallback.
"""
import ctypes
import itertools
import math

import numpy as np

from . import _native

_lib = _native.bind("ct_augment", "libpvnet_vote.so", last_error="pvv_last_error")

# per sample, then (place_y, place_x) per instance
COLUMNS = ("scale", "center_x", "center_y", "order", "alpha_0", "alpha_1", "alpha_2", "normal_0", "normal_1", "normal_2", "rot")
N_SAMPLE = len(COLUMNS)
NORMAL_COLUMNS = (7, 8, 9)               # standard normals; every other column is a uniform in [0, 1)
MAX_N, MAX_SIDE, MAX_BATCH = 16, 16384, 65535
ORDERS = tuple(itertools.permutations(range(3)))     # of (brightness, contrast, saturation), lexicographic
BOXES = {"linear": 0, "nearest": 1}                  # PVV_CT_BOXES_LINEAR, PVV_CT_BOXES_NEAREST
COLOR_VAR, LIGHT_STD = 0.4, 0.1                      # data_utils.py:209-210
# lib/utils/tless/tless_config.py:4-15, float32 there; channel 0 is the blue one
MEAN, STD = (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835)
EIG_VAL = (0.2141788, 0.01817699, 0.00341571)
EIG_VEC = ((-0.58752847, -0.69563484, 0.41340352), (-0.5832747, 0.00994535, -0.81221408), (-0.56089297, 0.71832671, 0.41158938))

PARAM = np.dtype([("inv_in", "<f8", 6), ("inv_out", "<f8", 6), ("light", "<f8", 3), ("a", "<f4", 3), ("oma", "<f4", 3),
                  ("order", "<i4", 3), ("pad", "<i4")])
assert PARAM.itemsize == 160                          # PVV_CT_AUGMENT_PARAM_BYTES
F32 = np.float32


def draws(B, N, generator=None):
    """The random numbers of a batch: a host float64 array [B, 11 + 2 N], one row per sample.  Columns 0-10 are ``COLUMNS``: the
    scale uniform, the two centre uniforms (x, y), the order uniform u (``floor(6 u)`` selects the permutation of brightness,
    contrast, saturation in lexicographic order), three alpha uniforms consumed in the drawn order, three standard normals for
    the lighting step and a reserved rotation uniform; columns 11 + 2 n and 12 + 2 n place instance n (dst_y, dst_x).  Drawn
    from torch's CPU generator (``torch.manual_seed`` governs it) or from ``generator``."""
    import torch
    B, N = int(B), int(N)
    d = torch.rand(B, N_SAMPLE + 2 * N, dtype=torch.float64, generator=generator).numpy()
    d[:, list(NORMAL_COLUMNS)] = torch.randn(B, 3, dtype=torch.float64, generator=generator).numpy()
    return d


_draws = draws                     # (``draws`` is also the name of an argument below)


def _check_draws(d, B, N):
    d = np.asarray(d)
    if d.dtype != np.float64 or d.ndim != 2 or d.shape[0] != B or d.shape[1] < N_SAMPLE + 2 * N:
        raise ValueError("clean_pvnet_amd.ct_augment: draws must be a host float64 array [%d, >= %d], got %s %s"
                         % (B, N_SAMPLE + 2 * N, d.shape, d.dtype))
    uni = np.delete(d, NORMAL_COLUMNS, axis=1)
    if not ((uni >= 0) & (uni < 1)).all() or not np.isfinite(d).all():
        raise ValueError("clean_pvnet_amd.ct_augment: the uniform draws must lie in [0, 1) and the normals be finite")
    return d


def randint(lo, hi, u):
    """``np.random.randint(lo, hi)`` from one uniform: ``lo + floor(u * (hi - lo))``; ``lo`` where numpy raises (hi <= lo)."""
    lo, hi = int(lo), int(hi)
    return lo if hi <= lo else lo + min(int(math.floor(float(u) * float(hi - lo))), hi - lo - 1)


def center_scale(H, W, u, scale_range, train):
    """``center`` and ``scale`` of tless_utils.augment, lines 20-41: (cx, cy, scale), the scale the same on both axes.  Train: the
    scale is float32(max(H, W)) times the drawn factor rounded to float32, multiplied in float32; the borders are float32 with
    their ``//``; the centre is an integer."""
    if not train:
        return float(F32(W / 2.)), float(F32(H / 2.)), float(max(H, W))
    factor = scale_range[0] + (scale_range[1] - scale_range[0]) * float(u[0])
    s = F32(max(H, W)) * F32(factor)
    c = []
    for size, v in ((W, u[1]), (H, u[2])):
        half = np.floor_divide(s, F32(2))
        border = half if s < size else F32(size) - half
        border_r = max(F32(size) - border, border + F32(1))
        c.append(float(randint(border, border_r, v)))
    return c[0], c[1], float(s)


def affine(cx, cy, scale, rot, dw, dh):
    """The closed form of ``get_affine_transform((cx, cy), scale, rot, (dw, dh))`` (data_utils.py:123-156) in binary64: the
    similarity that takes the centre to the middle of the destination, ``scale`` source pixels to ``dw`` and turns by ``-rot``
    degrees.  [2][3] as nested lists."""
    k = float(dw) / float(scale)
    if rot == 0:
        cs, sn = 1.0, 0.0
    else:
        rad = math.pi * float(rot) / 180
        cs, sn = math.cos(rad), math.sin(rad)
    a, b = k * cs, k * sn
    return [[a, b, dw * 0.5 - (a * cx + b * cy)], [-b, a, dh * 0.5 - (a * cy - b * cx)]]


def invert_affine(M):
    """[2][3] -> 6 floats in the operation order of OpenCV's ``invertAffineTransform`` (csrc/warp.hpp); a singular map gives zeros."""
    m = [float(v) for row in M for v in row]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1. / D if D != 0 else 0.
    A11, A22, m1, m3 = m[4] * D, m[0] * D, m[1] * (-D), m[3] * (-D)
    return [A11, m1, -A11 * m[2] - m1 * m[5], m3, A22, -m3 * m[2] - A22 * m[5]]


def colour_params(u, eig_val, eig_vec):
    """(order, a, oma, light) of one sample: the three steps in the drawn order with alpha = 1 + uniform(-0.4, 0.4) and 1 - alpha,
    each rounded to float32 where numpy rounds it (a float32 array or scalar times a Python float), and the binary64 lighting
    vector eigvec . (eigval * (0.1 z)) with float32 eigval, eigvec widened."""
    order = ORDERS[min(int(math.floor(6 * float(u[3]))), 5)]
    alpha = [1. + (-COLOR_VAR + (COLOR_VAR - -COLOR_VAR) * float(u[4 + i])) for i in range(3)]
    a, oma = [F32(v) for v in alpha], [F32(1 - v) for v in alpha]
    ev = [float(F32(v)) * (0.0 + LIGHT_STD * float(u[7 + i])) for i, v in enumerate(eig_val)]
    light = [(float(F32(r[0])) * ev[0] + float(F32(r[1])) * ev[1]) + float(F32(r[2])) * ev[2] for r in eig_vec]
    return order, a, oma, light


def host_block(d, H, W, *, train=True, input_size=(416, 512), down_ratio=4, scale_range=(0.6, 1.4), rot=0.0, eig_val=EIG_VAL,
               eig_vec=EIG_VEC):
    """Everything ``ct_augment`` derives from the draws and the sizes: (block, meta).  ``block`` is the [B] record array that
    ``pvv_ct_augment`` reads; ``meta`` holds ``center`` [B,2] float32, ``scale`` [B,2] float32, ``trans_input`` and
    ``trans_output`` [B,2,3] float64 and the sizes (ih, iw, oh, ow)."""
    B = len(d)
    if train:
        ih, iw = int(input_size[0]), int(input_size[1])
    else:
        ih, iw = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        rot = 0.0
    oh, ow = ih // int(down_ratio), iw // int(down_ratio)
    block = np.zeros(B, PARAM)
    meta = {"center": np.zeros((B, 2), F32), "scale": np.zeros((B, 2), F32), "trans_input": np.zeros((B, 2, 3)),
            "trans_output": np.zeros((B, 2, 3)), "sizes": (ih, iw, oh, ow)}
    for b in range(B):
        cx, cy, s = center_scale(H, W, d[b], scale_range, train)
        t_in, t_out = affine(cx, cy, s, rot, iw, ih), affine(cx, cy, s, rot, ow, oh)
        meta["center"][b], meta["scale"][b], meta["trans_input"][b], meta["trans_output"][b] = (cx, cy), (s, s), t_in, t_out
        block["inv_in"][b], block["inv_out"][b] = invert_affine(t_in), invert_affine(t_out)
        if train:
            block["order"][b], block["a"][b], block["oma"][b], block["light"][b] = colour_params(d[b], eig_val, eig_vec)
    return block, meta


def _call(symbol, dev, *args):
    _lib.call(symbol, dev, *args)


def _check_img(img, what):
    return _native.check_images(img, what, "ct_augment", MAX_BATCH, MAX_SIDE)


def ct_compose(bg, inst_img, inst_mask, num, draws):
    """The reference's ``cut_and_paste`` (tless_utils.py:86-97) for every instance of a batch.
    :param bg:        [B,H,W,3] uint8 CUDA tensor, the backgrounds at the canvas' size
    :param inst_img:  [B,N,h,w,3] uint8, the cut-outs' images; N <= 16
    :param inst_mask: [B,N,h,w] uint8 or bool; the object is ``mask != 0``
    :param num:       [B] int32 or int64: the first ``num[b]`` instances of sample b are pasted
    :param draws:     [B, >= 11 + 2 N] host float64 (``draws``); the placement columns are used
    :return: dict: ``img`` [B,H,W,3] uint8, ``label`` [B,H,W] uint8 (0 background, n + 1 instance n; later instances overwrite
             earlier ones) and ``place`` [B,N,6] int32 (y_min, x_min, h, w, dst_y, dst_x; a skipped instance is (0, 0, -1, -1, 0, 0))."""
    import torch
    B, H, W = _check_img(bg, "bg")
    for what, t in (("inst_img", inst_img), ("inst_mask", inst_mask), ("num", num)):
        _native.need_cuda(t, what, "ct_augment")
    if inst_img.dtype != torch.uint8 or inst_mask.dtype not in (torch.uint8, torch.bool) or num.dtype not in (torch.int32, torch.int64):
        raise TypeError("clean_pvnet_amd.ct_augment: inst_img must be uint8, inst_mask uint8 or bool, num int32 or int64, got %s, %s, %s"
                        % (inst_img.dtype, inst_mask.dtype, num.dtype))
    if inst_img.dim() != 5 or inst_img.shape[0] != B or inst_img.shape[4] != 3:
        raise ValueError("clean_pvnet_amd.ct_augment: inst_img must be [B = %d, N, h, w, 3], got %s" % (B, tuple(inst_img.shape)))
    N, h, w = (int(v) for v in inst_img.shape[1:4])
    if not (1 <= N <= MAX_N and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("clean_pvnet_amd.ct_augment: N must lie in [1, %d] and the cut-outs' sides in [1, %d], got %s" % (MAX_N, MAX_SIDE, tuple(inst_img.shape)))
    if tuple(inst_mask.shape) != (B, N, h, w):
        raise ValueError("clean_pvnet_amd.ct_augment: inst_mask must be [%d, %d, %d, %d], got %s" % (B, N, h, w, tuple(inst_mask.shape)))
    if tuple(num.shape) != (B,):
        raise ValueError("clean_pvnet_amd.ct_augment: num must be [B = %d], got %s" % (B, tuple(num.shape)))
    d = _check_draws(draws, B, N)
    dev = bg.device
    b_, ii, im, nm = bg.contiguous(), inst_img.contiguous(), _native.u8(inst_mask), num.to(torch.int32).contiguous()
    out = {"img": torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), "label": torch.empty(B, H, W, dtype=torch.uint8, device=dev),
           "place": torch.empty(B, N, 6, dtype=torch.int32, device=dev)}
    u = _native.upload(d[:, N_SAMPLE:N_SAMPLE + 2 * N], dev)
    _call("pvv_ct_compose", dev, b_.data_ptr(), ii.data_ptr(), im.data_ptr(), nm.data_ptr(), u.data_ptr(), B, H, W, N, h, w,
          out["img"].data_ptr(), out["label"].data_ptr(), out["place"].data_ptr())
    return out


def ct_augment(img, label, draws, *, train=True, input_size=(416, 512), down_ratio=4, scale_range=(0.6, 1.4), rot=0.0, boxes="linear",
               mean=MEAN, std=STD, eig_val=EIG_VAL, eig_vec=EIG_VEC, n_instances=None):
    """The reference's ``tless_utils.augment`` (:18-63) and ``Dataset.get_bbox`` (tless/ct.py:58-70) for a batch.
    :param img:         [B,H,W,3] uint8 CUDA tensor, channel 0 the blue one
    :param label:       [B,H,W] uint8: 0 background, i + 1 instance i; None: no boxes (the inference path)
    :param draws:       [B, >= 11] host float64 (``draws``), columns 0-9 are used; may be None with ``train=False``
    :param train:       False is ``augment(img, 'test')``: the centre is the image's, the scale ``max(H, W)``, the input size the
                        image's rounded up to multiples of 32, no colour step
    :param input_size:  (height, width) of the network's input with ``train=True``
    :param rot:         degrees, the same for the batch; non-zero is ``tless_train_utils.augment``'s rotation (cos and sin on the host)
    :param boxes:       'linear' (tless/ct.py:58-70: the float mask warped with INTER_LINEAR, != 0) or 'nearest' (tless_train/ct.py:75-76)
    :param mean, std, eig_val, eig_vec: taken as float32, as tless_config.py holds them
    :param n_instances: N of ``boxes``; by default what the width of ``draws`` implies
    :return: dict: ``inp`` [B,3,ih,iw] float32, ``orig_img`` [B,ih,iw,3] uint8 and, with a label, ``boxes`` [B,N,4] int32
             (x, y, x2, y2) on the output map, all on the device; ``center`` [B,2] float32, ``scale`` [B,2] float32,
             ``trans_input`` and ``trans_output`` [B,2,3] float64 as host tensors: they are functions of the draws alone."""
    import torch
    B, H, W = _check_img(img, "img")
    if boxes not in BOXES:
        raise ValueError("clean_pvnet_amd.ct_augment: boxes must be 'linear' or 'nearest', got %r" % (boxes,))
    if draws is None:
        if train:
            raise ValueError("clean_pvnet_amd.ct_augment: train=True needs draws")
        draws = np.zeros((B, N_SAMPLE))
    N = 0
    if label is not None:
        _native.need_cuda(label, "label", "ct_augment")
        if label.dtype != torch.uint8 or tuple(label.shape) != (B, H, W):
            raise TypeError("clean_pvnet_amd.ct_augment: label must be [%d, %d, %d] uint8, got %s %s" % (B, H, W, tuple(label.shape), label.dtype))
        N = (np.asarray(draws).shape[1] - N_SAMPLE) // 2 if n_instances is None else int(n_instances)
        if not 1 <= N <= MAX_N:
            raise ValueError("clean_pvnet_amd.ct_augment: n_instances must lie in [1, %d], got %d" % (MAX_N, N))
    d = _check_draws(draws, B, 0)
    if int(down_ratio) < 1 or not 0 < float(scale_range[0]) <= float(scale_range[1]):
        raise ValueError("clean_pvnet_amd.ct_augment: down_ratio must be >= 1 and scale_range (lo, hi) with 0 < lo <= hi")
    if train and not (int(down_ratio) <= int(input_size[0]) <= MAX_SIDE and int(down_ratio) <= int(input_size[1]) <= MAX_SIDE):
        raise ValueError("clean_pvnet_amd.ct_augment: input_size sides must lie in [down_ratio, %d], got %r" % (MAX_SIDE, tuple(input_size)))
    block, meta = host_block(d, H, W, train=bool(train), input_size=input_size, down_ratio=down_ratio, scale_range=[float(v) for v in scale_range],
                             rot=float(rot), eig_val=eig_val, eig_vec=eig_vec)
    ih, iw, oh, ow = meta["sizes"]
    if oh < 1 or ow < 1:
        raise ValueError("clean_pvnet_amd.ct_augment: down_ratio %d leaves no output map of a %d x %d input" % (down_ratio, ih, iw))
    mean_c, std_c = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    dev = img.device
    im = img.contiguous()
    lb = label.contiguous() if label is not None else None
    out = {"inp": torch.empty(B, 3, ih, iw, dtype=torch.float32, device=dev), "orig_img": torch.empty(B, ih, iw, 3, dtype=torch.uint8, device=dev)}
    if lb is not None:
        out["boxes"] = torch.empty(B, N, 4, dtype=torch.int32, device=dev)
    prm = _native.upload(block, dev)
    ws, _ = _lib.workspace("pvv_ct_augment_workspace_bytes", dev, B, N, ih, iw)
    _call("pvv_ct_augment", dev, im.data_ptr(), _native.ptr(lb), B, H, W, N, ih, iw, oh, ow, int(bool(train)), BOXES[boxes], prm.data_ptr(),
          mean_c, std_c, ws.data_ptr(), ws.numel(), out["orig_img"].data_ptr(), out["inp"].data_ptr(), _native.ptr(out.get("boxes")))
    for k in ("center", "scale", "trans_input", "trans_output"):
        out[k] = torch.from_numpy(meta[k])
    return out


class CtAugment:
    """The configuration of a detector loader: ``__call__(bg, inst_img, inst_mask, cls, num, draws=None)`` composes, augments and
    builds the targets, and returns the batch ``ct_train.NetworkWrapper`` consumes: ``inp``, ``ct_hm``, ``wh``, ``ct_cls``,
    ``ct_ind``, ``ct_01``, ``ct_num``, the ``boxes`` / ``cls`` / ``num`` they were made from and ``meta`` (``center``, ``scale``,
    ``ct_num``).  ``cls`` is [B,N] int32 or int64, the class of each instance."""

    def __init__(self, *, num_classes=30, train=True, input_size=(416, 512), down_ratio=4, scale_range=(0.6, 1.4), rot=0.0, boxes="linear",
                 mean=MEAN, std=STD, eig_val=EIG_VAL, eig_vec=EIG_VEC):
        self.num_classes = int(num_classes)
        self.kw = dict(train=bool(train), input_size=tuple(input_size), down_ratio=int(down_ratio), scale_range=tuple(scale_range), rot=float(rot),
                       boxes=boxes, mean=tuple(mean), std=tuple(std), eig_val=tuple(eig_val), eig_vec=tuple(tuple(r) for r in eig_vec))

    def __call__(self, bg, inst_img, inst_mask, cls, num, draws=None):
        from . import ct_train
        N = int(inst_img.shape[1])
        d = _draws(bg.shape[0], N) if draws is None else draws
        c = ct_compose(bg, inst_img, inst_mask, num, d)
        a = ct_augment(c["img"], c["label"], d, n_instances=N, **self.kw)
        oh, ow = a["inp"].shape[2] // self.kw["down_ratio"], a["inp"].shape[3] // self.kw["down_ratio"]
        ct_hm, wh, ct_cls, ct_ind, ct_01, ct_num = ct_train.ct_targets(a["boxes"], cls, num, self.num_classes, oh, ow)
        return {"inp": a["inp"], "ct_hm": ct_hm, "wh": wh, "ct_cls": ct_cls, "ct_ind": ct_ind, "ct_01": ct_01, "ct_num": ct_num,
                "boxes": a["boxes"], "cls": cls, "num": num, "meta": {"center": a["center"], "scale": a["scale"], "ct_num": ct_num}}
