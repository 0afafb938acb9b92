"""The T-LESS PVNet loader's training sample for a batch on the device (``libpvnet_vote.so``, the section "T-LESS PVNet
augmentation" of include/pvnet_vote.h).

The reference produces such a sample on a CPU core (lib/datasets/tless_train/pvnet.py): ``rotate_image`` turns a 400 x 400 cut-out
and its mask by a drawn angle (lib/utils/tless/tless_train_utils.py:153-172), ``cut_and_paste`` puts it on a 540 x 720 background
(tless_utils.py:86-97), ``get_fused_image`` builds a second canvas from six more rotated cut-outs (tless_train_utils.py:94-136), a
visibility ratio decides who occludes whom (pvnet.py:86-100), ``tless_pvnet_utils.augment`` crops to 256 x 256 around what is left
of the target, blanks everything outside a magnified box and runs ``color_aug`` (tless_pvnet_utils.py:21-73), and a float image
with an 18-channel vertex field is copied to the device.  Here the uint8 cut-outs and backgrounds go to the device once and
``tless_compose`` -> ``tless_pvnet_augment`` hand ``train.NetworkWrapper`` / ``train.pvnet_loss(kpt_2d=...)`` their batch on one
stream; ``rotate_image`` alone is what the detector's loader needs in front of ``ct_augment.ct_compose``.

The kernels hold no random number generator and evaluate no transcendental: ``draws`` returns a host table (``COLUMNS``, then
(rot, dst_y, dst_x) per distractor), and what depends only on the draws and the sizes -- ``getRotationMatrix2D``'s entries with
their cos and sin, the bounds of the rotated cut-outs, the inverse matrices, the drawn factors, the colour records -- is computed
here in binary64 and uploaded as one block per call.  What depends on pixels stays on the device: the rotated masks, their boxes
and sums, the placements, the visibility decision, the final box, ``scale`` / ``center`` / ``trans_input`` and the magnified box.
Each function equals its numpy twin (tests/tless_augment_twin.py) byte for byte; the control flow is the reference's own
(tests/golden/tless_augment_*.npz); parity of the resampling with OpenCV is unpinned.

``rotate_image``'s ``interp``: the reference calls ``cv2.warpAffine(mat, rotation_mat, (bound_w, bound_h), cv2.INTER_NEAREST)``, which
by OpenCV's Python signature (``warpAffine(src, M, dsize[, dst[, flags ...]])``) passes the constant as ``dst`` and leaves the flags
at their default: the warp is bilinear, the mask's too.  That reading is unverified (no OpenCV where this was built), so 'linear'
is the default and 'nearest' is offered.

Deviations: an empty rotated target mask gives ``path`` 3 (the target is skipped, the box is the whole canvas; the reference
raises); a distractor with an empty mask or beyond ``num[b]`` is skipped; a rotated cut-out larger than the canvas is placed at 0
and its outside dropped.  Not covered: the ``imgaug`` ``color_jitter`` and ``augmenters``, the background's ``cv2.resize``, image
decoding.  CUDA tensors in and out, the current stream, nothing read back, no state, no CPU fallback.
"""
import ctypes
import math

import numpy as np

from . import _native, ct_augment
from .ct_augment import EIG_VAL, EIG_VEC, MEAN, STD, colour_params, invert_affine

_lib = _native.bind("tless_augment", "libpvnet_vote.so", last_error="pvv_last_error")

# per sample, then (rot, dst_y, dst_x) per distractor.  Columns 3-9 lie where ct_augment.COLUMNS has them.
COLUMNS = ("scale", "box", "top", "order", "alpha_0", "alpha_1", "alpha_2", "normal_0", "normal_1", "normal_2", "rot", "dst_y", "dst_x", "black")
N_SAMPLE = len(COLUMNS)
PER_DISTRACTOR = 3
NORMAL_COLUMNS = ct_augment.NORMAL_COLUMNS
SCALE, BOX, TOP, ROT, DST_Y, DST_X, BLACK = 0, 1, 2, 10, 11, 12, 13
MAX_N, MAX_SIDE, MAX_BATCH = 16, 16384, 65535
INTERP = {"linear": 0, "nearest": 1}
TOP_BELOW, BLACK_FROM, OTHER_ROT = 0.5, 0.9, 360.0        # pvnet.py:93, tless_train_utils.py:95, :113

CUT = np.dtype([("M", "<f8", 6), ("inv", "<f8", 6), ("bh", "<i4"), ("bw", "<i4"), ("pad", "<i4", 2)])
assert CUT.itemsize == 112                                  # PVV_TLESS_CUT_BYTES
F32 = np.float32


def draws(B, N, generator=None):
    """The random numbers of a batch: a host float64 array [B, 14 + 3 N], one row per sample.  Columns 0-13 are ``COLUMNS``: the
    uniforms of the scale ratio and the box ratio, 'top' (the target goes on top iff u < 0.5), the colour columns of
    ``ct_augment.COLUMNS`` at their places (the order uniform, three alpha uniforms, three standard normals), the target's
    rotation (rot = u * rot_max), dst_y and dst_x, and 'black' (the fused background is black iff u >= 0.9); columns 14 + 3 n,
    15 + 3 n, 16 + 3 n are distractor n's rotation (u * 360), dst_y and dst_x.  Drawn from torch's CPU generator
    (``torch.manual_seed`` governs it) or from ``generator``."""
    import torch
    B, N = int(B), int(N)
    d = torch.rand(B, N_SAMPLE + PER_DISTRACTOR * N, dtype=torch.float64, generator=generator).numpy()
    d[:, list(NORMAL_COLUMNS)] = torch.randn(B, 3, dtype=torch.float64, generator=generator).numpy()
    return d


_draws = draws


def _check_draws(d, B, N):
    d = np.asarray(d)
    if d.dtype != np.float64 or d.ndim != 2 or d.shape[0] != B or d.shape[1] < N_SAMPLE + PER_DISTRACTOR * N:
        raise ValueError("clean_pvnet_amd.tless_augment: draws must be a host float64 array [%d, >= %d], got %s %s"
                         % (B, N_SAMPLE + PER_DISTRACTOR * N, d.shape, d.dtype))
    uni = np.delete(d, NORMAL_COLUMNS, axis=1)
    if not ((uni >= 0) & (uni < 1)).all() or not np.isfinite(d).all():
        raise ValueError("clean_pvnet_amd.tless_augment: the uniform draws must lie in [0, 1) and the normals be finite")
    return d


def rotate_side(h, w):
    """D(h, w) = floor(sqrt(h^2 + w^2)), the side of the plane a rotated h x w cut-out is stored in.  It bounds every
    ``bound_h`` / ``bound_w``: h |sin| + w |cos| <= sqrt(h^2 + w^2), the binary64 evaluation exceeds the exact value by less than
    2^-50 of it, and sqrt(h^2 + w^2), when no integer, lies at least 1 / (2 D + 2) below D + 1; when it is an integer -- h = 3 k,
    w = 4 k at atan(3 / 4) reaches it -- ``int`` of a value a few ulps above D is D."""
    return math.isqrt(int(h) * int(h) + int(w) * int(w))


def rotation(h, w, deg):
    """``rotate_image``'s host part (tless_train_utils.py:154-165) in the reference's order: (M, bound_h, bound_w), M the six
    entries of ``getRotationMatrix2D((w / 2, h / 2), deg, 1)`` shifted by ``bound / 2 - centre``."""
    cx, cy = w / 2, h / 2
    rad = float(deg) * (math.pi / 180)
    a, b = math.cos(rad), math.sin(rad)
    M = [a, b, (1. - a) * cx - b * cy, -b, a, b * cx + (1. - a) * cy]
    abs_cos, abs_sin = abs(M[0]), abs(M[1])
    bound_w, bound_h = int(h * abs_sin + w * abs_cos), int(h * abs_cos + w * abs_sin)
    M[2] += bound_w / 2 - cx
    M[5] += bound_h / 2 - cy
    return M, bound_h, bound_w


def cut_records(h, w, deg):
    """The records ``pvv_tless_rotate`` / ``pvv_tless_compose`` read for cut-outs of h x w turned by ``deg`` (any shape): a ``CUT``
    array of that shape."""
    deg = np.asarray(deg, np.float64)
    rec = np.zeros(deg.shape, CUT)
    D = rotate_side(h, w)
    for i in np.ndindex(deg.shape):
        M, bh, bw = rotation(h, w, deg[i])
        if not (0 <= bh <= D and 0 <= bw <= D):
            raise AssertionError("clean_pvnet_amd.tless_augment: bound %d x %d exceeds D = %d" % (bh, bw, D))
        rec["M"][i], rec["inv"][i], rec["bh"][i], rec["bw"][i] = M, invert_affine([M[:3], M[3:]]), bh, bw
    return rec


def _call(symbol, dev, *args):
    _lib.call(symbol, dev, *args)


def _interp(interp):
    if interp not in INTERP:
        raise ValueError("clean_pvnet_amd.tless_augment: interp must be 'linear' or 'nearest', got %r" % (interp,))
    return INTERP[interp]


def _sides(what, *sides):
    if not all(1 <= int(s) <= MAX_SIDE for s in sides):
        raise ValueError("clean_pvnet_amd.tless_augment: the sides of %s must lie in [1, %d], got %s" % (what, MAX_SIDE, sides))


def _check_img(img, what):
    B, H, W = _native.check_images(img, what, "tless_augment")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError("clean_pvnet_amd.tless_augment: B must lie in [1, %d], got %d" % (MAX_BATCH, B))
    _sides(what, H, W)
    return B, H, W


def rotate_image(img, deg, interp="linear"):
    """The reference's ``rotate_image`` (tless_train_utils.py:153-172) for any number of cut-outs.
    :param img:    [..,h,w,3] or [..,h,w] uint8 (or bool, [..,h,w]) CUDA tensor
    :param deg:    host array [..] of degrees: its shape tells the leading dimensions
    :param interp: 'linear' (what the reference's call does, see the module's text) or 'nearest'
    :return: dict: ``out`` [..,D,D,3] or [..,D,D] uint8 on the device, D = ``rotate_side(h, w)``: the rotated cut-out in its
             top-left ``bound_h`` x ``bound_w`` corner, zero elsewhere; ``size`` [..,2] int32 (bound_h, bound_w) and ``rot`` [..,2,3]
             float64, the matrix, as host tensors: they are functions of the angles alone."""
    import torch
    _native.need_cuda(img, "img", "tless_augment")
    nearest = _interp(interp)
    deg = np.asarray(deg, np.float64)
    lead = deg.shape
    rest = tuple(int(v) for v in img.shape[len(lead):])
    if img.dtype not in (torch.uint8, torch.bool) or tuple(img.shape[:len(lead)]) != lead or len(rest) not in (2, 3) or (len(rest) == 3 and rest[2] != 3):
        raise TypeError("clean_pvnet_amd.tless_augment: img must be %s + [h,w] or [h,w,3] uint8 or bool, got %s %s" % (list(lead), tuple(img.shape), img.dtype))
    if not np.isfinite(deg).all():
        raise ValueError("clean_pvnet_amd.tless_augment: deg must be finite")
    h, w = rest[:2]
    _sides("img", h, w)
    P = int(np.prod(lead, dtype=np.int64))
    if not 1 <= P <= MAX_BATCH:
        raise ValueError("clean_pvnet_amd.tless_augment: the number of cut-outs must lie in [1, %d], got %d" % (MAX_BATCH, P))
    channels = 3 if len(rest) == 3 else 1
    rec = cut_records(h, w, deg)
    D = rotate_side(h, w)
    dev = img.device
    src = _native.u8(img)
    out = torch.empty(lead + ((D, D, 3) if channels == 3 else (D, D)), dtype=torch.uint8, device=dev)
    block, (cuts,) = _native.upload_parts([rec], dev)
    _call("pvv_tless_rotate", dev, src.data_ptr(), cuts, P, h, w, channels, D, nearest, out.data_ptr())
    size = np.stack([rec["bh"], rec["bw"]], axis=-1).astype(np.int32)
    return {"out": out, "size": torch.from_numpy(size), "rot": torch.from_numpy(rec["M"].reshape(lead + (2, 3)).copy())}


def tless_compose(bg, img, mask, kpt_2d, other_img, other_mask, draws, fused_bg=None, num=None, rot_max=360., ratio=0.8, interp="linear"):
    """The reference's ``read_data`` rotation and ``get_training_img`` (lib/datasets/tless_train/pvnet.py:60-69, 73-105) for a batch.
    :param bg:         [B,H,W,3] uint8 CUDA tensor, the backgrounds at the canvas' size
    :param img, mask:  [B,h,w,3] uint8 and [B,h,w] uint8 or bool: the target's cut-out; a 'real' mask may hold 255
    :param kpt_2d:     [B,K,2] float32 or float64, (x, y) in the cut-out
    :param other_img, other_mask: [B,N,h',w',3] uint8 and [B,N,h',w'] uint8 or bool, the distractors; N <= 16
    :param draws:      [B, >= 14 + 3 N] host float64 (``draws``)
    :param fused_bg:   [B,H,W,3] uint8, the fused canvas' own background; None: ``bg``
    :param num:        [B] int32 or int64: the first ``num[b]`` distractors are used; None: all
    :param rot_max:    the target's rotation is u * rot_max degrees (cfg.tless.rot): a float or a host array [B]; the caller passes
                       0 for the samples ``get_rot`` (pvnet.py:20-30) leaves unrotated
    :param ratio:      cfg.tless.ratio, > 0: the occluded form is kept iff visible / pixel_num >= ratio
    :return: dict on the device: ``img`` [B,H,W,3] uint8, ``mask`` [B,H,W] uint8 (0 / 1), ``kpt_2d`` [B,K,2] float64, ``bbox`` [B,4]
             int32 (x, y, x + w - 1, y + h - 1 of the mask), ``path`` [B] int32 (0 on top by draw, 1 occluded and kept, 2 put on top by
             the ratio, 3 no target), ``place`` [B,1+N,6] int32 (y_min, x_min, h, w, dst_y, dst_x; the target first; a skipped cut-out
             is (0, 0, -1, -1, 0, 0)) and ``visible`` [B,2] int64 (the target's pixels no distractor covers, pixel_num)."""
    import torch
    B, H, W = _check_img(bg, "bg")
    nearest = _interp(interp)
    named = [("img", img), ("mask", mask), ("kpt_2d", kpt_2d), ("other_img", other_img), ("other_mask", other_mask)]
    named += [(k, t) for k, t in (("fused_bg", fused_bg), ("num", num)) if t is not None]
    for what, t in named:
        _native.need_cuda(t, what, "tless_augment")
    if not float(ratio) > 0:
        raise ValueError("clean_pvnet_amd.tless_augment: ratio must be > 0, got %r" % (ratio,))
    if img.dtype != torch.uint8 or other_img.dtype != torch.uint8 or mask.dtype not in (torch.uint8, torch.bool) or \
            other_mask.dtype not in (torch.uint8, torch.bool) or kpt_2d.dtype not in (torch.float32, torch.float64):
        raise TypeError("clean_pvnet_amd.tless_augment: img and other_img must be uint8, mask and other_mask uint8 or bool, kpt_2d float32 or "
                        "float64, got %s, %s, %s, %s, %s" % (img.dtype, other_img.dtype, mask.dtype, other_mask.dtype, kpt_2d.dtype))
    if img.dim() != 4 or img.shape[0] != B or img.shape[3] != 3 or tuple(mask.shape) != tuple(img.shape[:3]):
        raise ValueError("clean_pvnet_amd.tless_augment: img must be [B = %d, h, w, 3] and mask [B, h, w], got %s and %s" % (B, tuple(img.shape), tuple(mask.shape)))
    if other_img.dim() != 5 or other_img.shape[0] != B or other_img.shape[4] != 3 or tuple(other_mask.shape) != tuple(other_img.shape[:4]):
        raise ValueError("clean_pvnet_amd.tless_augment: other_img must be [B = %d, N, h, w, 3] and other_mask [B, N, h, w], got %s and %s"
                         % (B, tuple(other_img.shape), tuple(other_mask.shape)))
    if kpt_2d.dim() != 3 or kpt_2d.shape[0] != B or kpt_2d.shape[2] != 2 or kpt_2d.shape[1] > 65535:
        raise ValueError("clean_pvnet_amd.tless_augment: kpt_2d must be [B = %d, K <= 65535, 2], got %s" % (B, tuple(kpt_2d.shape)))
    ht, wt = (int(v) for v in img.shape[1:3])
    N, ho, wo = (int(v) for v in other_img.shape[1:4])
    K = int(kpt_2d.shape[1])
    if not 0 <= N <= MAX_N:
        raise ValueError("clean_pvnet_amd.tless_augment: N must lie in [0, %d], got %d" % (MAX_N, N))
    _sides("img", ht, wt)
    if N:
        _sides("other_img", ho, wo)
    if fused_bg is not None and (fused_bg.dtype != torch.uint8 or tuple(fused_bg.shape) != (B, H, W, 3)):
        raise TypeError("clean_pvnet_amd.tless_augment: fused_bg must be [%d, %d, %d, 3] uint8, got %s %s" % (B, H, W, tuple(fused_bg.shape), fused_bg.dtype))
    if num is not None and (num.dtype not in (torch.int32, torch.int64) or tuple(num.shape) != (B,)):
        raise TypeError("clean_pvnet_amd.tless_augment: num must be [B = %d] int32 or int64, got %s %s" % (B, tuple(num.shape), num.dtype))
    rot_max = np.asarray(rot_max, np.float64)
    if rot_max.shape not in ((), (B,)) or not np.isfinite(rot_max).all():
        raise ValueError("clean_pvnet_amd.tless_augment: rot_max must be a finite float or a host array [B = %d]" % B)
    rot_max = np.broadcast_to(rot_max, (B,))
    d = _check_draws(draws, B, N)
    cuts, u, flags = host_block(d, N, ht, wt, ho, wo, rot_max)
    dev = bg.device
    keep = [bg.contiguous(), img.contiguous(), _native.u8(mask), kpt_2d.to(torch.float64).contiguous(), other_img.contiguous(), _native.u8(other_mask),
            None if fused_bg is None else fused_bg.contiguous(), None if num is None else num.to(torch.int32).contiguous()]
    out = {"img": torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), "mask": torch.empty(B, H, W, dtype=torch.uint8, device=dev),
           "kpt_2d": torch.empty(B, K, 2, dtype=torch.float64, device=dev), "bbox": torch.empty(B, 4, dtype=torch.int32, device=dev),
           "path": torch.empty(B, dtype=torch.int32, device=dev), "place": torch.empty(B, 1 + N, 6, dtype=torch.int32, device=dev),
           "visible": torch.empty(B, 2, dtype=torch.int64, device=dev)}
    block, (p_cuts, p_u, p_flags) = _native.upload_parts([cuts, u, flags], dev)
    ws, _ = _lib.workspace("pvv_tless_compose_workspace_bytes", dev, B, N, H, W, ht, wt, ho, wo)
    _call("pvv_tless_compose", dev, keep[0].data_ptr(), _native.ptr(keep[6]), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
          keep[4].data_ptr(), keep[5].data_ptr(), _native.ptr(keep[7]), p_cuts, p_u, p_flags, B, H, W, N, K, ht, wt, ho, wo, nearest, float(ratio),
          ws.data_ptr(), ws.numel(), out["img"].data_ptr(), out["mask"].data_ptr(), out["kpt_2d"].data_ptr(), out["bbox"].data_ptr(),
          out["path"].data_ptr(), out["place"].data_ptr(), out["visible"].data_ptr())
    return out


def host_block(d, N, ht, wt, ho, wo, rot_max):
    """What ``tless_compose`` derives from the draws and the sizes: the cut-outs' records [B,1+N] (``CUT``, the target first), the
    placement uniforms [B,1+N,2] (dst_y, dst_x) and the flags [B,2] int32 (on top by draw, black fused background)."""
    B = len(d)
    deg = np.zeros((B, 1 + N))
    u = np.zeros((B, 1 + N, 2))
    deg[:, 0], u[:, 0, 0], u[:, 0, 1] = d[:, ROT] * rot_max, d[:, DST_Y], d[:, DST_X]
    for n in range(N):
        c = N_SAMPLE + PER_DISTRACTOR * n
        deg[:, 1 + n], u[:, 1 + n, 0], u[:, 1 + n, 1] = d[:, c] * OTHER_ROT, d[:, c + 1], d[:, c + 2]
    cuts = np.zeros((B, 1 + N), CUT)
    cuts[:, :1] = cut_records(ht, wt, deg[:, :1])
    if N:
        cuts[:, 1:] = cut_records(ho, wo, deg[:, 1:])
    flags = np.stack([d[:, TOP] < TOP_BELOW, d[:, BLACK] >= BLACK_FROM], axis=1).astype(np.int32)
    return cuts, u, flags


def ratios(d, scale_train_ratio, box_train_ratio):
    """(factor [B] float32, box_ratio [B] float64): ``np.random.uniform(lo, hi)`` of tless_pvnet_utils.py:31 and :54; the first
    multiplies a float32 array, so numpy rounds it to float32."""
    lo, hi = (float(v) for v in scale_train_ratio)
    factor = np.array([F32(lo + (hi - lo) * float(v)) for v in d[:, SCALE]], F32)
    lo, hi = (float(v) for v in box_train_ratio)
    return factor, np.array([lo + (hi - lo) * float(v) for v in d[:, BOX]], np.float64)


def tless_pvnet_augment(img, mask, kpt_2d, bbox, draws, input_size=(256, 256), scale_train_ratio=(1.8, 2.4), box_train_ratio=(1.0, 1.2), train=True,
                        mean=MEAN, std=STD, eig_val=EIG_VAL, eig_vec=EIG_VEC):
    """The reference's ``tless_pvnet_utils.augment(img, bbox, 'train')`` (:21-73) with the mask's warp and the keypoints' map of
    ``Dataset.__getitem__`` (tless_train/pvnet.py:115-116) for a batch.
    :param img:     [B,H,W,3] uint8 CUDA tensor, channel 0 the blue one
    :param mask:    [B,H,W] uint8 or bool
    :param kpt_2d:  [B,K,2] float32 or float64
    :param bbox:    [B,4] int32 on the device, (x0, y0, x1, y1) inclusive (``tless_compose``'s ``bbox``)
    :param draws:   [B, >= 14] host float64 (``draws``): the columns scale, box and the colour ones are used
    :param input_size: (height, width), cfg.tless.pvnet_input_scale reversed
    :param train:   False leaves the colour steps out; the geometry is the same
    :return: dict on the device: ``inp`` [B,3,ih,iw] float32, ``orig_img`` [B,ih,iw,3] uint8, ``mask`` [B,ih,iw] uint8, ``kpt_2d``
             [B,K,2] float64, ``trans_input`` [B,2,3] float64, ``center`` [B,2] float64, ``scale`` [B,2] float32 and ``box`` [B,4] int32,
             the rectangle ``magnify_box`` keeps (x0, y0, x1, y1)."""
    import torch
    B, H, W = _check_img(img, "img")
    for what, t in (("mask", mask), ("kpt_2d", kpt_2d), ("bbox", bbox)):
        _native.need_cuda(t, what, "tless_augment")
    if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != (B, H, W):
        raise TypeError("clean_pvnet_amd.tless_augment: mask must be [%d, %d, %d] uint8 or bool, got %s %s" % (B, H, W, tuple(mask.shape), mask.dtype))
    if kpt_2d.dtype not in (torch.float32, torch.float64) or kpt_2d.dim() != 3 or kpt_2d.shape[0] != B or kpt_2d.shape[2] != 2 or kpt_2d.shape[1] > 65535:
        raise TypeError("clean_pvnet_amd.tless_augment: kpt_2d must be [B = %d, K <= 65535, 2] float32 or float64, got %s %s" % (B, tuple(kpt_2d.shape), kpt_2d.dtype))
    if bbox.dtype != torch.int32 or tuple(bbox.shape) != (B, 4):
        raise TypeError("clean_pvnet_amd.tless_augment: bbox must be [B = %d, 4] int32, got %s %s" % (B, tuple(bbox.shape), bbox.dtype))
    ih, iw = int(input_size[0]), int(input_size[1])
    _sides("input_size", ih, iw)
    for what, r in (("scale_train_ratio", scale_train_ratio), ("box_train_ratio", box_train_ratio)):
        if not 0 < float(r[0]) <= float(r[1]) or not math.isfinite(float(r[1])):
            raise ValueError("clean_pvnet_amd.tless_augment: %s must be (lo, hi) with 0 < lo <= hi" % what)
    d = _check_draws(draws, B, 0)
    factor, box_ratio = ratios(d, scale_train_ratio, box_train_ratio)
    colour = np.zeros(B, ct_augment.PARAM)
    if train:
        for b in range(B):
            colour["order"][b], colour["a"][b], colour["oma"][b], colour["light"][b] = colour_params(d[b], eig_val, eig_vec)
    K = int(kpt_2d.shape[1])
    dev = img.device
    keep = [img.contiguous(), _native.u8(mask), kpt_2d.to(torch.float64).contiguous(), bbox.contiguous()]
    out = {"inp": torch.empty(B, 3, ih, iw, dtype=torch.float32, device=dev), "orig_img": torch.empty(B, ih, iw, 3, dtype=torch.uint8, device=dev),
           "mask": torch.empty(B, ih, iw, dtype=torch.uint8, device=dev), "kpt_2d": torch.empty(B, K, 2, dtype=torch.float64, device=dev),
           "trans_input": torch.empty(B, 2, 3, dtype=torch.float64, device=dev), "center": torch.empty(B, 2, dtype=torch.float64, device=dev),
           "scale": torch.empty(B, 2, dtype=torch.float32, device=dev), "box": torch.empty(B, 4, dtype=torch.int32, device=dev)}
    block, (p_colour, p_ratio, p_factor) = _native.upload_parts([colour, box_ratio, factor], dev)
    mean_c, std_c = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    ws, _ = _lib.workspace("pvv_tless_augment_workspace_bytes", dev, B, ih, iw)
    _call("pvv_tless_augment", dev, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), B, H, W, K, ih, iw, int(bool(train)),
          p_factor, p_ratio, p_colour, mean_c, std_c, ws.data_ptr(), ws.numel(), out["orig_img"].data_ptr(), out["inp"].data_ptr(),
          out["mask"].data_ptr(), out["kpt_2d"].data_ptr(), out["trans_input"].data_ptr(), out["center"].data_ptr(), out["scale"].data_ptr(),
          out["box"].data_ptr())
    return out


class TlessPVNetAugment:
    """The configuration of a T-LESS PVNet loader: ``__call__(bg, img, mask, kpt_2d, other_img, other_mask, draws=None, fused_bg=None,
    num=None, rot_max=None)`` composes and augments, and returns ``{'inp', 'mask', 'kpt_2d', 'meta'}``, what ``train.NetworkWrapper`` /
    ``train.pvnet_loss(kpt_2d=...)`` take."""

    def __init__(self, *, rot_max=360., ratio=0.8, interp="linear", input_size=(256, 256), scale_train_ratio=(1.8, 2.4), box_train_ratio=(1.0, 1.2),
                 train=True, mean=MEAN, std=STD, eig_val=EIG_VAL, eig_vec=EIG_VEC):
        self.compose_kw = dict(rot_max=rot_max, ratio=float(ratio), interp=interp)
        self.augment_kw = dict(input_size=tuple(input_size), scale_train_ratio=tuple(scale_train_ratio), box_train_ratio=tuple(box_train_ratio),
                               train=bool(train), mean=tuple(mean), std=tuple(std), eig_val=tuple(eig_val), eig_vec=tuple(tuple(r) for r in eig_vec))

    def __call__(self, bg, img, mask, kpt_2d, other_img, other_mask, draws=None, fused_bg=None, num=None, rot_max=None):
        d = _draws(bg.shape[0], other_img.shape[1]) if draws is None else draws
        kw = dict(self.compose_kw) if rot_max is None else dict(self.compose_kw, rot_max=rot_max)
        c = tless_compose(bg, img, mask, kpt_2d, other_img, other_mask, d, fused_bg=fused_bg, num=num, **kw)
        a = tless_pvnet_augment(c["img"], c["mask"], c["kpt_2d"], c["bbox"], d, **self.augment_kw)
        return {"inp": a["inp"], "mask": a["mask"], "kpt_2d": a["kpt_2d"], "meta": {}}
