"""PVNet's training augmentation and loader transforms for a batch on the device (``libpvnet_vote.so``, the section
"Training augmentation" of include/pvnet_vote.h).

The reference produces ``inp``, ``mask`` and ``kpt_2d`` per sample on a CPU core: ``rotate_instance`` (two ``cv2.warpAffine``
over the full image), ``crop_resize_instance_v1`` (a crop or pad, two ``cv2.resize``) -- lib/datasets/linemod/pvnet.py:62-78,
lib/datasets/augmentation.py -- then ``RandomBlur``, ``ColorJitter``, ``ToTensor`` and ``Normalize``
(lib/datasets/transforms.py:81-90), and copies a float32 image to the device.  Here the uint8 images as decoded go to the
device once and ``pvnet_augment`` -> ``pvnet_transform`` hand ``train.pvnet_loss(kpt_2d=...)`` its tensors on one stream.

The kernels hold no random number generator: ``draws`` returns a host table of uniforms and every random decision is a
stated function of one column (``COLUMNS``).  The host turns the data-independent columns into a small block per sample --
``math.cos`` / ``math.sin`` of the degree included, so that no transcendental is evaluated on the device -- and uploads it with
one non-blocking copy; the centroid, the box, the window and the contrast mean are computed on the device.  Each function
equals its numpy twin (tests/augment_twin.py) byte for byte; the control flow, the windows, the keypoints and the
normalisation are the reference's own (tests/golden/augment_*.npz), the colour jitter is PIL's; parity of the resampling and
the blur with OpenCV is unpinned.  Two deviations: a ``randint(lo, hi)`` with ``hi <= lo`` gives ``lo``
and a rotated mask that came out empty takes the no-foreground steps, where the reference raises.  CUDA tensors in and out,
the current stream, nothing read back, no state, no CPU fallback.
"""
import ctypes
import itertools
import math

import numpy as np

from . import _native

_lib = _native.bind("augment", "libpvnet_vote.so", last_error="pvv_last_error")

N_DRAWS = 12
COLUMNS = ("degree", "ratio", "hbeg", "wbeg", "blur", "blur_size", "brightness", "contrast", "saturation", "hue", "order", "unused")
MIN_SIDE, MAX_SIDE, MAX_BATCH = 8, 16384, 65535
BLUR_SIZES = (3, 5, 7, 9)
BLUR_TAPS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}
BLUR_SIGMA_9 = 1.7
ORDERS = tuple(itertools.permutations(range(4)))     # of (brightness, contrast, saturation, hue), lexicographic
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)     # transforms.py:88

GEOMETRY = np.dtype([("cos", "<f8"), ("sin", "<f8"), ("ratio", "<f8"), ("u_h", "<f8"), ("u_w", "<f8"), ("th", "<i4"), ("tw", "<i4")])
JITTER = np.dtype([("k", "<i4"), ("w", "<i4", 9), ("f", "<f4", 3), ("hue", "<i4"), ("order", "<i4", 4)])
assert GEOMETRY.itemsize == 48 and JITTER.itemsize == 72       # PVV_AUGMENT_PARAM_BYTES, PVV_TRANSFORM_PARAM_BYTES


def draws(B, generator=None):
    """The uniforms of a batch: a host float64 array [B, 12] in [0, 1), one row per sample, one column per decision
    (``COLUMNS``).  Drawn from torch's CPU generator (``torch.manual_seed`` governs it) or from ``generator``."""
    import torch
    return torch.rand(int(B), N_DRAWS, dtype=torch.float64, generator=generator).numpy()


_draws = draws                     # (``draws`` is also the name of an argument below)


def _check_draws(d, B):
    d = np.asarray(d)
    if d.dtype != np.float64 or d.shape != (B, N_DRAWS):
        raise ValueError("clean_pvnet_amd.augment: draws must be a host float64 array [%d, %d], got %s %s" % (B, N_DRAWS, d.shape, d.dtype))
    if not ((d >= 0) & (d < 1)).all():
        raise ValueError("clean_pvnet_amd.augment: draws must lie in [0, 1)")
    return d


def blur_taps(k):
    """The 9-entry table of the blur of size ``k``, centred on entry 4, summing to 256."""
    if k == 9:
        g = [math.exp(-((i - 4) * (i - 4)) / (2 * BLUR_SIGMA_9 * BLUR_SIGMA_9)) for i in range(9)]
        total = sum(g)
        taps = [int(round(256 * (v / total))) for v in g]
        taps[4] += 256 - sum(taps)
    else:
        taps = list(BLUR_TAPS[k])
    pad = (9 - len(taps)) // 2
    return [0] * pad + taps + [0] * pad


def geometry_params(d, out_size, rotate, resize_ratio):
    """Columns 0-3 as the block ``pvv_pvnet_augment`` reads."""
    height, width = out_size
    out = np.zeros(len(d), GEOMETRY)
    for b, u in enumerate(d):
        deg = rotate[0] + (rotate[1] - rotate[0]) * float(u[0])
        ratio = resize_ratio[0] + (resize_ratio[1] - resize_ratio[0]) * float(u[1])
        th, tw = int(height * ratio), int(width * ratio)
        if not (1 <= th <= MAX_SIDE and 1 <= tw <= MAX_SIDE):
            raise ValueError("clean_pvnet_amd.augment: resize ratio %r gives a window of %d x %d" % (ratio, th, tw))
        rad = deg * (math.pi / 180)
        out[b] = (math.cos(rad), math.sin(rad), ratio, float(u[2]), float(u[3]), th, tw)
    return out


def jitter_params(d, blur_prob, jitter):
    """Columns 4-10 as the block ``pvv_pvnet_transform`` reads.  A step whose amplitude is 0 is not applied."""
    lo = [max(0.0, 1 - jitter[0]), max(0.0, 1 - jitter[1]), max(0.0, 1 - jitter[2]), -jitter[3]]
    hi = [1 + jitter[0], 1 + jitter[1], 1 + jitter[2], jitter[3]]
    out = np.zeros(len(d), JITTER)
    for b, u in enumerate(d):
        k = BLUR_SIZES[min(int(math.floor(4 * float(u[5]))), 3)] if float(u[4]) < blur_prob else 0
        f = [lo[i] + (hi[i] - lo[i]) * float(u[6 + i]) for i in range(4)]
        order = ORDERS[min(int(math.floor(24 * float(u[10]))), 23)]
        out[b] = (k, blur_taps(k) if k else [0] * 9, f[:3], int(f[3] * 255) & 255, [op if jitter[op] != 0 else -1 for op in order])
    return out


def _call(symbol, dev, *args):
    _lib.call(symbol, dev, *args)


def pvnet_augment(img, mask, kpt_2d, out_size, draws, *, rotate=(-30, 30), overlap_ratio=0.8, resize_ratio=(0.8, 1.2)):
    """The reference's ``augment`` (linemod/pvnet.py:62-78) for a batch.
    :param img:      [B,H,W,3] uint8 CUDA tensor
    :param mask:     [B,H,W] uint8 or bool; foreground is ``mask != 0``
    :param kpt_2d:   [B,K,2] float32 or float64, (x, y)
    :param out_size: (height, width), the same for the batch
    :param draws:    [B,12] host float64 in [0, 1) (``draws``); columns 0-3 are used
    :return: dict: ``img`` [B,height,width,3] uint8, ``mask`` [B,height,width] uint8, ``kpt_2d`` [B,K,2] float64, ``path`` [B]
             int32 (0 no foreground, 1 the instance branch, 2 the rotated mask came out empty: the steps of 0 on the
             unrotated image) and ``window`` [B,6] int32 (th, tw, hbeg, wbeg, pad_h, pad_w)."""
    import torch
    B, H, W = _native.check_images(img, "img", "augment", MAX_BATCH, MAX_SIDE)
    _native.need_cuda(mask, "mask", "augment")
    _native.need_cuda(kpt_2d, "kpt_2d", "augment")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError("clean_pvnet_amd.augment: mask must be uint8 or bool, got %s" % mask.dtype)
    if kpt_2d.dtype not in (torch.float32, torch.float64):
        raise TypeError("clean_pvnet_amd.augment: kpt_2d must be float32 or float64, got %s" % kpt_2d.dtype)
    if tuple(mask.shape) != (B, H, W):
        raise ValueError("clean_pvnet_amd.augment: mask must be [%d, %d, %d], got %s" % (B, H, W, tuple(mask.shape)))
    if kpt_2d.dim() != 3 or kpt_2d.shape[0] != B or kpt_2d.shape[2] != 2 or kpt_2d.shape[1] > 65535:
        raise ValueError("clean_pvnet_amd.augment: kpt_2d must be [B = %d, K <= 65535, 2], got %s" % (B, tuple(kpt_2d.shape)))
    height, width = (int(v) for v in out_size)
    if not (MIN_SIDE <= height <= MAX_SIDE and MIN_SIDE <= width <= MAX_SIDE):
        raise ValueError("clean_pvnet_amd.augment: out_size sides must lie in [%d, %d], got %s" % (MIN_SIDE, MAX_SIDE, (height, width)))
    if not 0 <= float(overlap_ratio) <= 1:
        raise ValueError("clean_pvnet_amd.augment: overlap_ratio must lie in [0, 1], got %r" % (overlap_ratio,))
    if not (0 < resize_ratio[0] <= resize_ratio[1]) or not rotate[0] <= rotate[1]:
        raise ValueError("clean_pvnet_amd.augment: rotate and resize_ratio must be (lo, hi) with lo <= hi, the ratio positive")
    block = geometry_params(_check_draws(draws, B), (height, width), [float(v) for v in rotate], [float(v) for v in resize_ratio])
    dev = img.device
    K = int(kpt_2d.shape[1])
    im, kp = img.contiguous(), kpt_2d.detach().contiguous()
    m = _native.u8(mask)
    out = {"img": torch.empty(B, height, width, 3, dtype=torch.uint8, device=dev),
           "mask": torch.empty(B, height, width, dtype=torch.uint8, device=dev),
           "kpt_2d": torch.empty(B, K, 2, dtype=torch.float64, device=dev),
           "path": torch.empty(B, dtype=torch.int32, device=dev), "window": torch.empty(B, 6, dtype=torch.int32, device=dev)}
    prm = _native.upload(block, dev)
    mth, mtw = int(block["th"].max()), int(block["tw"].max())                    # the rotated windows lie in the workspace
    ws, _ = _lib.workspace("pvv_augment_workspace_bytes", dev, B, mth, mtw)
    _call("pvv_pvnet_augment", dev, im.data_ptr(), m.data_ptr(), kp.data_ptr() if K else None, int(kp.dtype == torch.float64), B, H, W, K,
          height, width, float(overlap_ratio), prm.data_ptr(), mth, mtw, ws.data_ptr(), ws.numel(), out["img"].data_ptr(), out["mask"].data_ptr(),
          out["kpt_2d"].data_ptr() if K else None, out["path"].data_ptr(), out["window"].data_ptr())
    return out


def pvnet_transform(img, draws, *, blur_prob=0.5, jitter=(0.1, 0.1, 0.05, 0.05), mean, std):
    """``make_transforms(cfg, True)`` (transforms.py:81-90) for a batch: the blur, the colour jitter, ``ToTensor``, ``Normalize``.
    :param img:        [B,h,w,3] uint8 CUDA tensor, sides >= 8
    :param draws:      [B,12] host float64 in [0, 1) (``draws``), columns 4-10 are used; None for ``make_transforms(cfg, False)``:
                       ``ToTensor`` and ``Normalize`` only
    :param blur_prob:  ``RandomBlur``'s probability
    :param jitter:     the amplitudes of brightness, contrast, saturation and hue (the hue's at most 0.5); a step whose amplitude
                       is 0 is not applied, as in torchvision
    :param mean, std:  3 floats each, taken as binary64
    :return:           [B,3,h,w] float32"""
    import torch
    B, h, w = _native.check_images(img, "img", "augment", MAX_BATCH, MAX_SIDE)
    mean_c, std_c = (ctypes.c_double * 3)(*[float(v) for v in mean]), (ctypes.c_double * 3)(*[float(v) for v in std])
    dev = img.device
    prm, ws, has_blur, has_contrast = None, None, 0, 0
    if draws is not None:
        jitter = [float(v) for v in jitter]
        if len(jitter) != 4 or min(jitter) < 0 or jitter[3] > 0.5:
            raise ValueError("clean_pvnet_amd.augment: jitter must be four amplitudes >= 0, the hue's <= 0.5, got %r" % (jitter,))
        if not 0 <= float(blur_prob) <= 1:
            raise ValueError("clean_pvnet_amd.augment: blur_prob must lie in [0, 1], got %r" % (blur_prob,))
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError("clean_pvnet_amd.augment: the image's sides must be at least %d, got %d x %d" % (MIN_SIDE, h, w))
        block = jitter_params(_check_draws(draws, B), float(blur_prob), jitter)
        has_blur, has_contrast = int((block["k"] > 0).any()), int((block["order"] == 1).any())
        prm = _native.upload(block, dev)
        ws, _ = _lib.workspace("pvv_transform_workspace_bytes", dev, B, h, w)
    im = img.contiguous()
    out = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
    _call("pvv_pvnet_transform", dev, im.data_ptr(), B, h, w, _native.ptr(prm), has_blur, has_contrast, mean_c, std_c, _native.ptr(ws),
          ws.numel() if ws is not None else 0, out.data_ptr())
    return out


class PVNetAugment:
    """The configuration of a loader's augmentation: ``__call__(img, mask, kpt_2d, height, width, draws=None)`` returns
    ``{'inp', 'mask', 'kpt_2d'}``, ready for ``train.NetworkWrapper`` / ``train.pvnet_loss(kpt_2d=...)``.  With ``train=False``
    only ``ToTensor`` and ``Normalize`` are applied, as the reference's test split does."""

    def __init__(self, *, train=True, rotate=(-30, 30), overlap_ratio=0.8, resize_ratio=(0.8, 1.2), blur_prob=0.5,
                 jitter=(0.1, 0.1, 0.05, 0.05), mean=MEAN, std=STD):
        self.train, self.rotate, self.overlap_ratio, self.resize_ratio = bool(train), tuple(rotate), overlap_ratio, tuple(resize_ratio)
        self.blur_prob, self.jitter, self.mean, self.std = blur_prob, tuple(jitter), tuple(mean), tuple(std)

    def __call__(self, img, mask, kpt_2d, height, width, draws=None):
        if not self.train:
            return {"inp": pvnet_transform(img, None, mean=self.mean, std=self.std), "mask": mask, "kpt_2d": kpt_2d}
        d = _draws(img.shape[0]) if draws is None else draws
        g = pvnet_augment(img, mask, kpt_2d, (height, width), d, rotate=self.rotate, overlap_ratio=self.overlap_ratio,
                          resize_ratio=self.resize_ratio)
        inp = pvnet_transform(g["img"], d, blur_prob=self.blur_prob, jitter=self.jitter, mean=self.mean, std=self.std)
        return {"inp": inp, "mask": g["mask"], "kpt_2d": g["kpt_2d"]}
