"""The numpy twin of clean_pvnet_amd.augment: the contract of DESIGN.md section 18, stage by stage, that the device is held to
byte for byte (tests/test_gpu_augment.py) and that tests/test_augment.py pins to the reference's own control flow
(tests/golden/augment_*.npz), to PIL's ``ImageEnhance`` and to plain binary64 samplers.

numpy evaluates each binary64 / float32 operation below once, in the order written, as the kernels do under
``-ffp-contract=off``.  ``math.cos`` / ``math.sin`` are taken on the host exactly as the product's host side takes them.  The
two fixed-point warps and ``invert_affine`` are those of tests/crop_twin.py.  ``getRotationMatrix2D``,
``warpAffine`` and ``resize`` below are also what tests/golden/make_augment_golden.py gives the reference's own code in place
of OpenCV, which is not installed where this is built.
"""
import itertools
import math

import numpy as np

from tests import crop_twin

F32, F64 = np.float32, np.float64
INTER_NEAREST, INTER_LINEAR, BORDER_CONSTANT = 0, 1, 0
BLUR_SIZES = (3, 5, 7, 9)
BLUR_TAPS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}
ORDERS = tuple(itertools.permutations(range(4)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROTATE, OVERLAP, RESIZE = (-30, 30), 0.8, (0.8, 1.2)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------ the draws
def uniform(lo, hi, u):
    return lo + (hi - lo) * float(u)


def randint(lo, hi, u):
    """``np.random.randint(lo, hi)`` from one uniform; ``lo`` where the reference raises (hi <= lo)."""
    lo, hi = int(lo), int(hi)
    return lo if hi <= lo else lo + min(int(math.floor(float(u) * float(hi - lo))), hi - lo - 1)


def degree_of(u, rotate=ROTATE):
    return uniform(float(rotate[0]), float(rotate[1]), u)


def cos_sin(deg):
    rad = deg * (math.pi / 180)
    return math.cos(rad), math.sin(rad)


def draws_for(B, seed):
    """A seeded table [B,12] of uniforms in [0, 1)."""
    return np.minimum(np.random.default_rng(seed).random((B, 12)), 1 - 2.0 ** -53)


# ------------------------------------------------------------------------------------------------------------ OpenCV's part
def getRotationMatrix2D(center, angle, scale):
    a, b = cos_sin(angle)
    a, b = a * scale, b * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1. - a) * cx - b * cy], [-b, a, b * cx + (1. - a) * cy]], F64)


def warpAffine(src, M, dsize, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    assert borderMode == BORDER_CONSTANT and borderValue == 0 and tuple(dsize) == (src.shape[1], src.shape[0])
    M = np.asarray(M, F64)
    if flags == INTER_NEAREST:
        return crop_twin.uncrop_mask(src[None], crop_twin.invert_affine(M)[None], dsize)[0].astype(src.dtype)
    assert flags == INTER_LINEAR
    return crop_twin.warp_u8(src, M, dsize)


def _resize_taps(dst, src):
    scale = F64(src) / F64(dst)
    f = ((np.arange(dst, dtype=F64) + 0.5) * scale - 0.5).astype(F32)
    fl = np.floor(f)
    s, f = fl.astype(np.int64), f - fl
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, F32(0), f).astype(F32)
    w0, w1 = np.rint((F32(1) - f) * F32(2048)).astype(np.int64), np.rint(f * F32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), w0, w1


def resize(src, dsize, interpolation=INTER_LINEAR):
    ow, oh = dsize
    h, w = src.shape[:2]
    if interpolation == INTER_NEAREST:
        sx = np.minimum(np.floor(np.arange(ow, dtype=F64) * (F64(w) / F64(ow))).astype(np.int64), w - 1)
        sy = np.minimum(np.floor(np.arange(oh, dtype=F64) * (F64(h) / F64(oh))).astype(np.int64), h - 1)
        return src[sy[:, None], sx[None, :]]
    assert interpolation == INTER_LINEAR
    x0, x1, a0, a1 = _resize_taps(ow, w)
    y0, y1, b0, b1 = _resize_taps(oh, h)
    p = src.astype(np.int64)
    S = p[:, x0] * a0[None, :, None] + p[:, x1] * a1[None, :, None]                        # [h, ow, 3]
    return ((S[y0] * b0[:, None, None] + S[y1] * b1[:, None, None] + (1 << 21)) >> 22).astype(np.uint8)


class cv2_stub:
    """What the golden script hands the reference's modules as ``cv2``."""
    INTER_NEAREST, INTER_LINEAR, BORDER_CONSTANT = INTER_NEAREST, INTER_LINEAR, BORDER_CONSTANT
    getRotationMatrix2D = staticmethod(getRotationMatrix2D)
    warpAffine = staticmethod(warpAffine)
    resize = staticmethod(resize)


# ------------------------------------------------------------------------------------------------------------ the geometry
def _fixed_window(img, mask, th, tw, hbeg, wbeg):
    """The crop at (hbeg, wbeg) and the centred pad of A:146-165 / A:180-194; returns the two pad offsets too."""
    H, W = mask.shape
    hpad, wpad = th >= H, tw >= W
    img, mask = img[hbeg:hbeg + th, wbeg:wbeg + tw], mask[hbeg:hbeg + th, wbeg:wbeg + tw]
    ph, pw = (th - H) // 2 if hpad else 0, (tw - W) // 2 if wpad else 0
    if hpad or wpad:
        nh, nw = mask.shape
        new_img, new_mask = np.zeros((th, tw, 3), np.uint8), np.zeros((th, tw), np.uint8)
        new_img[ph:ph + nh, pw:pw + nw], new_mask[ph:ph + nh, pw:pw + nw] = img, mask
        img, mask = new_img, new_mask
    return img, mask, ph, pw


def augment_one(img, mask, kpt_2d, out_size, u, rotate=ROTATE, overlap_ratio=OVERLAP, resize_ratio=RESIZE):
    """One sample; ``u`` its 12 draws.  Returns (img, mask, kpt_2d, path, window)."""
    height, width = out_size
    img, mask = np.asarray(img, np.uint8), np.asarray(mask).astype(np.uint8)
    kpt = np.asarray(kpt_2d).astype(F64).copy()
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    path, rot_img, rot_mask = 0, img, mask
    if len(xs):
        cx, cy = F64(int(xs.sum())) / F64(len(xs)), F64(int(ys.sum())) / F64(len(xs))
        M = getRotationMatrix2D((cx, cy), degree_of(u[0], rotate), 1)
        rm = warpAffine(mask, M, (W, H), flags=INTER_NEAREST)
        path = 1 if rm.any() else 2
        if path == 1:
            rot_img, rot_mask = warpAffine(img, M, (W, H), flags=INTER_LINEAR), rm
    if path != 1:
        th, tw = height, width
        hbeg, wbeg = (0 if th >= H else randint(0, H - th, u[2])), (0 if tw >= W else randint(0, W - tw, u[3]))
        o_img, o_mask, ph, pw = _fixed_window(img, mask, th, tw, hbeg, wbeg)
        return o_img, o_mask, kpt, path, np.array([th, tw, hbeg, wbeg, ph, pw], np.int32)
    ratio = uniform(float(resize_ratio[0]), float(resize_ratio[1]), u[1])
    th, tw = int(height * ratio), int(width * ratio)
    hs, ws = np.nonzero(rot_mask)
    hmin, hmax, wmin, wmax = int(hs.min()), int(hs.max()), int(ws.min()), int(ws.max())
    vh, vw = F64(hmin) + F64(overlap_ratio) * F64(hmax - hmin), F64(wmin) + F64(overlap_ratio) * F64(wmax - wmin)
    hrmax, hrmin = int(min(vh, H - th)), int(max(vh - th, 0))
    wrmax, wrmin = int(min(vw, W - tw)), int(max(vw - tw, 0))
    hpad, wpad = th >= H, tw >= W
    hbeg, wbeg = (0 if hpad else randint(hrmin, hrmax, u[2])), (0 if wpad else randint(wrmin, wrmax, u[3]))
    w_img, w_mask, ph, pw = _fixed_window(rot_img, rot_mask, th, tw, hbeg, wbeg)
    o_img, o_mask = resize(w_img, (width, height), INTER_LINEAR), resize(w_mask, (width, height), INTER_NEAREST)
    x, y = kpt[:, 0].copy(), kpt[:, 1].copy()
    xr, yr = (M[0, 0] * x + M[0, 1] * y) + M[0, 2], (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
    xr, yr = xr - F64(wbeg), yr - F64(hbeg)
    if hpad or wpad:
        xr, yr = xr + F64(pw), yr + F64(ph)
    kpt[:, 0], kpt[:, 1] = xr / F64(ratio), yr / F64(ratio)
    return o_img, o_mask, kpt, 1, np.array([th, tw, hbeg, wbeg, ph, pw], np.int32)


def pvnet_augment(img, mask, kpt_2d, out_size, draws, **kw):
    outs = [augment_one(img[b], mask[b], kpt_2d[b], out_size, draws[b], **kw) for b in range(len(img))]
    return {"img": np.stack([o[0] for o in outs]), "mask": np.stack([o[1] for o in outs]), "kpt_2d": np.stack([o[2] for o in outs]),
            "path": np.array([o[3] for o in outs], np.int32), "window": np.stack([o[4] for o in outs])}


# ------------------------------------------------------------------------------------------------------------ the transforms
def blur_taps(k):
    if k == 9:
        g = [math.exp(-((i - 4) * (i - 4)) / (2 * 1.7 * 1.7)) for i in range(9)]
        total = sum(g)
        taps = [int(round(256 * (v / total))) for v in g]
        taps[4] += 256 - sum(taps)
        return taps
    return list(BLUR_TAPS[k])


def blur(img, k):
    """The separable blur on a reflect-101 border in 8.8 fixed point: rows T = sum w*p, columns (sum w*T + 2^15) >> 16."""
    w, r = np.array(blur_taps(k), np.int64), k // 2
    p = np.pad(np.asarray(img, np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
    h, wd = img.shape[:2]
    T = sum(w[j] * p[:, j:j + wd] for j in range(k))
    return ((sum(w[j] * T[j:j + h] for j in range(k)) + (1 << 15)) >> 16).astype(np.uint8)


def luma(v):
    v = v.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def blend(d, p, f):
    """PIL's ImagingBlend(degenerate, image, factor) on uint8 bands, in float32."""
    d, p = np.asarray(d, np.int64), np.asarray(p, np.int64)
    t = d.astype(F32) + F32(f) * (p - d).astype(F32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def contrast_grey(img):
    return int(F64(int(luma(img).sum())) / F64(img.shape[0] * img.shape[1]) + 0.5)


def enhance(img, op, f):
    """``ImageEnhance.Brightness`` / ``Contrast`` / ``Color`` or the hue shift on [h,w,3] uint8."""
    if op == HUE:
        return adjust_hue(img, f)
    if op == BRIGHTNESS:
        d = np.zeros_like(img)
    elif op == CONTRAST:
        d = np.full_like(img, contrast_grey(img))
    else:
        d = np.repeat(luma(img)[..., None], 3, -1)
    return blend(d, img, f)


def rgb2hsv(rgb):
    """PIL's convert("HSV") of [...,3] uint8 (rgb2hsv_row: float32 where it declares floats, binary64 where a literal widens)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(F32)
    s = cr / np.where(grey, 1, maxc).astype(F32)
    rc, gc, bc = (maxc - r).astype(F32) / cr, (maxc - g).astype(F32) / cr, (maxc - b).astype(F32) / cr
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, ((2.0 + rc.astype(F64)) - bc.astype(F64)).astype(F32),
                                              ((4.0 + gc.astype(F64)) - rc.astype(F64)).astype(F32)))
    t = h.astype(F64) / 6.0 + 1.0
    h = (t - np.floor(t)).astype(F32)
    uh = np.clip((h.astype(F64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(F64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv2rgb(hsv):
    """PIL's convert("RGB") of an HSV image [...,3] uint8 (hsv2rgb)."""
    h, s, v = (hsv[..., i].astype(np.int64) for i in range(3))
    hf = h.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int64)
    f = (hf - i.astype(F32).astype(F64)).astype(F32)
    fs = (s.astype(F32).astype(F64) / 255.0).astype(F32)
    vf = v.astype(F32).astype(F64)
    rnd = lambda x: np.clip(np.floor(x + 0.5).astype(np.int64), 0, 255)          # noqa: E731
    p, q = rnd(vf * (1.0 - fs.astype(F64))), rnd(vf * (1.0 - (fs * f).astype(F64)))
    t = rnd(vf * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64))))
    k = i % 6
    out = np.stack([np.choose(k, [v, q, p, p, t, v]), np.choose(k, [t, v, v, q, p, p]), np.choose(k, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue_shift(f):
    """What torchvision's ``adjust_hue`` adds to the 8-bit hue, modulo 256."""
    return int(f * 255) & 255


def adjust_hue(img, f):
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + hue_shift(f)) & 255
    return hsv2rgb(hsv)


def jitter_of(u, blur_prob=0.5, jitter=(0.1, 0.1, 0.05, 0.05)):
    """(k, factors, the applied operations in order) of one sample's draws."""
    k = BLUR_SIZES[min(int(math.floor(4 * float(u[5]))), 3)] if float(u[4]) < blur_prob else 0
    lo = [max(0.0, 1 - jitter[0]), max(0.0, 1 - jitter[1]), max(0.0, 1 - jitter[2]), -jitter[3]]
    hi = [1 + jitter[0], 1 + jitter[1], 1 + jitter[2], jitter[3]]
    f = [uniform(lo[i], hi[i], u[6 + i]) for i in range(4)]
    order = ORDERS[min(int(math.floor(24 * float(u[10]))), 23)]
    return k, f, [op for op in order if jitter[op] != 0]


def normalise(u8, mean=MEAN, std=STD):
    """``ToTensor`` and ``Normalize`` as numpy runs them (X:32, 43-46): [h,w,3] uint8 -> [3,h,w] float32."""
    x = u8.astype(F32) / F32(255)
    x = (x.astype(F64) - np.asarray(mean, F64)).astype(F32)
    x = (x.astype(F64) / np.asarray(std, F64)).astype(F32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def transform_one(img, u, blur_prob=0.5, jitter=(0.1, 0.1, 0.05, 0.05), mean=MEAN, std=STD, u8=False):
    img = np.asarray(img, np.uint8)
    if u is not None:
        k, f, ops = jitter_of(u, blur_prob, jitter)
        if k:
            img = blur(img, k)
        for op in ops:
            img = enhance(img, op, f[op])
    return img if u8 else normalise(img, mean, std)


def pvnet_transform(img, draws, **kw):
    return np.stack([transform_one(img[b], None if draws is None else draws[b], **kw) for b in range(len(img))])


# ------------------------------------------------------------------------------------------------------------ binary64 samplers
def tap_f64(img, sy, sx):
    H, W = img.shape[:2]
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    v = np.asarray(img, F64)[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
    return np.where(ok[..., None], v, 0.)


def rotate_f64(img, M):
    """Plain bilinear interpolation of a float image at the exact inverse-mapped position, zero outside."""
    H, W = img.shape[:2]
    A = np.linalg.inv(np.vstack([M, [0, 0, 1]]))
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    u, v = A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2]
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = (u - u0)[..., None], (v - v0)[..., None]
    return (tap_f64(img, v0, u0) * (1 - fu) * (1 - fv) + tap_f64(img, v0, u0 + 1) * fu * (1 - fv)
            + tap_f64(img, v0 + 1, u0) * (1 - fu) * fv + tap_f64(img, v0 + 1, u0 + 1) * fu * fv)


def resize_f64(img, dsize):
    """Plain bilinear resize of a float image with half-pixel centres and replicated edges."""
    ow, oh = dsize
    h, w = img.shape[:2]
    img = np.asarray(img, F64)
    fx, fy = (np.arange(ow) + 0.5) * (w / ow) - 0.5, (np.arange(oh) + 0.5) * (h / oh) - 0.5
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    cx, cy = lambda i: np.clip(i, 0, w - 1), lambda i: np.clip(i, 0, h - 1)      # noqa: E731
    ax = np.where(((x0 < 0) | (x0 >= w - 1))[None, :, None], 0., ax)
    ay = np.where(((y0 < 0) | (y0 >= h - 1))[:, None, None], 0., ay)
    rows = img[:, cx(x0)] * (1 - ax) + img[:, cx(x0 + 1)] * ax
    return rows[cy(y0)] * (1 - ay) + rows[cy(y0 + 1)] * ay


def blur_f64(img, k):
    w, r = np.array(blur_taps(k), F64) / 256., k // 2
    p = np.pad(np.asarray(img, F64), ((r, r), (r, r), (0, 0)), mode="reflect")
    h, wd = img.shape[:2]
    T = sum(w[j] * p[:, j:j + wd] for j in range(k))
    return sum(w[j] * T[j:j + h] for j in range(k))


# ------------------------------------------------------------------------------------------------------------ shared inputs
def image(seed, H=48, W=70):
    return crop_twin.image(seed, H, W)


def blob(H, W, y0, y1, x0, x1, value=1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


def keypoints(mask, K, seed):
    """K points around the mask's box (or the image's centre), binary64 with fractional parts."""
    rng = np.random.default_rng(seed)
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    c = (xs.mean(), ys.mean()) if len(xs) else (W / 2, H / 2)
    return np.stack([c[0] + rng.uniform(-12, 12, K), c[1] + rng.uniform(-9, 9, K)], 1)


MIXED_ROTATE, MIXED_RESIZE = (-30, 90), (0.5, 2.5)     # u = 0, 0.25, 0.5 draw the degrees -30, 0, 30 exactly
MIXED_RATIOS = {(40, 66): (0.84, 1.3, 1.1, 1.0, 0.9),   # 48 x 70: rows pad from r = 1.2, columns from 1.0606...: columns only at 1.1
                (44, 40): (0.84, 1.8, 1.15, 1.0, 0.9)}  # 48 x 70: rows pad from r = 1.0909..., columns from 1.75: rows only at 1.15


def mixed_batch(out_size, H=48, W=70, K=9):
    """B = 5: crop on both axes, pad on both, pad on one axis only, an empty mask, a single-pixel mask, with the degrees -30, 0,
    30, 30, -30 under ``MIXED_ROTATE`` / ``MIXED_RESIZE``.  At the base ``out_size`` (40, 66) a 48 x 70 image can pad its
    columns alone, never its rows alone (th / H < tw / W); at (44, 40) it is the rows.  Returns (img, mask, kpt_2d, draws)."""
    masks = [blob(H, W, 14, 33, 22, 51), blob(H, W, 10, 30, 18, 44, 255), blob(H, W, 20, 40, 30, 60), np.zeros((H, W), np.uint8),
             blob(H, W, 25, 26, 37, 38)]
    masks[0][20, 30] = 0                                                           # a hole
    d = draws_for(5, 11)
    d[:, 0] = [0.0, 0.25, 0.5, 0.5, 0.0]
    d[:, 1] = [(r - MIXED_RESIZE[0]) / (MIXED_RESIZE[1] - MIXED_RESIZE[0]) for r in MIXED_RATIOS[tuple(out_size)]]
    img = np.stack([image(20 + i, H, W) for i in range(5)])
    kpt = np.stack([keypoints(masks[i], K, 30 + i) for i in range(5)])
    return img, np.stack(masks), kpt, d


MIXED_KW = dict(rotate=MIXED_ROTATE, resize_ratio=MIXED_RESIZE)


def empty_rotation_case(H=48, W=70):
    """(mask, draws of one sample): two pixels in opposite corners, rotated by -30 degrees (u = 0 on the default range) around
    their centre, both leave the image: path 2."""
    m = np.zeros((H, W), np.uint8)
    m[0, 0] = m[H - 1, W - 1] = 1
    d = draws_for(1, 21)[0]
    d[0] = 0.0
    return m, d


def contrast_boundary_image(H=40, W=66):
    """Greys, the left half at 100 and the right half at 101: PIL's L is the grey itself, the mean 100.5."""
    img = np.full((H, W, 3), 100, np.uint8)
    img[:, W // 2:] = 101
    return img
