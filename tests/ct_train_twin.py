"""numpy twin of the arithmetic contract of include/pvnet_vote.h, "Detector training: heat-map targets and the detector loss",
written from the contract with every operation and its order explicit.  The CPU tests (tests/test_ct_train.py) pin this twin to
fixtures made by the reference's own ``prepare_detection``, ``ct_collator`` and ``NetworkWrapper``
(tests/golden/make_ct_train_golden.py); the GPU tests (tests/test_gpu_ct_train.py) hold the device to the twin.

How results are held (u = 2**-24; nothing here is tuned):
  targets          ct_ind, wh, ct_cls, ct_01, ct_num, the radii and the whole heat map: as bytes against the reference (both use
                   numpy's exp); the device's heat map as bytes at every centre (exp(-0) = 1 decides positive against negative) and
                   within one float32 elsewhere (the exp of another library, rounded to float32 once).
  ct_loss, wh_loss within one float32 ulp of the reference's float64 run: every term here is binary64 from the same float32 inputs,
                   the sums differ in order only (n * 2**-53 relative, the terms of one sum have one sign), and the result is
                   rounded to float32 once.
  logit gradient   within one float32 ulp of the float64 run: both terms of each derivative have one sign, nothing cancels, and
                   1 - s is only used where the clamp passes (s <= 0.9999), so each element is a few 2**-53 off before its one
                   rounding to float32.
  the clamp        torch.clamp compares a float32 tensor with float32(1e-4) and float32(1 - 1e-4) = 0.99989998..., a float64 tensor
                   with 1e-4 and 0.9999.  The contract has the float32 values (``LO``, ``HI``).  The reference's float64 run
                   therefore differs from its own float32 run at every clamped element by log(1 - HI) - log(1e-4) = 1.66e-4, far
                   more than a rounding; the tests evaluate this twin with that run's own two constants (``lo=``, ``hi=``) when they
                   compare with it, and with the contract's when they compare with the float32 run.  The distance of the two
                   reference runs is measured by the fixture script and stored, and the float32 comparison allows the ulp plus it.
  wh gradient      as bytes against torch's CPU autograd: float32 operations in a stated order.
"""
import os

import numpy as np

from tests.train_twin import F32, F64, GOLDEN, SLOTS, TILE, U, fixed_sum, image_sum, ulp_apart  # noqa: F401

MAX_N = 512                                     # PVV_CT_TRAIN_MAX_N
LO, HI = F64(F32(1e-4)), F64(F32(1 - 1e-4))     # what a float32 sigmoid is clamped to
LN9999 = float(np.log(9999.0))


# ------------------------------------------------------------------------------------------------ the targets
def gaussian_radius(height, width):
    """The contract's R for integral height and width, binary64, every step rounded once."""
    height, width = F64(height), F64(width)
    mo = F64(0.7)
    s = height + width
    c1 = ((width * height) * (F64(1) - mo)) / (F64(1) + mo)
    r1 = (s + np.sqrt(s * s - F64(4) * c1)) / F64(2)
    b2 = F64(2) * s
    c2 = ((F64(1) - mo) * width) * height
    r2 = (b2 + np.sqrt(b2 * b2 - F64(16) * c2)) / F64(2)
    a3 = F64(4) * mo
    b3 = (F64(-2) * mo) * s
    c3 = ((mo - F64(1)) * width) * height
    d3 = b3 * b3 - (F64(4) * a3) * c3
    r12 = r2 if r2 < r1 else r1
    r3 = r12 if d3 < 0 else (b3 + np.sqrt(d3)) / F64(2)
    return r3 if r3 < r12 else r12


def one_object(box, cls, C, H, W):
    """None when the object is dropped, else (cx, cy, r, cls, float32 w, float32 h)."""
    x0, y0, x1, y1 = (F64(v) for v in box)
    if not all(abs(v) < 2.0 ** 24 for v in (x0, y0, x1, y1)):
        return None
    w, h = x1 - x0, y1 - y0
    if not (w > 0 and h > 0) or not 0 <= int(cls) < C:
        return None
    cx, cy = int(np.rint(F32((x0 + x1) / F64(2)))), int(np.rint(F32((y0 + y1) / F64(2))))
    if not (0 <= cx < W and 0 <= cy < H):
        return None
    r = max(0, int(gaussian_radius(np.ceil(h), np.ceil(w))))
    return cx, cy, r, int(cls), F32(w), F32(h)


def ct_targets(boxes, cls, num, C, H, W):
    """dict of ct_hm [B,C,H,W] f32, wh [B,N,2] f32, ct_cls, ct_ind [B,N] i64, ct_01 [B,N] f32, ct_num [B] i64 and radius [B,N] i64
    (packed like the rows; not an output of the device)."""
    boxes, cls, num = np.asarray(boxes), np.asarray(cls), np.asarray(num)
    B, N = cls.shape
    out = {"ct_hm": np.zeros((B, C, H, W), F32), "wh": np.zeros((B, N, 2), F32), "ct_cls": np.zeros((B, N), np.int64),
           "ct_ind": np.zeros((B, N), np.int64), "ct_01": np.zeros((B, N), F32), "ct_num": np.zeros(B, np.int64),
           "radius": np.zeros((B, N), np.int64)}
    for b in range(B):
        k = 0
        for n in range(min(max(int(num[b]), 0), N)):
            q = one_object(boxes[b, n], cls[b, n], C, H, W)
            if q is None:
                continue
            cx, cy, r, c, w, h = q
            sigma = F64(2 * r + 1) / F64(6)
            ss = sigma * sigma
            xs, ys = np.arange(max(0, cx - r), min(W, cx + r + 1)), np.arange(max(0, cy - r), min(H, cy + r + 1))
            dx, dy = (xs - cx).astype(F64)[None, :], (ys - cy).astype(F64)[:, None]
            g = np.exp(-((dx * dx) / ss + (dy * dy) / ss) / F64(2)).astype(F32)
            plane = out["ct_hm"][b, c, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            np.maximum(plane, g, out=plane)
            out["wh"][b, k] = (w, h)
            out["ct_cls"][b, k], out["ct_ind"][b, k], out["ct_01"][b, k], out["radius"][b, k] = c, cy * W + cx, 1, r
            k += 1
        out["ct_num"][b] = k
    return out


# ------------------------------------------------------------------------------------------------ the focal loss
def _sigmoid(z, lo, hi):
    with np.errstate(over="ignore"):
        s = F64(1) / (F64(1) + np.exp(-np.asarray(z, F32).astype(F64)))
    p = np.where(s < lo, lo, np.where(s > hi, hi, s))
    return s, p


def _neg_weight(g):
    w = F64(1) - g.astype(F64)
    w2 = w * w
    return w2 * w2


def focal_sums(z, g, lo=LO, hi=HI):
    """(P, Q, num_pos): the two binary64 sums in the contract's order and the integer count."""
    z, g = np.asarray(z, F32), np.asarray(g, F32)
    B = z.shape[0]
    _, p = _sigmoid(z, lo, hi)
    q = F64(1) - p
    pos = np.where(g == 1, np.log(p) * (q * q), F64(0))
    neg = np.where(g < 1, (np.log(q) * (p * p)) * _neg_weight(g), F64(0))
    return fixed_sum(pos.reshape(B, -1)), fixed_sum(neg.reshape(B, -1)), int((g == 1).sum())


def focal_loss(z, g, lo=LO, hi=HI):
    P, Q, npos = focal_sums(z, g, lo, hi)
    return F32(-Q) if npos == 0 else F32(-(P + Q) / F64(npos))


def focal_grad(z, g, go=1.0, lo=LO, hi=HI):
    """(gradient float32, the same before its rounding)."""
    z, g = np.asarray(z, F32), np.asarray(g, F32)
    npos = int((g == 1).sum())
    go = F64(F32(go))
    k = -go if npos == 0 else -go / F64(npos)
    s, p = _sigmoid(z, lo, hi)
    q = F64(1) - p
    dpos = (q * q) / p - (F64(2) * q) * np.log(p)
    dneg = ((F64(2) * p) * np.log(q) - (p * p) / q) * _neg_weight(g)
    dp = np.where(g == 1, dpos, np.where(g < 1, dneg, F64(0)))
    grad = np.where((s >= lo) & (s <= hi), (k * dp) * ((F64(1) - s) * s), F64(0))
    return grad.astype(F32), grad


# ------------------------------------------------------------------------------------------------ the wh loss
def bad_indices(ct_ind, ct_01, HW):
    ind = np.asarray(ct_ind).astype(np.int64)
    return int((((ind < 0) | (ind >= HW)) & (np.asarray(ct_01) != 0)).sum())


def wh_sums(wh_pred, wh, ct_ind, ct_01):
    """(S, M) binary64 in the contract's order; every index in range."""
    wp, tg, m = np.asarray(wh_pred, F32), np.asarray(wh, F32), np.asarray(ct_01, F32).astype(F64)
    B, _, H, W = wp.shape
    ind = np.asarray(ct_ind).astype(np.int64)
    flat = wp.reshape(B, 2, H * W).astype(F64)
    S = M = F64(0)
    for b in range(B):
        el = []
        for c in range(2):
            d = flat[b, c, ind[b]] * m[b] - tg[b, :, c].astype(F64) * m[b]
            z = np.abs(d)
            el.append(np.where(z < 1, (F64(0.5) * z) * z, z - F64(0.5)))
        S = S + image_sum(el[0] + el[1])
        M = M + image_sum(m[b])
    return S, M


def wh_loss(wh_pred, wh, ct_ind, ct_01):
    S, M = wh_sums(wh_pred, wh, ct_ind, ct_01)
    return F32(S / (M * F64(2) + F64(1e-4)))


def wh_grad(wh_pred, wh, ct_ind, ct_01, go=1.0):
    """float32 throughout; objects that share an index add up in ascending order from +0."""
    wp, tg, m = np.asarray(wh_pred, F32), np.asarray(wh, F32), np.asarray(ct_01, F32)
    B, _, H, W = wp.shape
    ind = np.asarray(ct_ind).astype(np.int64)
    _, M = wh_sums(wp, tg, ind, m)
    den = F32(M) * F32(2) + F32(1e-4)
    v = F32(go) / den
    out = np.zeros((B, 2, H * W), F32)
    flat = wp.reshape(B, 2, H * W)
    for b in range(B):
        for n in range(ind.shape[1]):
            for c in range(2):
                d = flat[b, c, ind[b, n]] * m[b, n] - tg[b, n, c] * m[b, n]
                t = (-v if d < -1 else v if d > 1 else v * d) * m[b, n]
                out[b, c, ind[b, n]] = out[b, c, ind[b, n]] + t
    assert out.dtype == F32 and den.dtype == F32
    return out.reshape(B, 2, H, W)


# ------------------------------------------------------------------------------------------------ the cases
def issue_boxes(C, H, W, N, seed, kind="float"):
    """Three images of boxes that cover what the issue lists (image 2 has num = 0): (boxes [3,N,4], cls [3,N], num [3]).
    Image 0: two overlapping objects of one class, a radius-0 object, windows clipped at the left, top, right and bottom border and
    at a corner, a degenerate box in the middle of the list, two objects with one centre, half-integer centres 3.5 and 4.5
    (both round to 4), a class outside [0, C) and a centre outside the map.  Image 1: random boxes up to N.  ``kind`` "int" rounds
    them to int64 (the half-integer centres then come from odd sums of integer corners)."""
    rng = np.random.default_rng(seed)
    c = lambda i: i % C                                                            # noqa: E731
    first = [
        ((10.0, 8.0, 22.0, 20.0), c(0)), ((14.0, 11.0, 27.0, 22.0), c(0)),         # overlapping, one class
        ((30.0, 5.0, 31.0, 6.0), c(1)),                                            # radius 0
        ((-5.0, 10.0, 7.0, 22.0), c(1)), ((20.0, -6.0, 32.0, 6.0), c(2)),          # clipped left, top
        ((9.0, 9.0, 9.0, 15.0), c(0)),                                             # degenerate, in the middle of the list
        ((W - 7.0, 10.0, W + 5.0, 22.0), c(2)), ((12.0, H - 7.0, 24.0, H + 5.0), c(1)),   # clipped right, bottom
        ((W - 8.0, H - 8.0, W + 4.0, H + 4.0), c(0)),                              # a corner
        ((16.0, 14.0, 24.0, 20.0), c(2)), ((13.0, 12.0, 27.0, 22.0), c(2)),        # one centre (20, 17), one class
        ((1.0, 25.0, 6.0, 30.0), c(1)), ((2.0, 26.0, 7.0, 31.0), c(1)),            # centres 3.5 and 4.5 in x: both 4
        ((5.0, 5.0, 9.0, 9.0), C), ((5.0, 5.0, 9.0, 9.0), -1),                     # a class outside [0, C)
        ((W + 4.0, 3.0, W + 12.0, 9.0), c(0)),                                     # a centre outside the map
        ((3.0, 1.0, 7.5, 4.25), c(0)),                                             # a fractional size: ceil matters
    ]
    if H < 34 or W < 45:                                                           # a map too small for the list: one object
        first = [((2.0, 1.0, 9.0, 6.0), c(1))]
    boxes, cls = np.zeros((3, N, 4), F64), np.zeros((3, N), np.int64)
    num = np.array([min(N, len(first)), N, 0], np.int64)
    for n, (bx, cl) in enumerate(first[:N]):
        boxes[0, n], cls[0, n] = bx, cl
    x0, y0 = rng.uniform(-4, W - 2, N), rng.uniform(-4, H - 2, N)
    boxes[1] = np.stack([x0, y0, x0 + rng.uniform(0.5, W / 2, N), y0 + rng.uniform(0.5, H / 2, N)], 1)
    cls[1] = rng.integers(0, C, N)
    boxes[2], cls[2] = boxes[1], cls[1]                                            # rows that num = 0 must ignore
    if kind == "int":
        return np.rint(boxes).astype(np.int64), cls, num
    return boxes.astype(F32), cls, num


def redraw_band(z, rng):
    """Logits redrawn until none lies within 0.01 of +-ln 9999: there a float32 and a binary64 sigmoid disagree about the clamp
    and the gradient jumps by O(1/num_pos).  A choice of inputs; no element is left out of any comparison."""
    z = np.asarray(z, F32).copy()
    while True:
        band = np.abs(np.abs(z.astype(F64)) - LN9999) < 0.01
        if not band.any():
            return z
        z[band] = (rng.standard_normal(int(band.sum())) * 3).astype(F32)


def make_inputs(B, C, H, W, N, seed, kind="float", clamp=None, no_pos=False):
    """Seeded inputs of a loss case: the targets of ``issue_boxes`` (its first B images), logits N(0, 3) redrawn outside the
    clamp band -- or, with ``clamp`` = 12 or 30, +-clamp on a quarter of the elements, positives included -- and wh predictions
    within a few pixels of the targets with saturated elements on both sides.  ``no_pos``: every box degenerate."""
    rng = np.random.default_rng(seed)
    boxes, cls, num = (a[:B] for a in issue_boxes(C, H, W, N, seed, kind))
    if no_pos:
        boxes = boxes.copy()
        boxes[..., 2] = boxes[..., 0]
    t = ct_targets(boxes, cls, num, C, H, W)
    z = redraw_band((rng.standard_normal((B, C, H, W)) * 3).astype(F32), rng)
    if clamp is not None:
        pick = rng.random(z.shape) < 0.25
        z[pick] = (rng.choice([-1, 1], int(pick.sum())) * clamp).astype(F32)
        pos = np.argwhere(t["ct_hm"] == 1)
        for i, at in enumerate(pos):
            z[tuple(at)] = F32(clamp if i % 2 else -clamp)
    wp = (rng.standard_normal((B, 2, H, W)) * 4 + 8).astype(F32)
    flat = wp.reshape(B, 2, H * W)
    for b in range(B):
        for n in range(int(t["ct_num"][b])):
            if n % 3:                                                              # within one pixel: the quadratic part
                flat[b, :, t["ct_ind"][b, n]] = t["wh"][b, n] + rng.uniform(-0.9, 0.9, 2).astype(F32)
    d = {"boxes": boxes, "cls": cls, "num": num, "ct_hm_pred": z, "wh_pred": wp}
    d.update(t)
    return d


# name -> (B, C, H, W, N, seed, kind, clamp, no_pos): the cases of tests/golden/ct_train_<name>.npz
GOLDEN_CASES = {
    "c3_37x53": (2, 3, 37, 53, 20, 31, "float", None, False),
    "c30_34x45_int": (3, 30, 34, 45, 130, 32, "int", None, False),
    "clamp12": (2, 3, 37, 53, 20, 33, "float", 12, False),
    "clamp30": (1, 4, 8, 12, 1, 34, "int", 30, False),
    "no_pos": (2, 3, 37, 53, 20, 35, "float", None, True),
}

# the shapes of the GPU tests, the smallest that reach every path -- 2x3x37x53: C*H*W odd, the scalar form, five full tiles and a
# partial one; 1x4x8x12: the 16-byte form, less than a tile, N = 1; 3x30x34x45: N = 130, integer boxes, an image with num = 0;
# 1x30x96x128: 360 tiles, so the image slots wrap
GPU_CASES = dict(GOLDEN_CASES)
GPU_CASES.update({
    "vec_4x8x12": (1, 4, 8, 12, 1, 36, "float", None, False),
    "slots_30x96x128": (1, 30, 96, 128, 17, 37, "float", None, False),
})
_cache = {}


def golden_inputs(name):
    B, C, H, W, N, seed, kind, clamp, no_pos = GOLDEN_CASES[name]
    return make_inputs(B, C, H, W, N, seed, kind, clamp, no_pos)


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, "ct_train_%s.npz" % name)))


def reference(name):
    """The inputs of a GPU case with the twin's results, computed once and shared; treat as read-only."""
    if name not in _cache:
        B, C, H, W, N, seed, kind, clamp, no_pos = GPU_CASES[name]
        d = make_inputs(B, C, H, W, N, seed, kind, clamp, no_pos)
        a = (d["wh_pred"], d["wh"], d["ct_ind"], d["ct_01"])
        d["ct_loss"], d["wh_loss"] = focal_loss(d["ct_hm_pred"], d["ct_hm"]), wh_loss(*a)
        d["hm_grad"], d["wh_grad"] = focal_grad(d["ct_hm_pred"], d["ct_hm"])[0], wh_grad(*a)
        d.update(B=B, C=C, H=H, W=W, N=N)
        _cache[name] = d
    return _cache[name]
