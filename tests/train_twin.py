"""numpy twin of the arithmetic contract of include/pvnet_vote.h, "Training: vote targets and the PVNet loss", written from
the contract with every operation and its order explicit, plus the bounds that results are held to.  The CPU tests
(tests/test_train.py) pin this twin to fixtures made by the reference's own ``compute_vertex`` and ``NetworkWrapper``
(tests/golden/make_train_golden.py); the GPU tests (tests/test_gpu_train.py) hold the device to the twin.

Bounds (u = 2**-24 for float32, v = 2**-53 for binary64; all derived, none tuned):
  vote loss against a binary64 evaluation   8*u*want.  d = pred*w - target*w rounds once (the products with w in {0, 1, 2} are
          exact), |d| -> (0.5*z)*z or z - 0.5 once more on a quantity already off by u: at most 4u relative per element
          (for z >= 1, z - 0.5 >= z/2), and the elements are non-negative, so the sum is off by 4u relative at most; the
          binary64 sum adds n*v, far below u; float32(S), / wsum and / 2K round three times.  One more u for second-order terms.
  vote loss against a float32 sum           n*u/(1 - n*u) * want with n = (elements + 8): any order of a float32 sum of
          non-negative terms is within (elements - 1)*u/(1 - ...) relative; both sides divide twice or three times.
  seg loss against a binary64 evaluation    2*u*want: the binary64 terms differ by a few v, the result rounds once.
  seg loss against float32 log-softmax      (pixels + 2)*u/(1 - (pixels + 2)*u) * want + (C + 6)*u*(zmax + log C): the float32
          mean of the pixel terms in any order, plus per pixel the roundings of z - m, exp, the C - 1 additions, log and the
          two additions of the log-sum-exp, each at most u of a quantity no larger than zmax + log C.
  seg gradient against a binary64 run       c*v*|go|/N before the float32 rounding, c = 2*(C + 6) + 2*(zrange + log C): a
          probability is at most 1; the two evaluations each round z - m, exp, C - 1 additions, the product, two divisions
          (C + 6 with slack for exp and log being a unit off) and torch's exp(z - m - log s) form turns an error of v relative
          in an exponent of magnitude up to zrange + log C into that many v relative.
  vote gradient                             bit for bit: every operation is a float32 operation in a stated order.
  vote gradient against other float32 ops   8*u*|g|: s = (go / 2K) / wsum and s*d round three times, * w is exact; another
          association of the same factors rounds as often.
  seg gradient against float32 softmax      2*((C + 8) + (zrange + log C))*u*|go|/N: as for binary64, with u for v and the
          final rounding of each side added.
  device seg loss / gradient against twin   a neighbouring float32 at most (binary64 exp and log of two libraries).
"""
import os

import numpy as np

F32, F64 = np.float32, np.float64
U, V = 2.0 ** -24, 2.0 ** -53
LANE, TILE, SLOTS = 4, 1024, 256               # PVV_TRAIN_LANE_PIXELS, PVV_TRAIN_TILE, PVV_TRAIN_IMAGE_SLOTS
MAX_K, MAX_C = 64, 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ the target
def compute_vertex(mask, kpt_2d):
    """[B,2K,H,W] float32 from mask [B,H,W] and kpt_2d [B,K,2]: the contract's target."""
    mask, kpt = np.asarray(mask), np.asarray(kpt_2d).astype(F64)
    B, H, W = mask.shape
    K = kpt.shape[1]
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    out = np.zeros((B, 2 * K, H, W), F32)
    for b in range(B):
        fg = mask[b] == 1
        for k in range(K):
            dx, dy = kpt[b, k, 0] - x[fg], kpt[b, k, 1] - y[fg]
            n = np.sqrt(dx * dx + dy * dy)
            n = np.where(n < 1e-3, n + 1e-3, n)
            out[b, 2 * k][fg] = (dx / n).astype(F32)
            out[b, 2 * k + 1][fg] = (dy / n).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ the fixed-order sums
def block_sum(a):
    """The last axis (256 slots) in the order slot j += slot j + s, s = 128 ... 1."""
    a = np.array(a, F64)
    assert a.shape[-1] == SLOTS
    s = SLOTS // 2
    while s > 0:
        a[..., :s] = a[..., :s] + a[..., s:2 * s]
        s //= 2
    return a[..., 0]


def tile_sums(terms, tiles=None):
    """terms [HW] binary64 per-pixel terms of one image -> the sums of its tiles; ``tiles`` picks which tiles, in any order."""
    terms = np.asarray(terms, F64)
    T = -(-terms.size // TILE)
    padded = np.zeros(T * TILE, F64)
    padded[:terms.size] = terms
    p = padded.reshape(T, SLOTS, LANE)
    if tiles is not None:
        p = p[np.asarray(tiles)]
    lane = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    return block_sum(lane)


def image_sum(tile_values):
    """The sum of one image from its tile sums (in tile order)."""
    slots = np.zeros(SLOTS, F64)
    for t0 in range(0, len(tile_values), SLOTS):
        chunk = np.asarray(tile_values[t0:t0 + SLOTS], F64)
        slots[:chunk.size] = slots[:chunk.size] + chunk
    return block_sum(slots)


def fixed_sum(terms):
    """terms [B, HW] -> the batch sum in the contract's order."""
    total = F64(0.0)
    for b in range(terms.shape[0]):
        total = total + image_sum(tile_sums(terms[b]))
    return total


# ------------------------------------------------------------------------------------------------ the vote loss
def vote_d(vertex_pred, target, mask):
    w = np.asarray(mask).astype(F32)[:, None]
    d = np.asarray(vertex_pred, F32) * w - np.asarray(target, F32) * w
    assert d.dtype == F32
    return d, w


def vote_elements(d):
    z = np.abs(d)
    with np.errstate(invalid="ignore"):
        e = np.where(z < F32(1), (F32(0.5) * z) * z, z - F32(0.5))
    assert e.dtype == F32
    return e


def mask_sum(mask):
    return int(np.asarray(mask).astype(np.int64).sum())


def vote_loss(vertex_pred, target, mask):
    """(loss float32, S binary64)."""
    d, _ = vote_d(vertex_pred, target, mask)
    e = vote_elements(d).astype(F64)
    B, C2 = e.shape[:2]
    pix = np.zeros((B, e.shape[2] * e.shape[3]), F64)
    for c in range(C2):                                            # ascending channel
        pix = pix + e[:, c].reshape(B, -1)
    S = fixed_sum(pix)
    wsum = F32(mask_sum(mask))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (F32(S) / wsum) / F32(C2), S


def vote_grad(vertex_pred, target, mask, go=1.0):
    d, w = vote_d(vertex_pred, target, mask)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (F32(go) / F32(d.shape[1])) / F32(mask_sum(mask))
        g = np.where(d < F32(-1), -s, np.where(d > F32(1), s, s * d)) * w
    assert g.dtype == F32
    return g


# ------------------------------------------------------------------------------------------------ the seg loss
def _softmax_parts(seg_pred, mask):
    z = np.asarray(seg_pred, F32)
    B, C, H, W = z.shape
    label = np.asarray(mask).astype(np.int64)
    m = z[:, 0].copy()
    for c in range(1, C):
        m = np.where(z[:, c] > m, z[:, c], m)
    e = np.exp(z.astype(F64) - m.astype(F64)[:, None])
    s = np.zeros((B, H, W), F64)
    rest = np.zeros((B, H, W), F64)
    for c in range(C):
        s = s + e[:, c]
        rest = np.where(label != c, rest + e[:, c], rest)
    return z, label, m, e, s, rest


def bad_labels(mask, C):
    label = np.asarray(mask).astype(np.int64)
    return int(((label < 0) | (label >= C)).sum())


def seg_loss(seg_pred, mask):
    """(loss float32, G binary64); labels are in range."""
    z, label, m, e, s, _ = _softmax_parts(seg_pred, mask)
    B, C, H, W = z.shape
    assert bad_labels(mask, C) == 0
    zl = np.take_along_axis(z, label[:, None], 1)[:, 0]
    term = (m.astype(F64) - zl.astype(F64)) + np.log(s)
    G = fixed_sum(term.reshape(B, -1))
    return F32(G / F64(B * H * W)), G


def seg_grad(seg_pred, mask, go=1.0):
    """(gradient float32, the same before its rounding)."""
    z, label, m, e, s, rest = _softmax_parts(seg_pred, mask)
    B, C, H, W = z.shape
    N, go = F64(B * H * W), F64(F32(go))
    g = np.empty(z.shape, F64)
    for c in range(C):
        g[:, c] = np.where(label == c, ((-go * rest) / s) / N, ((go * e[:, c]) / s) / N)
    return g.astype(F32), g


# ------------------------------------------------------------------------------------------------ the bounds
def vote_bound_f64(want):
    return 8 * U * abs(want)


def vote_bound_f32(want, elements):
    n = elements + 8
    if n * U >= 1:                                                 # the any-order bound says nothing from 2^24 terms on
        return np.inf
    return n * U / (1 - n * U) * abs(want)


def seg_bound_f64(want):
    return 2 * U * abs(want)


def seg_bound_f32(want, pixels, C, zmax):
    n = pixels + 2
    if n * U >= 1:
        return np.inf
    return n * U / (1 - n * U) * abs(want) + (C + 6) * U * (zmax + np.log(C))


def seg_grad_bound_f64(C, zrange, go, N):
    return (2 * (C + 6) + 2 * (zrange + np.log(C))) * V * abs(go) / N


def vote_grad_bound_f32(g):
    return 8 * U * np.abs(g)


def seg_grad_bound_f32(C, zrange, go, N):
    return 2 * ((C + 8) + (zrange + np.log(C))) * U * abs(go) / N


def ulp_apart(a, b):
    """How many float32 values lie between a and b (0: the same bits but for the sign of zero); NaN only equals NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if np.isnan(a).any() or np.isnan(b).any():
        assert np.array_equal(np.isnan(a), np.isnan(b))
        a, b = np.where(np.isnan(a), F32(0), a), np.where(np.isnan(b), F32(0), b)
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------ the cases
def issue_kpts(mask_b, K, rng):
    """K keypoints for one image: the first three lie on a foreground pixel's centre, 5e-4 px and 1.5e-3 px from one."""
    H, W = mask_b.shape
    kpt = np.stack([rng.uniform(-5, W + 5, K), rng.uniform(-5, H + 5, K)], 1)
    fg = np.argwhere(mask_b == 1)
    if len(fg) and K >= 3:
        (y0, x0), (y1, x1), (y2, x2) = fg[len(fg) // 3], fg[len(fg) // 2], fg[2 * len(fg) // 3]
        kpt[0] = [x0, y0]
        kpt[1] = [x1 + 5e-4, y1]
        kpt[2] = [x2, y2 - 1.5e-3]
    return kpt


def blob_mask(B, H, W, rng, labels=1, empty=()):
    """uint8 masks: an ellipse of label 1 per image (labels up to ``labels`` in bands inside it); images in ``empty`` are zeros."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        if b in empty:
            continue
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        inside = ((y - cy) / (0.3 * H)) ** 2 + ((x - cx) / (0.35 * W)) ** 2 < 1
        m[b][inside] = 1
        for lab in range(2, labels + 1):
            m[b][inside & (x % (2 * labels) == lab)] = lab
    return m


def make_inputs(B, K, C, H, W, seed, empty=(), kpt_dtype=F64):
    """Seeded inputs of a case: predictions with saturated elements on both sides (|d| > 1) and logits up to +-40."""
    rng = np.random.default_rng(seed)
    mask = blob_mask(B, H, W, rng, labels=C - 1, empty=empty)
    kpt = np.stack([issue_kpts(mask[b], K, rng) for b in range(B)]).astype(kpt_dtype)
    target = compute_vertex(mask, kpt)
    vp = (target + rng.standard_normal(target.shape).astype(F32) * F32(0.3)).astype(F32)
    far = rng.random(target.shape) < 0.03
    vp[far] = (rng.choice([-1, 1], int(far.sum())) * rng.uniform(1.2, 4.0, int(far.sum()))).astype(F32)
    sp = (rng.standard_normal((B, C, H, W)) * 3).astype(F32)
    big = rng.random((B, H, W)) < 0.02
    sp[:, 0][big], sp[:, C - 1][big] = F32(40), F32(-40)
    big = rng.random((B, H, W)) < 0.02
    sp[:, 0][big], sp[:, C - 1][big] = F32(-40), F32(40)
    return {"mask": mask, "kpt_2d": kpt, "vertex_pred": vp, "seg_pred": sp, "target": target}


# name -> (B, K, C, H, W, seed, empty images): the cases of tests/golden/train_<name>.npz
GOLDEN_CASES = {
    "k9_c2_37x53": (2, 9, 2, 37, 53, 11, ()),
    "k1_c3_8x12": (1, 1, 3, 8, 12, 12, ()),
    "empty_beside": (2, 2, 2, 9, 10, 13, (0,)),
}


def golden_inputs(name):
    B, K, C, H, W, seed, empty = GOLDEN_CASES[name]
    return make_inputs(B, K, C, H, W, seed, empty)


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, "train_%s.npz" % name)))


# name -> (B, K, C, H, W, seed, empty images): the shapes of the GPU tests, the smallest that reach every path --
# 37x53: H*W odd, the scalar form, one full and one partial tile; 40x64: the 16-byte form, 2.5 tiles; 480x640: 300 tiles, so an
# image slot sums two; B = 3 with an empty mask
GPU_CASES = {
    "scalar_37x53": (2, 9, 2, 37, 53, 21, ()),
    "vec_40x64": (2, 9, 3, 40, 64, 22, ()),
    "slots_480x640": (1, 1, 2, 480, 640, 23, ()),
    "empty_of_three": (3, 1, 3, 40, 64, 24, (1,)),
}
_cache = {}


def reference(name):
    """The inputs of a GPU case with the twin's results, computed once and shared; treat as read-only."""
    if name not in _cache:
        B, K, C, H, W, seed, empty = GPU_CASES[name]
        d = make_inputs(B, K, C, H, W, seed, empty, kpt_dtype=F32 if name == "vec_40x64" else F64)
        d["vote_loss"], d["S"] = vote_loss(d["vertex_pred"], d["target"], d["mask"])
        d["vote_grad"] = vote_grad(d["vertex_pred"], d["target"], d["mask"])
        d["seg_loss"], d["G"] = seg_loss(d["seg_pred"], d["mask"])
        d["seg_grad"], d["seg_grad64"] = seg_grad(d["seg_pred"], d["mask"])
        d.update(B=B, K=K, C=C, H=H, W=W)
        _cache[name] = d
    return _cache[name]
