"""The numpy twin of the decoder stage's bfloat16 matrix-core mode (include/pvnet_vote.h, "PVNet decoder stage", compute mode:
``PVV_HEAD_STAGE_BF16`` beside ``PVV_HEAD_STAGE``).  It builds on tests/head_bf16_twin.py (``bf16``, ``split``, ``_products``,
``_gemm``, ``_gamma``, ``sum32``'s rule) and tests/decoder_twin.py (the cases and their input recipe) and changes nothing there.

The operands are stated bit for bit; the order of the float32 sum is not.  So ``stage`` returns
  a64         the contract's steps in binary64 on the bit-exact operands -- u the float32 upsample of head_twin (or u = a), z =
              cat([u, skip]) in its ring of zeros, z and weight each rounded once to bfloat16 -- with t and a rounded to float32.
              A product of two bfloat16 values has 16 bits: every product is exact in binary64.
  bound_acc   how far a device that sums in ANY order in float32 may lie from a64: head_bf16_twin's e_a (u = 2^-24)
      e1     gamma_(n-1) * S1, S1 = sum |product| over the n = 9 * C products
      e_t    d + 2u * (|t| + d), d = |scale| * e1
      e_a    max(1, |slope|) * e_t + 2u * |slope| * (|t| + e_t)
      and 2^-40 of the magnitudes for the binary64 evaluation's own roundings.
  and, with ``order``, ``a32``: the twin's own float32 evaluation, the products added one at a time in ascending order,
  descending order or a seeded permutation.
``within`` holds a float32 result to |got - a64| <= bound_acc; a float16 / bfloat16 result to the interval between the store's
rounding of a64 - bound_acc and of a64 + bound_acc (rounding is monotone).  The NaN, +Inf and -Inf sets are a64's.
``bound_mode`` is a64's distance from the true function ``decoder_twin.stage64``: |a64 - G| + |G - stage64|, G the steps in
binary64 on the UNROUNDED operands; |G - stage64| is evaluated, |a64 - G| bounded with rho = 2^-9 per operand:
      m_acc  (2*rho + rho^2) * |weight| . |z|
      m_t    |scale| * m_acc + 2u * (|t| + |scale| * m_acc)
      m_a    max(1, |slope|) * m_t + 2u * |slope| * (|t| + m_t)

CASES: decoder_twin's nine, and
  c16, c17            C = 16, exactly one k-step of 16 channels, and one channel more
  straddle            C2 = 11, C0 = 9: the second group of eight holds three of a's channels and five of skip's
  c32, c33            the kernel's channel chunk at one and two row blocks per workgroup, and one channel more
  wide_*              256 tiles, below which the launch splits M over more workgroups: the workgroups of four row blocks
                      (M = 65, chunk 16: C = 16 and C = 17) and of two (M = 33), with and without the upsample; images 34
                      wide, so every second tile is two pixels of one
EXACT_CASES: inputs whose every partial sum has fewer than 24 bits, so that any order gives a64's bits -- head_bf16_twin's
``make_exact_inputs`` as the pattern -- one with the upsample and one without, C = 35: two chunks and a straddling group.
"""
import functools

import numpy as np

from tests import decoder_twin as dt
from tests import head_bf16_twin as hb
from tests import head_twin as ht
from tests.head_twin import F32, U, same_bits, to_bf16, to_f16  # noqa: F401  (re-exported for the tests)

KEYS = ("a", "skip", "weight", "scale", "shift")
ORDERS = ("ascending", "descending", "permuted")


def sum32(pairs, order="ascending", seed=0):
    """``head_bf16_twin.sum32`` from +0 without its list of all terms (K of them, [B, M, P] each): every product exact (binary64,
    then float32: 16 bits), added one at a time in float32 in ascending, descending or a seeded permutation's order."""
    (a, b), = pairs
    idx = list(range(a.shape[1]))
    if order == "descending":
        idx.reverse()
    elif order != "ascending":
        idx = list(np.random.default_rng(seed).permutation(len(idx)))
    acc = np.zeros((b.shape[0], a.shape[0], b.shape[2]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in idx:
            acc = (acc + (a[None, :, k, None] * b[:, None, k, :]).astype(F32)).astype(F32)
    return acc


def stage(a, skip, weight, scale, shift, slope=0.1, *, up=True, rounding="nearest", round_w=True, round_z=True, coords="align",
          ring="zero", channels="a_skip", crop=False, order=None, seed=0):
    """dict(a64, bound_acc, t) [B, M, H, W]; with ``order`` also ``a32``.  The keyword flags after ``up`` state one rule wrongly
    each, for the mutation tests (``crop``: decoder_twin.stage's -- an upsample where the same resolution was meant);
    ``round_w = round_z = False`` is the function ``bound_mode`` measures from."""
    a, skip = np.asarray(a, F32), np.asarray(skip, F32)
    u = ht.upsample(a, coords=coords) if up or crop else a
    if crop:
        u = u[:, :, :a.shape[2], :a.shape[3]]
    B, _, H, W = u.shape
    z = np.concatenate([u, skip] if channels == "a_skip" else [skip, u], axis=1)
    col = ht.im2col(z, ring)                                                                 # [B, K, P], k = c*9 + tap
    w = np.asarray(weight, F32)
    M = w.shape[0]
    sc = np.asarray(scale, F32).astype(np.float64)[None, :, None]
    sh = np.asarray(shift, F32).astype(np.float64)[None, :, None]
    sl = F32(slope)
    with np.errstate(invalid="ignore", over="ignore"):
        p = hb._products(hb.split(w.reshape(M, -1), "bfloat16", rounding, True, round_w), hb.split(col, "bfloat16", rounding, True, round_z))
        acc, S1 = hb._gemm(p), hb._gemm(p, absolute=True)
        e1 = hb._gamma(col.shape[1] - 1) * S1 + 2.0 ** -40 * S1
        t = (acc * sc + sh).astype(F32)
        a_out = np.where(t > 0, t, t * sl).astype(F32)
        ta = np.abs(t.astype(np.float64))
        d = np.abs(sc) * e1
        e_t = d + 2 * U * (ta + d)
        e_a = max(1.0, abs(float(sl))) * e_t + 2 * U * abs(float(sl)) * (ta + e_t)
        a64 = a_out.astype(np.float64)
        bound = np.where(np.isfinite(a64), e_a, np.nan)
    shape = (B, M, H, W)
    res = dict(a64=a64.reshape(shape), bound_acc=bound.reshape(shape), t=t.reshape(shape))
    if order is not None:
        acc32 = sum32(p, order, seed)
        with np.errstate(invalid="ignore", over="ignore"):
            t32 = ht.fmaf(acc32, sc.astype(F32), sh.astype(F32)).reshape(acc32.shape)
            res["a32"] = np.where(t32 > 0, t32, t32 * sl).astype(F32).reshape(shape)
    return res


def bound_mode(a, skip, weight, bn, slope=0.1, *, up=True):
    """(true64, bound) [B, M, H, W]: ``decoder_twin.stage64``'s function and ``a64``'s distance from it, the module docstring's
    m_a plus |G - stage64|."""
    rho = 2.0 ** -9
    r2 = 2 * rho + rho * rho
    true64, _ = dt.stage64(a, skip, weight, bn, slope, up=up)
    gamma, beta, mean, var, eps = bn
    scale, shift = ht.fold_bn(gamma, beta, mean, var, eps)
    a, skip = np.asarray(a, F32), np.asarray(skip, F32)
    w = np.asarray(weight, F32).astype(np.float64)
    M = w.shape[0]
    w = w.reshape(M, -1)
    col = ht.im2col(np.concatenate([ht.upsample(a) if up else a, skip], axis=1)).astype(np.float64)
    sc, sh = scale.astype(np.float64)[None, :, None], shift.astype(np.float64)[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.einsum("mk,bkp->bmp", w, col)
        m_acc = r2 * np.einsum("mk,bkp->bmp", np.abs(w), np.abs(col))
        t = acc * sc + sh
        m_t = np.abs(sc) * m_acc + 2 * U * (np.abs(t) + np.abs(sc) * m_acc)
        m_a = max(1.0, abs(slope)) * m_t + 2 * U * abs(slope) * (np.abs(t) + m_t)
        G = stage(a, skip, weight, scale, shift, slope, up=up, round_w=False, round_z=False)["a64"]
        shared = np.abs(G - true64)
    return true64, (shared + m_a.reshape(true64.shape)) * (1 + 2.0 ** -20)


def nonfinite_sets_match(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


def _outward(v64, direction):
    """float64 ``v64`` as a float32 that is not on the inner side of it."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = v64.astype(F32)
        off = (v.astype(np.float64) > v64) if direction < 0 else (v.astype(np.float64) < v64)
        return np.where(off, np.nextafter(v, F32(direction * np.inf)), v)


def rounded(v, kind):
    """float32 ``v`` through the store of output type ``kind`` ("float32", "float16", "bfloat16"), as float64."""
    if kind == "float32":
        return np.asarray(v, F32).astype(np.float64)
    if kind == "float16":
        return to_f16(v).astype(np.float64)
    return (to_bf16(v).astype(np.uint32) << np.uint32(16)).view(F32).reshape(np.shape(v)).astype(np.float64)


def within(got, ref, kind="float32"):
    """Whether ``got`` -- the device's values as float32 or float64, of output type ``kind`` -- lies within ``bound_acc`` of
    ``ref["a64"]`` where that is finite (for the half types: between the two rounded ends of the interval) and has its
    non-finite sets (those of a64 through the same store: a half type's overflow is an Inf of the twin's too)."""
    got = np.asarray(got).astype(np.float64)
    a64, bound = ref["a64"], ref["bound_acc"]
    f = np.isfinite(a64)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "float32":
            ok = np.abs(got[f] - a64[f]) <= bound[f]
            return bool(ok.all()) and nonfinite_sets_match(got, a64)
        lo, hi = rounded(_outward(a64[f] - bound[f], -1), kind), rounded(_outward(a64[f] + bound[f], +1), kind)
        ok = (lo <= got[f]) & (got[f] <= hi)
        return bool(ok.all()) and nonfinite_sets_match(got[~f], a64[~f])


def worst(got, ref):
    """The largest |got - a64| / bound_acc over the finite outputs, for the tests' printed figures."""
    got = np.asarray(got, F32).astype(np.float64)
    f = np.isfinite(ref["a64"]) & np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.abs(got[f] - ref["a64"][f]) / np.maximum(ref["bound_acc"][f], 1e-300))) if f.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ cases
CHUNK = 32                         # channels of the kernel's chunk at one and two row blocks per workgroup; 16 at four
FILL = 256                         # tiles from which the launch keeps all of M's row blocks in one workgroup
OWN_CASES = {
    "c16": dict(B=1, C2=13, C0=3, h=5, w=6, M=8, up=True),
    "c17": dict(B=1, C2=14, C0=3, h=5, w=6, M=8, up=True),
    "straddle": dict(B=1, C2=11, C0=9, h=5, w=6, M=5, up=True),
    "c32": dict(B=1, C2=20, C0=12, h=5, w=6, M=40, up=True),
    "c33": dict(B=1, C2=20, C0=13, h=9, w=35, M=8, up=False),
    "wide_c16_up": dict(B=16, C2=13, C0=3, h=32, w=17, M=65, up=True),
    "wide_c17_same": dict(B=16, C2=14, C0=3, h=64, w=34, M=65, up=False),
    "wide_two_up": dict(B=16, C2=3, C0=2, h=32, w=17, M=33, up=True),
    "wide_two_same": dict(B=16, C2=2, C0=3, h=64, w=34, M=33, up=False),
}
CASES = dict(dt.CASES, **OWN_CASES)
EXACT_CASES = {
    "exact_up": dict(B=1, C2=13, C0=22, h=5, w=9, M=40, up=True),
    "exact_same": dict(B=2, C2=21, C0=14, h=9, w=35, M=97, up=False),
}
EXACT_SLOPE = 0.125


def make_inputs(name):
    """decoder_twin's tensors and plants for its cases; this file's by the same recipe."""
    if name in dt.CASES:
        return dt.make_inputs(name)
    c = OWN_CASES[name]
    rng = np.random.default_rng(sorted(OWN_CASES).index(name) + 30270)
    B, C2, C0, h, w, M, up = (c[k] for k in ("B", "C2", "C0", "h", "w", "M", "up"))
    H, W = (2 * h, 2 * w) if up else (h, w)
    a = rng.standard_normal((B, C2, h, w)).astype(F32)
    skip = rng.standard_normal((B, C0, H, W)).astype(F32)
    weight = (rng.standard_normal((M, C2 + C0, 3, 3)) / np.sqrt(9 * (C2 + C0))).astype(F32)
    gamma, beta, mean, var = dt._bn(rng, M)
    a[0, 0, 1, 1], a[0, C2 - 1, 2, 2] = np.nan, np.inf
    return dict(c, H=H, W=W, a=a, skip=skip, weight=weight, gamma=gamma, beta=beta, mean=mean, var=var, eps=dt.EPS, slope=0.1)


def make_exact_inputs(name):
    """An exact-sum case: ``a`` uniform in [1.25, 1.75] (every blend lies there too, so bf16(u) is a multiple of 2^-7 in [1, 2)),
    skip = +-[1, 2), weight multiples of 1/4 in [-1, 1], scale = 2^-6, shift = 3 * 2^-9, slope 0.125: the products are multiples
    of 2^-9 and every partial sum stays below 9 * 35 * 2 < 2^10 in magnitude -- fewer than 24 bits in any order; t and a are
    exact too."""
    c = EXACT_CASES[name]
    rng = np.random.default_rng(sorted(EXACT_CASES).index(name) + 40270)
    B, C2, C0, h, w, M, up = (c[k] for k in ("B", "C2", "C0", "h", "w", "M", "up"))
    H, W = (2 * h, 2 * w) if up else (h, w)
    a = rng.uniform(1.25, 1.75, (B, C2, h, w)).astype(F32)
    skip = (rng.uniform(1, 2, (B, C0, H, W)) * rng.choice([-1.0, 1.0], (B, C0, H, W))).astype(F32)
    weight = (rng.integers(-4, 5, (M, C2 + C0, 3, 3)) / 4.0).astype(F32)
    return dict(c, H=H, W=W, a=a, skip=skip, weight=weight, scale=np.full(M, 2.0 ** -6, F32), shift=np.full(M, 3 * 2.0 ** -9, F32),
                slope=EXACT_SLOPE)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs with the folded ``scale`` / ``shift``, ``slope``, and ``stage``'s dict with ``a32``, the ascending
    float32 evaluation: computed once, shared, not to be written to."""
    if name in EXACT_CASES:
        d = make_exact_inputs(name)
    else:
        d = make_inputs(name)
        d["scale"], d["shift"] = ht.fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    d.update(stage(*(d[k] for k in KEYS), d["slope"], up=d["up"], order="ascending"))
    return dt._frozen(d)
