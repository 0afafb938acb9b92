"""The numpy twin of the output head's bfloat16 matrix-core modes (include/pvnet_vote.h, "PVNet output head", the compute modes).
It builds on tests/head_twin.py and changes nothing there.

The operands are stated bit for bit; the order of the two float32 sums is not.  So ``forward`` returns
  out64       steps 1-6 of the contract in binary64 on the bit-exact operands -- u the float32 upsample of head_twin, every
              operand of the two convolutions rounded (``bfloat16``) or split (``bfloat16x3``: hi = bf16(v), lo = bf16(v - hi), the
              products hi*hi + hi*lo + lo*hi) -- with step 4, t and a, rounded to float32.  A product of two bfloat16 values has 16
              bits: every product is exact in binary64 and the sum of n of them carries at most n * 2^-53 of their magnitude.
  bound_acc   how far a device that sums in ANY order in float32 may lie from out64 (u = 2^-24, gamma_n = n*u / (1 - n*u)):
      e1     gamma_(n1-1) * S1, S1 = sum |product| over the n1 = pieces * 9 * C products of conv1 (pieces = 1 or 3): any-order
             float32 summation of n1 terms from +0 takes n1 - 1 additions
      e_t    d + 2u * (|t| + d), d = |scale| * e1: the device's float32 t is the rounding of a value within d of the twin's
      e_a    max(1, |slope|) * e_t + 2u * |slope| * (|t| + e_t): LeakyReLU and the rounding of its product
      e_op   what the device's conv2 operand may differ by from the twin's.  Rounding is monotone, so the device's hi piece lies
             between bf16(a - e_a) and bf16(a + e_a): dhi = the larger distance of the two from the twin's hi -- zero unless a
             rounding boundary lies within e_a of a, one bfloat16 ulp (plus e_a) where one does.  ``bfloat16``: the operand is
             hi, the term |w2_hi| * dhi.  ``bfloat16x3``: the operand pair enters as w2_hi * (hi + lo) + w2_lo * hi;
             hi + lo = a - r with |r| <= 2^-18 |a| on both sides (lo's own ulp: half of 2^-8 of |lo| <= 2^-9 |a|), so the term is
             |w2_hi| * (e_a + 2^-17 * (|a| + e_a)) + |w2_lo| * dhi
      e2     gamma_(n2-1) * (|bias2| + S2 + e_op) + e_op, n2 = pieces * M1 + 1 terms with the bias
      and 2^-40 of the magnitudes for the binary64 evaluation's own roundings.
  bound_mode  out64's distance from the true function ``head_twin.forward64``: |out64 - G| + |G - forward64|, G being steps 1-6 in
              binary64 on the UNROUNDED operands (the float32 u, scale and shift, t and a rounded to float32: what out64 shares
              with every float32 evaluation).  |G - forward64| is evaluated, not bounded -- both are functions of the inputs
              alone --; |out64 - G| is bounded term by term
      rho    the relative error of one operand: 2^-9 for ``bfloat16`` (half an ulp of 8 bits); for ``bfloat16x3`` a product
             v*w = (hi+lo+r)(hi'+lo'+r') misses lo*lo' and the residuals: at most 2^-18 + 2 * 2^-18 * (1 + 2^-9) < 2^-16
             relative to |v*w| (|lo| <= 2^-9 |v|, |r| <= 2^-18 |v|), written as rho = 2^-17 per operand
      m_acc  (2*rho + rho^2) * |weight1| . |z|
      m_t    |scale| * m_acc + 2u * (|t| + |scale| * m_acc)       (t is rounded to float32 in out64 and in G)
      m_a    max(1, |slope|) * m_t + 2u * |slope| * (|t| + m_t)
      m_out  (2*rho + rho^2) * |weight2| . (|a| + m_a) + |weight2| . m_a
Non-finite values come out of the binary64 arithmetic as they do on the device: NaN in, NaN out; in ``bfloat16x3`` an Inf operand has
lo = NaN, which is why only the set of non-finite outputs is pinned there.

CASES: head_twin's with their plants -- but the last output row's weights of 2e38 against a bias of -3e38, finite only in
one summation order, are ordinary draws again -- and ``c16`` / ``c17``: C = 16, exactly one K-step of 16 channels, and one channel
more.  EXACT_CASES: inputs whose every partial sum has fewer than 24 bits, so that any order gives out64's bits.
"""
import functools

import numpy as np

from tests import head_twin as ht
from tests.head_twin import F32, U, canon, same_bits, to_bf16, to_f16  # noqa: F401  (re-exported for the tests)

MODES = ("bfloat16", "bfloat16x3")
DEVICE_MODES = ("bfloat16",)       # what ``pvnet_head(compute=...)`` offers: the split mode measured slower than the float32 kernel
KEYS = ("fm", "x", "weight1", "scale", "shift", "weight2", "bias2")


def bf16(v, rounding="nearest"):
    """float32 ``v`` rounded to bfloat16, as float32.  ``rounding="truncate"`` is the mutation."""
    v = np.ascontiguousarray(np.asarray(v, F32))
    if rounding == "nearest":
        bits = to_bf16(v).astype(np.uint32) << np.uint32(16)
    else:
        bits = v.view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(F32).reshape(v.shape)


def split(v, mode, rounding="nearest", keep_lo=True, rounded=True):
    """(hi, lo) float32; lo is None for ``bfloat16``.  ``rounded=False`` leaves the operand as it is (a mutation), ``keep_lo=False``
    drops lo."""
    v = np.asarray(v, F32)
    if not rounded:
        return v, None
    hi = bf16(v, rounding)
    if mode == "bfloat16" or not keep_lo:
        return hi, None
    with np.errstate(invalid="ignore", over="ignore"):
        return hi, bf16((v - hi).astype(F32), rounding)


def _products(w, z, drop=None):
    """The (weight piece, operand piece) pairs of one convolution as binary64 arrays: hi*hi, then hi*lo and lo*hi."""
    (wh, wl), (zh, zl) = w, z
    pairs = [(wh, zh)]
    if zl is not None:
        pairs.append((wh, zl))
    if wl is not None:
        pairs.append((wl, zh))
    if drop is not None and len(pairs) == 3:
        del pairs[drop]
    return [(a.astype(np.float64), b.astype(np.float64)) for a, b in pairs]


def _gemm(pairs, absolute=False):
    f = np.abs if absolute else (lambda a: a)
    with np.errstate(invalid="ignore", over="ignore"):
        return sum(np.einsum("mk,bkp->bmp", f(a), f(b)) for a, b in pairs)


def _gamma(n):
    return max(n, 0) * U / (1 - max(n, 0) * U)


def sum32(pairs, start, order="ascending", seed=0):
    """One float32 evaluation of a convolution: every product exact (binary64, then float32: 16 bits), added one at a time in
    float32 to ``start`` [M] or None (+0); ``order`` is ascending, descending or a seeded permutation of all the terms."""
    terms = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in pairs:
            terms.extend((a[None, :, k, None] * b[:, None, k, :]).astype(F32) for k in range(a.shape[1]))
        if start is not None:
            terms.insert(0, np.broadcast_to(np.asarray(start, F32)[None, :, None], terms[0].shape))
        idx = list(range(len(terms)))
        if order == "descending":
            idx.reverse()
        elif order != "ascending":
            idx = list(np.random.default_rng(seed).permutation(len(terms)))
        acc = np.zeros(terms[0].shape, F32)
        for i in idx:
            acc = (acc + terms[i]).astype(F32)
    return acc


def forward(fm, x, weight1, scale, shift, weight2, bias2, slope=0.1, mode="bfloat16", *, rounding="nearest", keep_lo=True,
            drop=None, round_w1=True, round_a=True, round_bias=False, unrounded=False, order=None, seed=0):
    """dict(out64, bound_acc, t, a) [B, M, 2h, 2w]; with ``order`` also ``out32``, the twin's own float32 evaluation in that
    order.  The keyword flags after ``mode`` state one rule wrongly each, for the mutation tests; ``unrounded`` leaves every
    operand as it is: the function ``bound_mode`` measures from."""
    assert mode in MODES
    if unrounded:
        round_w1 = round_a = False
    fm, x = np.asarray(fm, F32), np.asarray(x, F32)
    u = ht.upsample(fm)
    B, _, H, W = u.shape
    col = ht.im2col(np.concatenate([u, x], axis=1))                                          # [B, K, P], k = c*9 + tap
    w1 = np.asarray(weight1, F32)
    M1 = w1.shape[0]
    w2 = np.asarray(weight2, F32).reshape(-1, M1)
    sc = np.asarray(scale, F32).astype(np.float64)[None, :, None]
    sh = np.asarray(shift, F32).astype(np.float64)[None, :, None]
    b2 = np.asarray(bias2, F32)
    if round_bias:
        b2 = bf16(b2)
    sl = F32(slope)
    with np.errstate(invalid="ignore", over="ignore"):
        p1 = _products(split(w1.reshape(M1, -1), mode, rounding, keep_lo, round_w1), split(col, mode, rounding, keep_lo, not unrounded), drop)
        acc1, S1 = _gemm(p1), _gemm(p1, absolute=True)
        n1 = len(p1) * col.shape[1]
        e1 = _gamma(n1 - 1) * S1 + 2.0 ** -40 * S1
        t = (acc1 * sc + sh).astype(F32)
        a = np.where(t > 0, t, t * sl).astype(F32)
        ta = np.abs(t.astype(np.float64))
        d = np.abs(sc) * e1
        e_t = d + 2 * U * (ta + d)
        e_a = max(1.0, abs(float(sl))) * e_t + 2 * U * abs(float(sl)) * (ta + e_t)
        za = split(a, mode, rounding, keep_lo, round_a)
        wz = split(w2, mode, rounding, keep_lo, not unrounded)
        p2 = _products(wz, za, drop)
        out64 = b2.astype(np.float64)[None, :, None] + _gemm(p2)
        S2 = np.abs(b2.astype(np.float64))[None, :, None] + _gemm(p2, absolute=True)
        # what the device's operand may differ by
        a64 = a.astype(np.float64)
        lo_a, hi_a = (a64 - e_a).astype(F32), (a64 + e_a).astype(F32)                        # outward enough: e_a >= 2u|a| wherever t != 0
        lo_a, hi_a = np.nextafter(lo_a, F32(-np.inf)), np.nextafter(hi_a, F32(np.inf))
        hi = za[0].astype(np.float64)
        dhi = np.maximum(np.abs(bf16(lo_a).astype(np.float64) - hi), np.abs(bf16(hi_a).astype(np.float64) - hi))
        dhi = np.where(np.isfinite(dhi), dhi, e_a + 2.0 ** -7 * (np.abs(a64) + e_a))
        wh = np.abs(wz[0].astype(np.float64))
        if mode == "bfloat16":
            e_op = np.einsum("om,bmp->bop", wh, dhi)
        else:
            wl = np.abs(wz[1].astype(np.float64)) if wz[1] is not None else 0 * wh
            e_op = np.einsum("om,bmp->bop", wh, e_a + 2.0 ** -17 * (np.abs(a64) + e_a)) + np.einsum("om,bmp->bop", wl, dhi)
        n2 = len(p2) * M1 + 1
        bound_acc = _gamma(n2 - 1) * (S2 + e_op) + e_op + 2.0 ** -40 * S2
        bound_acc = np.where(np.isfinite(out64), bound_acc, np.nan)
    shape = (B, -1, H, W)
    res = dict(out64=out64.reshape(shape), bound_acc=bound_acc.reshape(shape), t=t.reshape(shape), a=a.reshape(shape))
    if order is not None:
        acc32 = sum32(p1, None, order, seed)
        with np.errstate(invalid="ignore", over="ignore"):
            t32 = ht.fmaf(acc32, sc.astype(F32), sh.astype(F32)).reshape(acc32.shape)
            a32 = np.where(t32 > 0, t32, t32 * sl).astype(F32)
        p2_32 = _products(wz, split(a32, mode, rounding, keep_lo, round_a), drop)
        res["out32"] = sum32(p2_32, b2, order, seed + 1).reshape(shape)
    return res


def bound_mode(fm, x, weight1, bn, weight2, bias2, slope=0.1, mode="bfloat16"):
    """(true64, bound) [B, M2, 2h, 2w]: ``head_twin.forward64``'s function and ``out64``'s distance from it, the module
    docstring's m_out plus |G - forward64|."""
    assert mode in MODES
    rho = 2.0 ** -9 if mode == "bfloat16" else 2.0 ** -17
    r2 = 2 * rho + rho * rho
    true64, _ = ht.forward64(fm, x, weight1, bn, weight2, bias2, slope)
    B, M2, H, W = true64.shape
    gamma, beta, mean, var, eps = bn
    scale, shift = ht.fold_bn(gamma, beta, mean, var, eps)
    w1 = np.asarray(weight1, F32).astype(np.float64)
    M1 = w1.shape[0]
    w1 = w1.reshape(M1, -1)
    w2 = np.asarray(weight2, F32).astype(np.float64).reshape(-1, M1)
    col = ht.im2col(np.concatenate([ht.upsample(fm), np.asarray(x, F32)], axis=1)).astype(np.float64)
    sc, sh = scale.astype(np.float64)[None, :, None], shift.astype(np.float64)[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.einsum("mk,bkp->bmp", w1, col)
        m_acc = r2 * np.einsum("mk,bkp->bmp", np.abs(w1), np.abs(col))
        t = acc * sc + sh
        m_t = np.abs(sc) * m_acc + 2 * U * (np.abs(t) + np.abs(sc) * m_acc)
        a = np.where(t > 0, t, t * slope)
        m_a = max(1.0, abs(slope)) * m_t + 2 * U * abs(slope) * (np.abs(t) + m_t)
        m_out = r2 * np.einsum("om,bmp->bop", np.abs(w2), np.abs(a) + m_a) + np.einsum("om,bmp->bop", np.abs(w2), m_a)
        G = forward(fm, x, weight1, scale, shift, weight2, bias2, slope, mode, unrounded=True)["out64"]
        shared = np.abs(G - true64)
    return true64, (shared + m_out.reshape(B, M2, H, W)) * (1 + 2.0 ** -20)


def nonfinite_sets_match(got, want, mode):
    """The contract's rule: ``bfloat16`` pins the NaN set and the +-Inf sets; ``bfloat16x3`` only the set of non-finite outputs."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if mode == "bfloat16x3":
        return np.array_equal(np.isfinite(got), np.isfinite(want))
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
            and np.array_equal(np.isneginf(got), np.isneginf(want)))


def within(got, ref, mode):
    """Whether float32 ``got`` lies within ``bound_acc`` of ``ref["out64"]`` where that is finite and has its non-finite sets."""
    got = np.asarray(got, F32).astype(np.float64)
    f = np.isfinite(ref["out64"])
    with np.errstate(invalid="ignore"):
        ok = np.abs(got[f] - ref["out64"][f]) <= ref["bound_acc"][f]
    return bool(ok.all()) and nonfinite_sets_match(got, ref["out64"], mode)


def worst(got, ref):
    """The largest |got - out64| / bound_acc over the finite outputs, for the tests' printed figures."""
    got = np.asarray(got, F32).astype(np.float64)
    f = np.isfinite(ref["out64"]) & np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.abs(got[f] - ref["out64"][f]) / np.maximum(ref["bound_acc"][f], 1e-300))) if f.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ cases
CASES = dict(ht.CASES,
             c16=dict(B=1, C2=13, C0=3, h=5, w=6, M1=8, M2=4),                    # C = 16: exactly one K-step
             c17=dict(B=1, C2=14, C0=3, h=5, w=6, M1=8, M2=4))                    # one channel over: a K-step's padding
EXACT_CASES = {"exact_reference_channels": "reference_channels", "exact_two_blocks": "two_blocks"}
EXACT_SLOPE = 0.125


def make_inputs(name):
    """head_twin's tensors and plants for its cases, the last output row drawn again; ``c16`` and ``c17`` by the same recipe."""
    if name in ht.CASES:
        d = ht.make_inputs(name)
        if d["M1"] >= 5:
            rng = np.random.default_rng(sorted(ht.CASES).index(name) + 70261)
            d["weight2"][d["M2"] - 1] = (rng.standard_normal((d["M1"], 1, 1)) / np.sqrt(d["M1"])).astype(F32)
            d["bias2"][d["M2"] - 1] = F32(rng.standard_normal())
        return d
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 80261)
    B, C2, C0, h, w, M1, M2 = (c[k] for k in ("B", "C2", "C0", "h", "w", "M1", "M2"))
    C = C2 + C0
    d = dict(c, fm=rng.standard_normal((B, C2, h, w)).astype(F32), x=rng.standard_normal((B, C0, 2 * h, 2 * w)).astype(F32),
             weight1=(rng.standard_normal((M1, C, 3, 3)) / np.sqrt(9 * C)).astype(F32), gamma=rng.uniform(0.5, 1.5, M1).astype(F32),
             beta=rng.standard_normal(M1).astype(F32), mean=(0.1 * rng.standard_normal(M1)).astype(F32),
             var=rng.uniform(0.5, 1.5, M1).astype(F32), eps=ht.EPS,
             weight2=(rng.standard_normal((M2, M1, 1, 1)) / np.sqrt(M1)).astype(F32), bias2=rng.standard_normal(M2).astype(F32))
    d["fm"][0, 0, 1, 1], d["fm"][0, C2 - 1, 2, 2] = np.nan, np.inf
    d["gamma"][0], d["beta"][0], d["mean"][0] = 0, -0.0, 0.5
    d["var"][1] = 0
    d["bias2"][0] = 70000
    return d


def make_exact_inputs(name):
    """An exact-sum case at the sizes of ``EXACT_CASES[name]``: fm uniform in [1.25, 1.75] (bf16(u) is a multiple of 2^-7 in [1, 2)),
    x = +-[1, 2), weight1 multiples of 1/4 in [-1, 1], scale = 2^-6, shift = 3 * 2^-9, slope 0.125, weight2 one entry of +-1 or
    +-1/2 per row at a column that differs from row to row, bias2 = 0: the products are multiples of 2^-9 and every sum stays
    below 2^10 in magnitude, so fewer than 24 bits in any order."""
    c = ht.CASES[EXACT_CASES[name]]
    rng = np.random.default_rng(sorted(EXACT_CASES).index(name) + 90261)
    B, C2, C0, h, w, M1, M2 = (c[k] for k in ("B", "C2", "C0", "h", "w", "M1", "M2"))
    fm = rng.uniform(1.25, 1.75, (B, C2, h, w)).astype(F32)
    x = (rng.uniform(1, 2, (B, C0, 2 * h, 2 * w)) * rng.choice([-1.0, 1.0], (B, C0, 2 * h, 2 * w))).astype(F32)
    weight1 = (rng.integers(-4, 5, (M1, C2 + C0, 3, 3)) / 4.0).astype(F32)
    weight2 = np.zeros((M2, M1, 1, 1), F32)
    cols = (np.arange(M2) * 7 + 3) % M1 if M2 <= M1 else (np.arange(M2) + 5) % M1         # distinct while M2 <= M1 (7 is coprime to 32, 5)
    weight2[np.arange(M2), cols, 0, 0] = rng.choice([1.0, -1.0, 0.5, -0.5], M2)
    return dict(c, fm=fm, x=x, weight1=weight1, scale=np.full(M1, 2.0 ** -6, F32), shift=np.full(M1, 3 * 2.0 ** -9, F32),
                weight2=weight2, bias2=np.zeros(M2, F32), slope=EXACT_SLOPE)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs with the folded ``scale`` / ``shift``, ``slope``, and per mode ``forward``'s dict with ``out32``, the
    ascending float32 evaluation: computed once, shared, not to be written to."""
    if name in EXACT_CASES:
        d = make_exact_inputs(name)
    else:
        d = make_inputs(name)
        d["scale"], d["shift"] = ht.fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
        d["slope"] = 0.1
    for mode in MODES:
        d[mode] = forward(*(d[k] for k in KEYS), d["slope"], mode, order="ascending")
    return _freeze(d)
