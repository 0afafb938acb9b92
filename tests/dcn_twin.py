"""The numpy twin of the DCNv2 forward contract (include/pvnet_vote.h, "Modulated deformable convolution"): float32, operation by
operation, no fused multiply-add in the columns and exactly one -- emulated -- per step of the output's chain.

Columns.  For output pixel (y, x), channel c of deformable group g = c / (C/dg) and tap (i, j), t = i*kw + j:
    h = float32(y*stride_h - pad_h + i*dil_h) + offset[b, g*2*kh*kw + 2t, y, x]
    w = float32(x*stride_w - pad_w + j*dil_w) + offset[b, g*2*kh*kw + 2t + 1, y, x]
    not (h > -1 and w > -1 and h < H and w < W)  ->  val = 0        (a NaN offset too)
    else h0 = floor(h), lh = h - h0, hh = 1 - lh; w0, lw, hw alike; v1..v4 the neighbours (h0, w0), (h0, w0+1), (h0+1, w0),
         (h0+1, w0+1), each 0 unless h0 >= 0 / w0 >= 0 / h0+1 <= H-1 / w0+1 <= W-1 hold for its row and column;
         val = (((hh*hw)*v1 + (hh*lw)*v2) + (lh*hw)*v3) + (lh*lw)*v4
    col[k, p] = val * mask[b, g*kh*kw + t, y, x],   k = c*kh*kw + t,   p = y*Wo + x
Output.  acc = bias[o]; for k ascending: acc = fmaf(weight[o, k], col[k, p], acc); out[b, o, p] = acc.

The device may add 0 * 0 terms to fill an instruction, which changes at most the sign of a zero: ``same_bits`` compares bit
patterns after mapping -0 to +0, NaNs by position.
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of float32


# ------------------------------------------------------------------------------------------------------------------- fmaf
def fmaf(a, b, c):
    """float32 fma, exactly: the product of two float32 is exact in binary64 (48 bits); the sum with c is formed with a TwoSum,
    and where its error term is not zero and the sum's last bit is even the sum moves one ulp towards the error (round to odd);
    a round-to-odd binary64 rounds to float32 like the exact value (53 >= 24 + 2 bits)."""
    a, b, c = (np.atleast_1d(np.asarray(v, F32)).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        s = np.ascontiguousarray(s)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


# ---------------------------------------------------------------------------------------------------------------- columns
def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def out_size(H, W, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(kernel), pair(stride), pair(padding), pair(dilation)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def columns(input, offset, mask, kernel, stride=1, padding=0, dilation=1, dg=1, dtype=F32, absolute=False):
    """col [B, C*kh*kw, Ho*Wo].  ``dtype=np.float64`` evaluates the same function in binary64 at the float32 h and w;
    ``absolute`` forms it with |v| and |mask| (the magnitude the error bound is relative to)."""
    x, off, msk = np.asarray(input, F32), np.asarray(offset, F32), np.asarray(mask, F32)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(kernel), pair(stride), pair(padding), pair(dilation)
    B, C, H, W = x.shape
    Ho, Wo = out_size(H, W, kernel, stride, padding, dilation)
    KK, P, Cg = kh * kw, Ho * Wo, C // dg
    assert C % dg == 0 and off.shape == (B, 2 * dg * KK, Ho, Wo) and msk.shape == (B, dg * KK, Ho, Wo), (off.shape, msk.shape)
    off = off.reshape(B, dg, KK, 2, Ho, Wo)
    t = np.arange(KK)
    base_h = (np.arange(Ho) * sh - ph)[None, :] + ((t // kw) * dh)[:, None]                  # [KK, Ho] integers
    base_w = (np.arange(Wo) * sw - pw)[None, :] + ((t % kw) * dw)[:, None]                   # [KK, Wo]
    with np.errstate(invalid="ignore", over="ignore"):
        h = base_h.astype(F32)[None, None, :, :, None] + off[:, :, :, 0]                     # [B, dg, KK, Ho, Wo] float32
        w = base_w.astype(F32)[None, None, :, None, :] + off[:, :, :, 1]
        inside = (h > F32(-1)) & (w > F32(-1)) & (h < F32(H)) & (w < F32(W))
    h, w = np.where(inside, h, F32(0)), np.where(inside, w, F32(0))
    h0, w0 = np.floor(h), np.floor(w)
    one = dtype(1)
    lh, lw = h.astype(dtype) - h0.astype(dtype), w.astype(dtype) - w0.astype(dtype)
    hh, hw = one - lh, one - lw
    h0, w0 = h0.astype(np.int64), w0.astype(np.int64)
    top, left, bottom, right = h0 >= 0, w0 >= 0, h0 + 1 <= H - 1, w0 + 1 <= W - 1
    planes = x.reshape(B, dg, Cg, H * W)

    def corner(dy, dx, ok):
        flat = (np.clip(h0 + dy, 0, H - 1) * W + np.clip(w0 + dx, 0, W - 1)).reshape(B, dg, 1, KK * P)
        v = np.take_along_axis(planes, np.broadcast_to(flat, (B, dg, Cg, KK * P)), axis=3)
        v = np.where((ok & inside).reshape(B, dg, 1, KK * P), v, F32(0)).astype(dtype)
        return np.abs(v) if absolute else v

    def per_tap(a):
        return a.reshape(B, dg, 1, KK * P)

    v1, v2, v3, v4 = corner(0, 0, top & left), corner(0, 1, top & right), corner(1, 0, bottom & left), corner(1, 1, bottom & right)
    val = ((per_tap(hh * hw) * v1 + per_tap(hh * lw) * v2) + per_tap(lh * hw) * v3) + per_tap(lh * lw) * v4
    m = per_tap(msk.reshape(B, dg, KK, Ho, Wo)).astype(dtype)
    col = val * (np.abs(m) if absolute else m)
    assert col.dtype == dtype
    return col.reshape(B, C * KK, P)


# ----------------------------------------------------------------------------------------------------------------- output
def chain(col, weight, bias):
    """out [B, M, P]: per output the fmaf chain over k from the bias."""
    col, wt = np.asarray(col, F32), np.asarray(weight, F32)
    M = wt.shape[0]
    wt = wt.reshape(M, -1)
    B, K, P = col.shape
    assert wt.shape[1] == K
    bs = np.zeros(M, F32) if bias is None else np.asarray(bias, F32)
    acc = np.broadcast_to(bs[None, :, None], (B, M, P)).astype(F32)
    for k in range(K):
        acc = fmaf(wt[None, :, k, None], col[:, None, k, :], acc)
    return acc


def forward(input, offset, mask, weight, bias, stride=1, padding=0, dilation=1, dg=1):
    """out [B, M, Ho, Wo] float32."""
    kernel = tuple(np.shape(weight)[2:])
    Ho, Wo = out_size(np.shape(input)[2], np.shape(input)[3], kernel, stride, padding, dilation)
    out = chain(columns(input, offset, mask, kernel, stride, padding, dilation, dg), weight, bias)
    return out.reshape(out.shape[0], out.shape[1], Ho, Wo)


def forward64(input, offset, mask, weight, bias, stride=1, padding=0, dilation=1, dg=1):
    """(out64, bound) [B, M, Ho, Wo]: the same function in binary64 at the float32 h and w, and the float32 evaluation's
    distance from it.  Every term weight[o,k] * col[k,p] reaches the result through at most 8 roundings inside the column (hh or
    lh -- h - floor(h) is exact for h >= 0, and for h in (-1, 0) only the lh terms have a neighbour --, hw or lw, their product,
    the product with v, three additions, the mask) and at most K roundings of the chain (the fused product adds none); the bias
    through K.  With u = 2^-24 and gamma_n = n*u / (1 - n*u):  |out - out64| <= gamma_(K+8) * (|bias| + sum_k |weight| * colabs),
    colabs the column formed with |v| and |mask|."""
    kernel = tuple(np.shape(weight)[2:])
    wt = np.asarray(weight, F32).astype(np.float64)
    M = wt.shape[0]
    wt = wt.reshape(M, -1)
    K = wt.shape[1]
    bs = np.zeros(M) if bias is None else np.asarray(bias, F32).astype(np.float64)
    col = columns(input, offset, mask, kernel, stride, padding, dilation, dg, dtype=np.float64)
    mag = columns(input, offset, mask, kernel, stride, padding, dilation, dg, dtype=np.float64, absolute=True)
    out = bs[None, :, None] + np.einsum("mk,bkp->bmp", wt, col)
    bound = (K + 8) * U * (np.abs(bs)[None, :, None] + np.einsum("mk,bkp->bmp", np.abs(wt), mag)) / (1 - (K + 8) * U)
    Ho, Wo = out_size(np.shape(input)[2], np.shape(input)[3], kernel, stride, padding, dilation)
    return out.reshape(-1, M, Ho, Wo), bound.reshape(-1, M, Ho, Wo)


def gemm_bound(weight, bias, colabs):
    """gamma_(K+8) * (|bias| + |weight| @ colabs) for columns given directly, [B, M, P]."""
    wt = np.abs(np.asarray(weight, np.float64).reshape(np.shape(weight)[0], -1))
    K = wt.shape[1]
    bs = np.zeros(wt.shape[0]) if bias is None else np.abs(np.asarray(bias, np.float64))
    return (K + 8) * U * (bs[None, :, None] + np.einsum("mk,bkp->bmp", wt, np.asarray(colabs, np.float64))) / (1 - (K + 8) * U)


# ------------------------------------------------------------------------------------------------------------- comparison
def canon(a):
    """float32 bit patterns with -0 as +0 and every NaN as one pattern."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    bits = a.view(np.uint32).copy()
    bits[bits == np.uint32(0x80000000)] = 0
    bits[np.isnan(a)] = np.uint32(0x7FC00000)
    return bits


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(canon(a), canon(b))


# ------------------------------------------------------------------------------------------------------------------ cases
# name -> B, C, M, H, W, kernel, stride, padding, dilation, dg
CASES = {
    "odd_k_small_m": dict(B=2, C=3, M=5, H=7, W=9, kernel=(3, 3), stride=1, padding=1, dilation=1, dg=1),        # K = 27, pixel tail
    "two_groups_m33": dict(B=1, C=4, M=33, H=13, W=11, kernel=(3, 3), stride=2, padding=2, dilation=2, dg=2),    # M just over a tile
    "m_several_tiles": dict(B=1, C=16, M=256, H=9, W=9, kernel=(3, 3), stride=1, padding=1, dilation=1, dg=1),
    "k_chunks_pixel_tiles": dict(B=1, C=64, M=64, H=34, W=45, kernel=(3, 3), stride=1, padding=1, dilation=1, dg=1),
    "one_by_one": dict(B=2, C=8, M=8, H=6, W=5, kernel=(1, 1), stride=1, padding=0, dilation=1, dg=1),
    # beyond the issue's five: kh*kw = 15 > 9 taps (the sampling state is not kept in LDS), a group of an odd number of k
    # values (15: a zero row in the middle of the chain), every geometry parameter different in the two directions
    "uncached_odd_group": dict(B=2, C=2, M=3, H=9, W=8, kernel=(5, 3), stride=(1, 2), padding=(2, 1), dilation=(1, 2), dg=2),
}
ISSUE_CASES = ("odd_k_small_m", "two_groups_m33", "m_several_tiles", "k_chunks_pixel_tiles", "one_by_one")
COLUMN_CASES = ("odd_k_small_m", "two_groups_m33", "one_by_one", "uncached_odd_group")


def make_inputs(name):
    """The case's tensors, deterministic: offsets N(0, 2^2) with a tenth of them rounded to integers, and planted per case:
    samples exactly on -1, on H-1 / W-1 and on H / W, an exact interior integer, +-1e9 and one NaN."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20260)
    B, C, M, H, W, dg = c["B"], c["C"], c["M"], c["H"], c["W"], c["dg"]
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(c["kernel"]), pair(c["stride"]), pair(c["padding"]), pair(c["dilation"])
    Ho, Wo = out_size(H, W, c["kernel"], c["stride"], c["padding"], c["dilation"])
    KK = kh * kw
    x = rng.standard_normal((B, C, H, W)).astype(F32)
    weight = (rng.standard_normal((M, C, kh, kw)) / np.sqrt(C * KK)).astype(F32)
    bias = rng.standard_normal(M).astype(F32)
    off = (2 * rng.standard_normal((B, dg, KK, 2, Ho, Wo))).astype(F32)
    off = np.where(rng.random(off.shape) < 0.1, np.rint(off), off).astype(F32)
    mask = rng.random((B, dg * KK, Ho, Wo)).astype(F32)
    mask[rng.random(mask.shape) < 0.02] = 0
    plants = [("h", -1.0), ("h", H - 1.0), ("h", float(H)), ("h", float(H // 2)), ("w", -1.0), ("w", W - 1.0), ("w", float(W)),
              ("w", float(W // 2)), ("h", 1e9), ("w", -1e9), ("h", np.nan)]
    sites = rng.choice(B * dg * KK * Ho * Wo, size=len(plants), replace=False)
    planted = []
    for site, (axis, target) in zip(sites, plants):
        b, g, t, y, xx = np.unravel_index(site, (B, dg, KK, Ho, Wo))
        base = y * sh - ph + (t // kw) * dh if axis == "h" else xx * sw - pw + (t % kw) * dw
        value = F32(target) - F32(base) if np.isfinite(target) and abs(target) < 1e6 else F32(target)
        off[b, g, t, 0 if axis == "h" else 1, y, xx] = value
        if np.isfinite(target) and abs(target) < 1e6:
            off[b, g, t, 1 if axis == "h" else 0, y, xx] = F32(0.25)      # the other coordinate stays near the tap: the sample counts
        planted.append((int(b), int(g), int(t), int(y), int(xx), axis, float(target)))
    return dict(c, input=x, weight=weight, bias=bias, offset=off.reshape(B, 2 * dg * KK, Ho, Wo), mask=mask, Ho=Ho, Wo=Wo,
                planted=planted)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs with the twin's ``col`` [B, K, P] and ``out`` [B, M, Ho, Wo]: computed once, shared, not to be written to."""
    d = make_inputs(name)
    d["col"] = columns(d["input"], d["offset"], d["mask"], d["kernel"], d["stride"], d["padding"], d["dilation"], d["dg"])
    d["out"] = chain(d["col"], d["weight"], d["bias"]).reshape(d["B"], d["M"], d["Ho"], d["Wo"])
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d
