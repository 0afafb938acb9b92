"""The numpy twin of the DCNv2 backward contract (include/pvnet_vote.h, "Modulated deformable convolution, backward"): float32
operation by operation, ``dcn_twin.fmaf`` for the two chains, integers for the scatter, binary64 where the contract says so.
h, w, the window test, the neighbours v1..v4 and the blend weights w1..w4 are the forward's (tests/dcn_twin.py).

  1. gcol[b,k,p]   acc = +0; for o ascending: acc = fmaf(weight[o,k], grad_out[b,o,p], acc)
  2. per (b,g,t,p), over the group's channels ascending, from +0, inside the window only, gc = gcol[b, c*KK + t, p], m the mask:
       grad_mask  += gc * (((w1*v1 + w2*v2) + w3*v3) + w4*v4)
       grad_off_h += (ch * gc) * m,   ch = (((0 + (-wl)*v1) + (-wh)*v2) + wl*v3) + wh*v4,   wl = float(w0+1) - w,  wh = w - float(w0)
       grad_off_w += (cw * gc) * m,   cw = (((0 + (-hl)*v1) + hl*v2) + (-hh)*v3) + hh*v4,    hl = float(h0+1) - h,  hh = h - float(h0)
     max_b = the largest |gc * m| of the image, window or not (bit patterns: a NaN is "not finite")
  3. grad_input    n = rint(binary64(w_i * (gc * m)) * 2^(40 - e_b)) summed as int64 per element; float32(binary64(sum) * 2^(e_b - 40));
                   2^e_b the smallest power of two >= max_b; all NaN when max_b is not finite, all +0 when it is 0
  4. grad_weight   per (b, slab of SLAB pixels): acc = +0; for p ascending: acc = fmaf(grad_out[b,o,p], col[b,k,p], acc);
                   float32 of the binary64 sum over (b, slab) ascending
  5. grad_bias     per image 256 binary64 lane sums (p = l, l+256, ..), folded s[i] += s[i+w] for w = 128..1; images ascending; float32

``backward64`` is the anchor: the same function in torch ops on the CPU in binary64 -- gather the four neighbours, blend, ``floor``
taken as a constant, the forward's window test -- differentiated by autograd, evaluated at the float32 h and w.  ``bounds`` is
the float32 contract's distance from it, counted from the operations above.
"""
import functools

import numpy as np

from tests import dcn_twin
from tests.dcn_twin import F32, U, fmaf, out_size, pair

SLAB = 512                          # PVV_DCN_SLAB
FIX = 40                            # contributions are multiples of 2^(e_b - FIX)
LANES = 256


def gamma(n):
    return n * U / (1 - n * U)


# ------------------------------------------------------------------------------------------------------------- the sampling
def taps(shape, offset, kernel, stride=1, padding=0, dilation=1, dg=1):
    """The forward's sampling state per (b, g, t, y, x), all [B, dg, KK, P]: float32 h, w; ``inside``; int64 h0, w0 (0
    outside); float32 w1..w4; ``ok`` [4] the neighbours inside the plane (and the window); ``flat`` [4] their clipped indices."""
    B, C, H, W = shape
    off = np.asarray(offset, F32)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(kernel), pair(stride), pair(padding), pair(dilation)
    Ho, Wo = out_size(H, W, kernel, stride, padding, dilation)
    KK, P = kh * kw, Ho * Wo
    off = off.reshape(B, dg, KK, 2, Ho, Wo)
    t = np.arange(KK)
    base_h = (np.arange(Ho) * sh - ph)[None, :] + ((t // kw) * dh)[:, None]
    base_w = (np.arange(Wo) * sw - pw)[None, :] + ((t % kw) * dw)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        h = (base_h.astype(F32)[None, None, :, :, None] + off[:, :, :, 0]).reshape(B, dg, KK, P)
        w = (base_w.astype(F32)[None, None, :, None, :] + off[:, :, :, 1]).reshape(B, dg, KK, P)
        inside = (h > F32(-1)) & (w > F32(-1)) & (h < F32(H)) & (w < F32(W))
    hz, wz = np.where(inside, h, F32(0)), np.where(inside, w, F32(0))
    hf, wf = np.floor(hz), np.floor(wz)
    lh, lw = hz - hf, wz - wf
    hh, hw = F32(1) - lh, F32(1) - lw
    h0, w0 = hf.astype(np.int64), wf.astype(np.int64)
    top, left, bottom, right = h0 >= 0, w0 >= 0, h0 + 1 <= H - 1, w0 + 1 <= W - 1
    ok = [top & left & inside, top & right & inside, bottom & left & inside, bottom & right & inside]
    flat = [np.clip(h0 + dy, 0, H - 1) * W + np.clip(w0 + dx, 0, W - 1) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
    z = F32(0)
    wts = [np.where(inside, a, z) for a in (hh * hw, hh * lw, lh * hw, lh * lw)]
    assert all(a.dtype == F32 for a in wts)
    return dict(h=hz, w=wz, inside=inside, h0=h0, w0=w0, wts=wts, ok=ok, flat=flat, Ho=Ho, Wo=Wo, KK=KK, P=P)


def neighbours(input, tp, dg, dtype=F32):
    """v1..v4 [B, dg, Cg, KK, P], 0 where the neighbour is outside."""
    x = np.asarray(input, F32)
    B, C, H, W = x.shape
    Cg, KK, P = C // dg, tp["KK"], tp["P"]
    planes = x.reshape(B, dg, Cg, H * W)
    out = []
    for flat, ok in zip(tp["flat"], tp["ok"]):
        idx = np.broadcast_to(flat.reshape(B, dg, 1, KK * P), (B, dg, Cg, KK * P))
        v = np.take_along_axis(planes, idx, axis=3).reshape(B, dg, Cg, KK, P)
        out.append(np.where(ok[:, :, None], v, F32(0)).astype(dtype))
    return out


# ------------------------------------------------------------------------------------------------------------ 1. gcol
def gcol(weight, gout):
    """[B, K, P] float32: the chain over o from +0."""
    wt = np.asarray(weight, F32)
    M = wt.shape[0]
    wt = wt.reshape(M, -1)
    go = np.asarray(gout, F32).reshape(np.shape(gout)[0], M, -1)
    acc = np.zeros((go.shape[0], wt.shape[1], go.shape[2]), F32)
    for o in range(M):
        acc = fmaf(wt[o][None, :, None], go[:, o][:, None, :], acc).reshape(acc.shape)
    return acc


# ---------------------------------------------------------------------------------------- 2. grad_offset, grad_mask, the maximum
def abs_bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32) & np.uint32(0x7FFFFFFF)


def coord(input, mask, gc5, tp, dg):
    """(grad_offset [B, dg, KK, 2, P], grad_mask [B, dg, KK, P], maxbits [B] uint32) from gcol as [B, dg, Cg, KK, P]."""
    B, _, Cg, KK, P = gc5.shape
    m = np.asarray(mask, F32).reshape(B, dg, KK, P)
    v = neighbours(input, tp, dg)
    w1, w2, w3, w4 = tp["wts"]
    inside, h, w = tp["inside"], tp["h"], tp["w"]
    hl, hh = (tp["h0"] + 1).astype(F32) - h, h - tp["h0"].astype(F32)
    wl, wh = (tp["w0"] + 1).astype(F32) - w, w - tp["w0"].astype(F32)
    gh, gw, gm = (np.zeros((B, dg, KK, P), F32) for _ in range(3))
    mx = np.zeros(B, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(Cg):
            gc = gc5[:, :, c]
            v1, v2, v3, v4 = (a[:, :, c] for a in v)
            mx = np.maximum(mx, abs_bits(gc * m).reshape(B, -1).max(axis=1))
            val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
            ch = (((F32(0) + (-wl) * v1) + (-wh) * v2) + wl * v3) + wh * v4
            cw = (((F32(0) + (-hl) * v1) + hl * v2) + (-hh) * v3) + hh * v4
            gm = np.where(inside, gm + gc * val, gm)
            gh = np.where(inside, gh + (ch * gc) * m, gh)
            gw = np.where(inside, gw + (cw * gc) * m, gw)
    assert gm.dtype == F32 and gh.dtype == F32
    return np.stack([gh, gw], axis=3), gm, mx


# ------------------------------------------------------------------------------------------------------- 3. grad_input
def pow2_exp(bits):
    """e with 2^e the smallest power of two >= the finite float32 > 0 of these bits."""
    mant, ex = np.frexp(np.float64(np.uint32(bits).view(F32)))
    return int(ex) - 1 if mant == 0.5 else int(ex)


def contributions(mask, gc5, tp, dg, shape):
    """Every (image, flat element of [C, H, W], float32 value w_i * (gc * m)) of the scatter, as three flat arrays."""
    B, C, H, W = shape
    _, _, Cg, KK, P = gc5.shape
    m = np.asarray(mask, F32).reshape(B, dg, 1, KK, P)
    with np.errstate(invalid="ignore", over="ignore"):
        top = gc5 * m
        chan = (np.arange(dg)[:, None] * Cg + np.arange(Cg)[None, :]).reshape(1, dg, Cg, 1, 1)
        img = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), top.shape)
        bs, es, vs = [], [], []
        for wt, ok, flat in zip(tp["wts"], tp["ok"], tp["flat"]):
            sel = np.broadcast_to(ok[:, :, None], top.shape)
            val = wt[:, :, None] * top
            elem = chan * (H * W) + flat[:, :, None]
            bs.append(img[sel]), es.append(np.broadcast_to(elem, top.shape)[sel]), vs.append(val[sel])
    vals = np.concatenate(vs)
    assert vals.dtype == F32
    return np.concatenate(bs), np.concatenate(es), vals


def fixed_point_scatter(img, elem, vals, maxbits, shape, order=None):
    """grad_input [B, C, H, W] float32 from the contributions, added in ``order`` (any permutation gives the same bytes)."""
    B, C, H, W = shape
    if order is not None:
        img, elem, vals = img[order], elem[order], vals[order]
    out = np.zeros((B, C * H * W), F32)
    for b in range(B):
        mb = int(maxbits[b])
        if mb >= 0x7F800000:
            out[b] = np.nan
        elif mb:
            e = pow2_exp(mb)
            sel = img == b
            n = np.rint(vals[sel].astype(np.float64) * 2.0 ** (FIX - e)).astype(np.int64)
            total = np.zeros(C * H * W, np.int64)
            np.add.at(total, elem[sel], n)
            out[b] = (total.astype(np.float64) * 2.0 ** (e - FIX)).astype(F32)
    return out.reshape(B, C, H, W)


def float64_scatter(img, elem, vals, shape):
    """The same contributions added in binary64, with how many reached each element."""
    B, C, H, W = shape
    total, count = np.zeros((B, C * H * W)), np.zeros((B, C * H * W), np.int64)
    np.add.at(total, (img, elem), vals.astype(np.float64))
    np.add.at(count, (img, elem), 1)
    return total.reshape(shape), count.reshape(shape)


# ------------------------------------------------------------------------------------------------------ 4. grad_weight
def grad_weight(col, gout, weight_shape):
    col = np.asarray(col, F32)
    B, K, P = col.shape
    M = weight_shape[0]
    go = np.asarray(gout, F32).reshape(B, M, P)
    total = np.zeros((M, K))
    for b in range(B):
        for p0 in range(0, P, SLAB):
            acc = np.zeros((M, K), F32)
            for p in range(p0, min(P, p0 + SLAB)):
                acc = fmaf(go[b, :, p][:, None], col[b, :, p][None, :], acc).reshape(M, K)
            total = total + acc.astype(np.float64)
    return total.astype(F32).reshape(weight_shape)


# -------------------------------------------------------------------------------------------------------- 5. grad_bias
def grad_bias(gout):
    go = np.asarray(gout, F32)
    B, M = go.shape[:2]
    go = go.reshape(B, M, -1).astype(np.float64)
    P = go.shape[2]
    steps = -(-P // LANES)
    padded = np.zeros((B, M, steps * LANES))
    padded[:, :, :P] = go
    padded = padded.reshape(B, M, steps, LANES)
    total = np.zeros(M)
    for b in range(B):
        s = np.zeros((M, LANES))
        for j in range(steps):
            s = s + padded[b, :, j]
        w = LANES // 2
        while w:
            s[:, :w] = s[:, :w] + s[:, w:2 * w]
            w //= 2
        total = total + s[:, 0]
    return total.astype(F32)


# ------------------------------------------------------------------------------------------------------------ the whole
def backward(input, offset, mask, weight, gout, stride=1, padding=0, dilation=1, dg=1, need=(True,) * 5):
    """(grad_input, grad_offset, grad_mask, grad_weight, grad_bias) float32, None where not needed."""
    x, wt = np.asarray(input, F32), np.asarray(weight, F32)
    B, C, H, W = x.shape
    kernel = tuple(wt.shape[2:])
    tp = taps(x.shape, offset, kernel, stride, padding, dilation, dg)
    KK, P, Ho, Wo, Cg = tp["KK"], tp["P"], tp["Ho"], tp["Wo"], C // dg
    out = [None] * 5
    if need[0] or need[1] or need[2]:
        gc5 = gcol(wt, gout).reshape(B, dg, Cg, KK, P)
        goff, gm, mx = coord(x, mask, gc5, tp, dg)
        if need[1]:
            out[1] = goff.reshape(B, 2 * dg * KK, Ho, Wo)
        if need[2]:
            out[2] = gm.reshape(B, dg * KK, Ho, Wo)
        if need[0]:
            out[0] = fixed_point_scatter(*contributions(mask, gc5, tp, dg, x.shape), mx, x.shape)
    if need[3]:
        out[3] = grad_weight(dcn_twin.columns(x, offset, mask, kernel, stride, padding, dilation, dg), gout, wt.shape)
    if need[4]:
        out[4] = grad_bias(gout)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------- the anchor
def dcn64(x, off, msk, wt, bs, stride=1, padding=0, dilation=1, dg=1):
    """The modulated deformable convolution in torch ops, binary64, differentiable: [B, M, Ho, Wo].  The sampling positions are
    the float32 ones of ``off``'s values (a constant is added to each offset, so that d position / d offset stays 1)."""
    import torch
    B, C, H, W = x.shape
    M, kernel = wt.shape[0], tuple(wt.shape[2:])
    tp = taps(tuple(x.shape), off.detach().numpy().astype(F32), kernel, stride, padding, dilation, dg)
    KK, P, Cg = tp["KK"], tp["P"], C // dg
    inside = torch.from_numpy(tp["inside"])
    o = off.reshape(B, dg, KK, 2, P)
    zero = torch.zeros((), dtype=torch.float64)

    def position(o1, at32):
        o1s = torch.where(inside, o1, zero)                                         # (a NaN or huge offset stays out of the graph)
        return o1s + (torch.from_numpy(at32.astype(np.float64)) - o1s).detach()

    h, w = position(o[:, :, :, 0], tp["h"]), position(o[:, :, :, 1], tp["w"])
    lh, lw = h - torch.from_numpy(tp["h0"]).double(), w - torch.from_numpy(tp["w0"]).double()      # floor: a constant
    hh, hw = 1 - lh, 1 - lw
    planes = x.reshape(B, dg, Cg, H * W)
    val = 0
    for wgt, ok, flat in zip((hh * hw, hh * lw, lh * hw, lh * lw), tp["ok"], tp["flat"]):
        idx = torch.from_numpy(flat).reshape(B, dg, 1, KK * P).expand(B, dg, Cg, KK * P)
        v = torch.gather(planes, 3, idx).reshape(B, dg, Cg, KK, P)
        v = torch.where(torch.from_numpy(ok)[:, :, None], v, zero)
        val = val + torch.where(inside, wgt, zero)[:, :, None] * v
    col = (val * msk.reshape(B, dg, 1, KK, P)).reshape(B, C * KK, P)
    out = torch.einsum("mk,bkp->bmp", wt.reshape(M, -1), col)
    if bs is not None:
        out = out + bs[None, :, None]
    return out.reshape(B, M, tp["Ho"], tp["Wo"])


def backward64(input, offset, mask, weight, bias, gout, stride=1, padding=0, dilation=1, dg=1):
    """The five gradients in binary64 by autograd through ``dcn64``, as numpy arrays."""
    import torch
    leaves = [torch.from_numpy(np.asarray(a, F32).astype(np.float64)).requires_grad_(True) for a in (input, offset, mask, weight, bias)]
    out = dcn64(*leaves, stride, padding, dilation, dg)
    out.backward(torch.from_numpy(np.asarray(gout, F32).astype(np.float64)).reshape(out.shape))
    return tuple(a.grad.numpy() for a in leaves)


def bounds(input, offset, mask, weight, gout, stride=1, padding=0, dilation=1, dg=1, gout_err=None):
    """|contract - backward64| <= these, per gradient, as gamma_n * sum |terms| with n counted from the contract
    (u = 2^-24, gamma_n = n*u / (1 - n*u); one is added to every n for the binary64 arithmetic on both sides):
      gcol         M roundings (one per fmaf step) on sum_o |weight| |grad_out|  =: G
      grad_bias    n = 2:  the one float32 rounding
      grad_weight  n = SLAB + 10:  8 inside a column element (dcn_twin.forward64), at most SLAB chain steps, the final rounding
      grad_mask    n = M + Cg + 9:  gcol M, the blend without the mask 7, the product 1, Cg additions
      grad_offset  n = M + Cg + 9:  gcol M, ch / cw 6 (a difference 1, a product 1, four additions), two products, Cg additions
      grad_input   n = M + 7:  gcol M, w_i 3 (two differences, a product), gc * m 1, the product 1, the final float32 1; plus
                   half a quantum 2^(e - 41) per contribution, e from the largest G * |m| (* (1 + gamma_(M+1)): never below the
                   contract's own e_b)
    With ``gout_err`` (|grad_out - the exact upstream gradient| elementwise) the terms' sums with it in place of |grad_out| are
    added: every gradient is linear in grad_out."""
    x, wt = np.asarray(input, F32), np.asarray(weight, F32)
    B, C, H, W = x.shape
    M, kernel = wt.shape[0], tuple(wt.shape[2:])
    tp = taps(x.shape, offset, kernel, stride, padding, dilation, dg)
    KK, P, Ho, Wo, Cg = tp["KK"], tp["P"], tp["Ho"], tp["Wo"], C // dg
    awt = np.abs(wt.astype(np.float64)).reshape(M, -1)
    m = np.abs(np.asarray(mask, F32).astype(np.float64)).reshape(B, dg, 1, KK, P)
    v = [np.abs(a) for a in neighbours(x, tp, dg, np.float64)]
    inside = tp["inside"][:, :, None]
    w64 = [np.where(tp["inside"], np.abs(a.astype(np.float64)), 0.0)[:, :, None] for a in tp["wts"]]
    h, w = tp["h"].astype(np.float64), tp["w"].astype(np.float64)
    hl, hh = (tp["h0"] + 1 - h)[:, :, None], (h - tp["h0"])[:, :, None]
    wl, wh = (tp["w0"] + 1 - w)[:, :, None], (w - tp["w0"])[:, :, None]
    valabs = sum(a * b for a, b in zip(w64, v))
    chabs = np.where(inside, wl * v[0] + wh * v[1] + wl * v[2] + wh * v[3], 0.0)
    cwabs = np.where(inside, hl * v[0] + hl * v[1] + hh * v[2] + hh * v[3], 0.0)
    colabs = (valabs * m).reshape(B, C * KK, P)
    chan = (np.arange(dg)[:, None] * Cg + np.arange(Cg)[None, :]).reshape(1, dg, Cg, 1, 1)

    def terms(ago):
        """The sums of |terms| of the five gradients for an upstream magnitude ago [B, M, P], and G * |m|."""
        G = np.einsum("mk,bmp->bkp", awt, ago).reshape(B, dg, Cg, KK, P)
        t_off = np.stack([(chabs * G * m).sum(axis=2), (cwabs * G * m).sum(axis=2)], axis=3).reshape(B, 2 * dg * KK, Ho, Wo)
        t_mask = (valabs * G).sum(axis=2).reshape(B, dg * KK, Ho, Wo)
        t_in = np.zeros((B, C * H * W))
        for wq, ok, flat in zip(w64, tp["ok"], tp["flat"]):
            sel = np.broadcast_to(ok[:, :, None], G.shape)
            img = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), G.shape)
            elem = np.broadcast_to(chan * (H * W) + flat[:, :, None], G.shape)
            np.add.at(t_in, (img[sel], elem[sel]), (wq * G * m)[sel])
        t_w = np.einsum("bmp,bkp->mk", ago, colabs).reshape(wt.shape)
        return t_in.reshape(x.shape), t_off, t_mask, t_w, ago.sum(axis=(0, 2)), G * m

    ago = np.abs(np.asarray(gout, F32).astype(np.float64)).reshape(B, M, P)
    t_in, t_off, t_mask, t_w, t_b, Gm = terms(ago)
    count = np.zeros((B, C * H * W))
    for ok, flat in zip(tp["ok"], tp["flat"]):
        sel = np.broadcast_to(ok[:, :, None], Gm.shape)
        img = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), Gm.shape)
        elem = np.broadcast_to(chan * (H * W) + flat[:, :, None], Gm.shape)
        np.add.at(count, (img[sel], elem[sel]), 1.0)
    top = Gm.reshape(B, -1).max(axis=1) * (1 + gamma(M + 1))
    quantum = np.array([2.0 ** (np.ceil(np.log2(t)) + 1 - FIX - 1) if t > 0 else 0.0 for t in top])       # 2^(e - 41), e rounded up once more for log2's own rounding
    out = [gamma(M + 8) * t_in + count.reshape(x.shape) * quantum[:, None, None, None], gamma(M + Cg + 10) * t_off,
           gamma(M + Cg + 10) * t_mask, gamma(SLAB + 11) * t_w, gamma(3) * t_b]
    if gout_err is not None:
        extra = terms(np.asarray(gout_err, np.float64).reshape(B, M, P))
        out = [a + b for a, b in zip(out, extra[:5])]
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ cases
def upstream(name):
    """The case's upstream gradient, N(0, 1), deterministic."""
    d = dcn_twin.reference(name)
    rng = np.random.default_rng(sorted(dcn_twin.CASES).index(name) + 771)
    return rng.standard_normal((d["B"], d["M"], d["Ho"], d["Wo"])).astype(F32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs (dcn_twin.reference), its upstream gradient ``gout`` and the twin's five gradients ``grads``: computed
    once, shared, not to be written to."""
    d = dict(dcn_twin.reference(name))
    d["gout"] = upstream(name)
    d["grads"] = backward(d["input"], d["offset"], d["mask"], d["weight"], d["gout"], d["stride"], d["padding"], d["dilation"], d["dg"])
    d["gout"].setflags(write=False)
    for g in d["grads"]:
        g.setflags(write=False)
    return d
