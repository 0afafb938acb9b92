"""The numpy twin of the PVNet output head's contract (include/pvnet_vote.h, "PVNet output head"): float32, operation by operation,
no fused multiply-add in the upsample and exactly one -- emulated, ``dcn_twin.fmaf`` -- per step of the two chains and in the
BatchNorm.

Upsample, per axis (torch's align_corners=True source index in float32):
    r = float32(n_in-1) / float32(n_out-1) if n_in > 1 and n_out > 1 else 0;  src = r * float32(dst);  i0 = int(src);
    i1 = i0 + (i0 < n_in-1);  l1 = src - float32(i0);  l0 = 1 - l1
    u = hl0*(wl0*v00 + wl1*v01) + hl1*(wl0*v10 + wl1*v11)           a zero weight still multiplies its sample
z = cat([u, x]) inside a ring of zeros.  Conv1: acc = +0; for k = c*9 + dy*3 + dx ascending: acc = fmaf(weight1[o,k], z.., acc).
t = fmaf(acc, scale, shift);  a = t if t > 0 else t * float32(slope).  Conv2: acc = bias2[o]; for m ascending: acc = fmaf(weight2[o,m],
a[m], acc).  Store: float32, ``astype(float16)``, or bfloat16 by integer round-to-nearest-even.

The device may add 0 * 0 terms to fill an instruction, which changes at most the sign of a zero: ``same_bits`` (of dcn_twin)
compares bit patterns after mapping -0 to +0, NaNs by position.

The kernel's tile is 8 x 32 output pixels, not 8 x 16: ``reference_channels`` (18 x 34) still spans 3 x 2 tiles with a partial
last tile in both axes, so it stands as the issue states it.  ``max_rows`` is beyond the issue's five: M1 = M2 = 64, the largest,
where the activations need more than 64 KiB of LDS.
"""
import functools

import numpy as np

from tests.dcn_twin import F32, U, canon, chain, fmaf, gemm_bound, same_bits  # noqa: F401  (re-exported for the tests)

EPS = 1e-5                          # nn.BatchNorm2d's default
U64 = 2.0 ** -53


# --------------------------------------------------------------------------------------------------------------- upsample
def axis(n_in, n_out, coords="align"):
    """(i0, i1, l0, l1, src) of one axis, float32 as the contract states it.  ``coords="half_pixel"`` is the mutation:
    align_corners=False."""
    dst = np.arange(n_out).astype(F32)
    if coords == "align":
        r = F32(n_in - 1) / F32(n_out - 1) if n_in > 1 and n_out > 1 else F32(0)
        src = (r * dst).astype(F32)
    else:
        src = np.maximum((F32(n_in) / F32(n_out)) * (dst + F32(0.5)) - F32(0.5), F32(0)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1, src


def exact_axis(n_in, n_out):
    """(i0, i1, l1, src) in binary64 at the exact source index dst * (n_in-1) / (n_out-1)."""
    dst = np.arange(n_out, dtype=np.float64)
    src = dst * (n_in - 1) / (n_out - 1) if n_in > 1 and n_out > 1 else np.zeros(n_out)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), src - i0, src


def _blend(v, ay, ax, dtype):
    (y0, y1, hl0, hl1), (x0, x1, wl0, wl1) = ay, ax
    hl0, hl1 = hl0.astype(dtype)[:, None], hl1.astype(dtype)[:, None]
    wl0, wl1 = wl0.astype(dtype)[None, :], wl1.astype(dtype)[None, :]
    v = v.astype(dtype)
    v00, v01, v10, v11 = v[:, :, y0][:, :, :, x0], v[:, :, y0][:, :, :, x1], v[:, :, y1][:, :, :, x0], v[:, :, y1][:, :, :, x1]
    with np.errstate(invalid="ignore", over="ignore"):
        u = hl0 * (wl0 * v00 + wl1 * v01) + hl1 * (wl0 * v10 + wl1 * v11)
    assert u.dtype == dtype
    return u


def upsample(fm, dtype=F32, absolute=False, coords="align"):
    """u [B, C2, 2h, 2w].  ``dtype=np.float64`` evaluates the same blend in binary64 at the float32 src (l0 = 1 - l1 exact);
    ``absolute`` forms it with |fm| (the magnitude the blend's roundings are relative to)."""
    fm = np.asarray(fm, F32)
    h, w = fm.shape[2:]
    y0, y1, hl0, hl1, _ = axis(h, 2 * h, coords)
    x0, x1, wl0, wl1, _ = axis(w, 2 * w, coords)
    if dtype is not F32:
        hl0, wl0 = 1.0 - hl1.astype(np.float64), 1.0 - wl1.astype(np.float64)
    return _blend(np.abs(fm) if absolute else fm, (y0, y1, hl0, hl1), (x0, x1, wl0, wl1), dtype)


def upsample64(fm):
    """(u64, bound) [B, C2, 2h, 2w]: the blend in binary64 at the exact source index, and the float32 ``upsample``'s distance from
    it.  A bilinear blend is piecewise linear in each coordinate, so moving one coordinate by d changes it by at most d times the
    largest difference of two neighbours along that axis in the cells touched: the coordinate term, per axis
    |src_f32 - src_exact| * max |v[i+1][j] - v[i][j]| over the rows i0 of both evaluations and the columns of both.  It dominates.
    The blend's own roundings: every product wl*v passes through at most 6 (l0 twice, two products, two sums; l1 = src - i0 is
    exact), counted as gamma_8 * the blend of |v|."""
    fm = np.asarray(fm, F32)
    h, w = fm.shape[2:]
    f64 = fm.astype(np.float64)
    ey0, ey1, el1y, esy = exact_axis(h, 2 * h)
    ex0, ex1, el1x, esx = exact_axis(w, 2 * w)
    u64 = _blend(f64, (ey0, ey1, 1 - el1y, el1y), (ex0, ex1, 1 - el1x, el1x), np.float64)
    y0, y1, _, _, sy = axis(h, 2 * h)
    x0, x1, _, _, sx = axis(w, 2 * w)
    with np.errstate(invalid="ignore"):
        dv = np.abs(np.diff(f64, axis=2, append=f64[:, :, -1:]))                  # [.., i, j] = |v[i+1][j] - v[i][j]|, 0 past the end
        dw = np.abs(np.diff(f64, axis=3, append=f64[:, :, :, -1:]))
        slope_h = functools.reduce(np.fmax, [dv[:, :, i][:, :, :, j] for i in (y0, ey0) for j in (x0, x1, ex0, ex1)])
        slope_w = functools.reduce(np.fmax, [dw[:, :, i][:, :, :, j] for i in (y0, y1, ey0, ey1) for j in (x0, ex0)])
        coord = np.abs(sy.astype(np.float64) - esy)[:, None] * slope_h + np.abs(sx.astype(np.float64) - esx)[None, :] * slope_w
        nan = np.isnan(u64)
        coord = np.where(nan, np.nan, coord)
        bound = coord + 8 * U * upsample(fm, np.float64, absolute=True) / (1 - 8 * U)
    return u64, bound


# ------------------------------------------------------------------------------------------------------------ the function
def im2col(z, ring="zero"):
    """[B, C*9, H*W] of z [B, C, H, W] for a 3 x 3 window with a ring of one: k = c*9 + dy*3 + dx."""
    B, C, H, W = z.shape
    p = np.pad(z, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="constant" if ring == "zero" else "edge")
    col = np.stack([p[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=2)    # [B, C, 9, H, W]
    return col.reshape(B, C * 9, H * W)


def fold_bn(gamma, beta, mean, var, eps=EPS, use_eps=True, from_rounded_scale=False):
    """(scale, shift) float32: binary64 scale = gamma / sqrt(var + eps), shift = beta - mean * scale from the unrounded scale, each
    rounded once.  The two flags are the mutations."""
    g, b, m, v = (np.asarray(a, F32).astype(np.float64) for a in (gamma, beta, mean, var))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = g / np.sqrt(v + (eps if use_eps else 0.0))
        shift = b - m * (scale.astype(F32).astype(np.float64) if from_rounded_scale else scale)
    return scale.astype(F32), shift.astype(F32)


def to_f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, F32).astype(np.float16)


def to_bf16(a):
    """The bfloat16 bit patterns (uint16) of float32 ``a``, rounded to nearest even by integer arithmetic; a NaN keeps its upper
    bits and gets the quiet bit."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    bits = a.view(np.uint32).astype(np.uint64)
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    return np.where(np.isnan(a), (bits >> 16) | 0x40, rounded).astype(np.uint16)


def forward(fm, x, weight1, scale, shift, weight2, bias2, slope=0.1, *, coords="align", ring="zero", order="fm_x",
            bias_first=True, parts=False):
    """out [B, M2, 2h, 2w] float32.  ``coords``, ``ring``, ``order`` and ``bias_first`` state a rule wrongly for the mutation tests;
    ``parts`` also returns the pre-activation t [B, M1, 2h, 2w]."""
    fm, x = np.asarray(fm, F32), np.asarray(x, F32)
    u = upsample(fm, coords=coords)
    B, _, H, W = u.shape
    z = np.concatenate([u, x] if order == "fm_x" else [x, u], axis=1)
    w1, w2 = np.asarray(weight1, F32), np.asarray(weight2, F32)
    M1, M2 = w1.shape[0], w2.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = chain(im2col(z, ring), w1.reshape(M1, -1), None)                                       # [B, M1, P]
        t = fmaf(acc, np.asarray(scale, F32)[None, :, None], np.asarray(shift, F32)[None, :, None]).reshape(acc.shape)
        a = np.where(t > 0, t, t * F32(slope)).astype(F32)
        if bias_first:
            out = chain(a, w2.reshape(M2, M1), bias2)
        else:
            out = (chain(a, w2.reshape(M2, M1), None) + np.asarray(bias2, F32)[None, :, None]).astype(F32)
    out = out.reshape(B, M2, H, W)
    return (out, t.reshape(B, M1, H, W)) if parts else out


def half_ulp(v, out_dtype):
    """Half an ulp of the target type at |v| (an upper bound: relative to |v|, and half the smallest subnormal below that)."""
    rel, tiny = {"float16": (2.0 ** -11, 2.0 ** -25), "bfloat16": (2.0 ** -8, 2.0 ** -134)}[out_dtype]
    return np.maximum(rel * np.abs(v), tiny)


def forward64(fm, x, weight1, bn, weight2, bias2, slope=0.1, out_dtype=None):
    """(out64, bound) [B, M2, 2h, 2w]: the function in binary64 -- exact source index, the BatchNorm from its own parameters
    ``bn`` = (gamma, beta, mean, var, eps) -- and the float32 contract's distance from it, term by term (u = 2^-24):
      e_u    ``upsample64``: the coordinate term and the blend's roundings; 0 for the image's channels
      e_acc  gemm_bound(weight1, |z| + e_z) -- gamma_(K+8) * |weight1| . |z| for the chain's roundings -- + |weight1| . e_z
      e_t    d + u * (|t| + d),  d = |scale| * e_acc + u * |scale| * |acc| + u * |shift| (scale and shift rounded to float32) + the
             reference's own cancellation in binary64, 2^-48 * ((|acc| + |mean|) * |scale| + |beta|): one fmaf
      e_a    e_t (LeakyReLU is 1-Lipschitz) + 2u * slope * (|t| + e_t) for the float32 slope and its product
      e_out  gemm_bound(weight2, bias2, |a| + e_a) + |weight2| . e_a
      and half an ulp of the target type at |out| + e_out for a half-precision output."""
    fm, x = np.asarray(fm, F32), np.asarray(x, F32)
    gamma, beta, mean, var, eps = bn
    w1 = np.asarray(weight1, F32).astype(np.float64)
    M1 = w1.shape[0]
    w1 = w1.reshape(M1, -1)
    w2 = np.asarray(weight2, F32).astype(np.float64).reshape(-1, M1)
    b2 = np.asarray(bias2, F32).astype(np.float64)
    g, b, m, v = (np.asarray(a, F32).astype(np.float64) for a in (gamma, beta, mean, var))
    with np.errstate(invalid="ignore", over="ignore"):
        u64, e_u = upsample64(fm)
        B, _, H, W = u64.shape
        z = np.concatenate([u64, x.astype(np.float64)], axis=1)
        e_z = np.concatenate([e_u, np.zeros(x.shape)], axis=1)
        col, ecol = im2col(z), im2col(e_z)
        acc = np.einsum("mk,bkp->bmp", w1, col)
        e_acc = gemm_bound(w1, None, np.abs(col) + ecol) + np.einsum("mk,bkp->bmp", np.abs(w1), ecol)
        scale = (g / np.sqrt(v + eps))[None, :, None]
        shift = (b - m * g / np.sqrt(v + eps))[None, :, None]
        t = acc * scale + shift
        d = (np.abs(scale) * (1 + U) * e_acc + U * np.abs(scale) * np.abs(acc) + U * np.abs(shift)
             + 2.0 ** -48 * ((np.abs(acc) + np.abs(m)[None, :, None]) * np.abs(scale) + np.abs(b)[None, :, None]))
        e_t = d + U * (np.abs(t) + d)
        a = np.where(t > 0, t, t * slope)
        e_a = e_t + 2 * U * abs(slope) * (np.abs(t) + e_t)
        out = b2[None, :, None] + np.einsum("om,bmp->bop", w2, a)
        bound = gemm_bound(w2, b2, np.abs(a) + e_a) + np.einsum("om,bmp->bop", np.abs(w2), e_a)
        bound = bound * (1 + 2.0 ** -20)                                                 # the binary64 evaluation's own roundings
        if out_dtype is not None:
            bound = bound + half_ulp(np.abs(out) + bound, out_dtype)
    return out.reshape(B, -1, H, W), bound.reshape(B, -1, H, W)


# ------------------------------------------------------------------------------------------------------------------ cases
CASES = {
    "one_by_one": dict(B=2, C2=3, C0=1, h=1, w=1, M1=2, M2=1),                # r = 0; every pixel is border
    "odd_k": dict(B=1, C2=2, C0=3, h=5, w=7, M1=5, M2=3),                     # K = 45; smaller than one tile
    "reference_channels": dict(B=1, C2=32, C0=3, h=9, w=17, M1=32, M2=20),    # PVNet's channels; 3 x 2 tiles, the last ones partial
    "two_blocks": dict(B=1, C2=4, C0=3, h=6, w=6, M1=33, M2=38),              # two 32-row blocks for M1 and M2; M1 odd
    "no_image": dict(B=2, C2=3, C0=0, h=6, w=7, M1=4, M2=2),                  # no image channels; K = 27
    "max_rows": dict(B=1, C2=2, C0=1, h=5, w=5, M1=64, M2=64),                # the largest M1 and M2: the kernel's LDS limit is raised
    "rows_2_1": dict(B=1, C2=2, C0=1, h=5, w=5, M1=34, M2=3),                 # two row blocks for M1, one for M2
    "rows_1_2": dict(B=1, C2=3, C0=2, h=5, w=5, M1=5, M2=33),                 # one row block for M1, two for M2
}


def make_inputs(name):
    """The case's tensors, deterministic, with planted in every case (where its sizes allow):
      fm         one NaN at [0, 0, 1, 1] and one +Inf at [0, C2-1, 2, 2] ([0, 0, 0, 0] and [0, 1, 0, 0] at 1 x 1): image 0 only, and
                 two rows and columns off the far edges, where the float32 and the exact source index pick the same cells
      channel 0  gamma = 0, beta = -0, mean = 0.5: shift = -0, the pre-activation is exactly -0 wherever acc < 0
      channel 1  running_var = 0: the scale is gamma / sqrt(eps)
      channel 2  mean = 1e6 and beta = mean * scale + 0.37 (M1 >= 3): the shift is the small difference of two large numbers, so
                 folding it from the rounded scale shows
      channels 3, 4 (M1 >= 5)  gamma = 0, beta = 1: a = 1 exactly; the last output takes them with weight 2e38 each from a bias
                 of -3e38 and nothing else: finite only when the chain starts at the bias
      bias2[0] = 70000: the first output overflows float16."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20261)
    B, C2, C0, h, w, M1, M2 = (c[k] for k in ("B", "C2", "C0", "h", "w", "M1", "M2"))
    C = C2 + C0
    fm = rng.standard_normal((B, C2, h, w)).astype(F32)
    x = rng.standard_normal((B, C0, 2 * h, 2 * w)).astype(F32)
    weight1 = (rng.standard_normal((M1, C, 3, 3)) / np.sqrt(9 * C)).astype(F32)
    gamma = rng.uniform(0.5, 1.5, M1).astype(F32)
    beta = rng.standard_normal(M1).astype(F32)
    mean = (0.1 * rng.standard_normal(M1)).astype(F32)
    var = rng.uniform(0.5, 1.5, M1).astype(F32)
    weight2 = (rng.standard_normal((M2, M1, 1, 1)) / np.sqrt(M1)).astype(F32)
    bias2 = rng.standard_normal(M2).astype(F32)
    if h == 1:
        fm[0, 0, 0, 0], fm[0, 1, 0, 0] = np.nan, np.inf
        fm[1], x[1], weight1[0] = np.abs(fm[1]), np.abs(x[1]), -np.abs(weight1[0])      # acc < 0 in channel 0 of the finite image
    else:
        assert h >= 5 and w >= 5
        fm[0, 0, 1, 1], fm[0, C2 - 1, 2, 2] = np.nan, np.inf
    gamma[0], beta[0], mean[0] = 0, -0.0, 0.5
    var[1] = 0
    if M1 >= 3:
        mean[2] = 1e6
        beta[2] = F32(float(mean[2]) * float(gamma[2]) / np.sqrt(float(var[2]) + EPS) + 0.37)
    if M1 >= 5:
        gamma[3:5], beta[3:5] = 0, 1
        weight2[M2 - 1] = 0
        weight2[M2 - 1, 3:5] = 2e38
        bias2[M2 - 1] = -3e38
    bias2[0] = 70000
    return dict(c, fm=fm, x=x, weight1=weight1, gamma=gamma, beta=beta, mean=mean, var=var, eps=EPS, weight2=weight2, bias2=bias2)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs with the folded ``scale`` / ``shift`` and the twin's ``u`` [B,C2,H,W], pre-activation ``t`` and ``out``
    [B,M2,H,W]: computed once, shared, not to be written to."""
    d = make_inputs(name)
    d["scale"], d["shift"] = fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    d["u"] = upsample(d["fm"])
    d["out"], d["t"] = forward(d["fm"], d["x"], d["weight1"], d["scale"], d["shift"], d["weight2"], d["bias2"], parts=True)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d
