"""The numpy twin of a PVNet decoder stage (include/pvnet_vote.h, "PVNet decoder stage": ``PVV_HEAD_STAGE`` of
``pvv_head_forward``) and of the whole decoder, built from the head's twin (tests/head_twin.py): the same ``upsample``,
``im2col``, ``chain`` and ``fmaf``, stopped after the activation.

    u = upsample(a) (the head's float32 align_corners=True blend), or u = a under ``PVV_HEAD_SAME_RES``
    z = cat([u, skip]) inside a ring of zeros;  acc = +0;  for k = c*9 + dy*3 + dx ascending: acc = fmaf(weight[o,k], z.., acc)
    t = fmaf(acc, scale, shift);  a = t if t > 0 else t * float32(slope)

``stage64`` is the same function in binary64 with the float32 contract's distance from it: ``head_twin.forward64``'s terms up to
``e_a``.  ``decoder`` composes three stages and ``head_twin.forward`` as lib/networks/pvnet/resnet18.py:81-92 of the reference does.

``split_rows`` is beyond the issue's cases: an upsampling stage with more than 64 output channels, which the kernel splits over
two workgroups of two row blocks (four row blocks with the upsample's state spill).  So are ``same_res_one_block`` and
``same_res_two_blocks``: the kernel without the upsample at one and two row blocks, which no other case reaches.
"""
import functools

import numpy as np

from tests import head_twin as ht
from tests.head_twin import EPS, F32, U, same_bits, to_bf16, to_f16  # noqa: F401  (re-exported for the tests)

KEYS = ("a", "skip", "weight", "scale", "shift")


# ------------------------------------------------------------------------------------------------------------ the function
def stage(a, skip, weight, scale, shift, slope=0.1, *, up=True, coords="align", ring="zero", order="a_skip", crop=False):
    """out [B, M, H, W] float32.  ``coords``, ``ring``, ``order`` and ``crop`` state a rule wrongly for the mutation tests:
    ``crop`` upsamples where the same resolution was meant, and keeps the top-left h x w of the result."""
    a, skip = np.asarray(a, F32), np.asarray(skip, F32)
    u = ht.upsample(a, coords=coords) if up or crop else a
    if crop:
        u = u[:, :, :a.shape[2], :a.shape[3]]
    B, _, H, W = u.shape
    z = np.concatenate([u, skip] if order == "a_skip" else [skip, u], axis=1)
    w1 = np.asarray(weight, F32)
    M = w1.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = ht.chain(ht.im2col(z, ring), w1.reshape(M, -1), None)
        t = ht.fmaf(acc, np.asarray(scale, F32)[None, :, None], np.asarray(shift, F32)[None, :, None]).reshape(acc.shape)
        out = np.where(t > 0, t, t * F32(slope)).astype(F32)
    return out.reshape(B, M, H, W)


def stage64(a, skip, weight, bn, slope=0.1, *, up=True):
    """(a64, bound) [B, M, H, W]: the stage in binary64 -- exact source index, the BatchNorm from its own parameters ``bn`` =
    (gamma, beta, mean, var, eps) -- and the float32 contract's distance from it: ``head_twin.forward64``'s e_u (0 without the
    upsample and for the skip tensor's channels), e_acc, e_t and e_a, term by term as stated there."""
    a, skip = np.asarray(a, F32), np.asarray(skip, F32)
    gamma, beta, mean, var, eps = bn
    w1 = np.asarray(weight, F32).astype(np.float64)
    M = w1.shape[0]
    w1 = w1.reshape(M, -1)
    g, b, m, v = (np.asarray(p, F32).astype(np.float64) for p in (gamma, beta, mean, var))
    with np.errstate(invalid="ignore", over="ignore"):
        u64, e_u = ht.upsample64(a) if up else (a.astype(np.float64), np.zeros(a.shape))
        B, _, H, W = u64.shape
        z = np.concatenate([u64, skip.astype(np.float64)], axis=1)
        e_z = np.concatenate([e_u, np.zeros(skip.shape)], axis=1)
        col, ecol = ht.im2col(z), ht.im2col(e_z)
        acc = np.einsum("mk,bkp->bmp", w1, col)
        e_acc = ht.gemm_bound(w1, None, np.abs(col) + ecol) + np.einsum("mk,bkp->bmp", np.abs(w1), ecol)
        scale = (g / np.sqrt(v + eps))[None, :, None]
        shift = (b - m * g / np.sqrt(v + eps))[None, :, None]
        t = acc * scale + shift
        d = (np.abs(scale) * (1 + U) * e_acc + U * np.abs(scale) * np.abs(acc) + U * np.abs(shift)
             + 2.0 ** -48 * ((np.abs(acc) + np.abs(m)[None, :, None]) * np.abs(scale) + np.abs(b)[None, :, None]))
        e_t = d + U * (np.abs(t) + d)
        out = np.where(t > 0, t, t * slope)
        e_a = e_t + 2 * U * abs(slope) * (np.abs(t) + e_t)
        e_a = e_a * (1 + 2.0 ** -20)                                                     # the binary64 evaluation's own roundings
    return out.reshape(B, M, H, W), e_a.reshape(B, M, H, W)


def decoder(x, x2s, x4s, x8s, xfc, p, slope=0.1):
    """out [B, seg_dim + ver_dim, H, W]: resnet18.py:81-92 from the backbone's outputs.  ``p``: name -> tensors, the folded
    ``scale`` / ``shift`` of every BatchNorm included."""
    fm = stage(xfc, x8s, p["conv8s.weight"], p["conv8s.scale"], p["conv8s.shift"], slope, up=False)
    fm = stage(fm, x4s, p["conv4s.weight"], p["conv4s.scale"], p["conv4s.shift"], slope)
    fm = stage(fm, x2s, p["conv2s.weight"], p["conv2s.scale"], p["conv2s.shift"], slope)
    return ht.forward(fm, x, p["convraw.weight1"], p["convraw.scale"], p["convraw.shift"], p["convraw.weight2"], p["convraw.bias2"], slope)


# ------------------------------------------------------------------------------------------------------------------ cases
CASES = {
    "one_by_one": dict(B=2, C2=3, C0=1, h=1, w=1, M=2, up=True),                 # r = 0; every pixel is border
    "odd_chunks": dict(B=1, C2=70, C0=59, h=5, w=9, M=5, up=True),               # C = 129: several chunks, odd, partial last chunk and tile
    "no_skip_same_res": dict(B=2, C2=5, C0=0, h=9, w=35, M=97, up=False),        # four row blocks, the last partial; two tiles along W
    "stage_4s": dict(B=1, C2=128, C0=64, h=5, w=17, M=64, up=True),              # conv4s's channels
    "stage_8s": dict(B=1, C2=256, C0=128, h=9, w=33, M=128, up=False),           # conv8s's channels, the largest M
    "stage_2s": dict(B=1, C2=64, C0=64, h=4, w=16, M=32, up=True),               # conv2s's channels, exactly one full tile
    "split_rows": dict(B=1, C2=5, C0=2, h=5, w=5, M=70, up=True),                # M > 64 with the upsample: two workgroups per tile
    "same_res_one_block": dict(B=1, C2=3, C0=2, h=5, w=6, M=5, up=False),        # no upsample with one row block
    "same_res_two_blocks": dict(B=1, C2=2, C0=3, h=5, w=6, M=40, up=False),      # no upsample with two row blocks
}
BEYOND_ISSUE = ("split_rows", "same_res_one_block", "same_res_two_blocks")
ISSUE_CASES = tuple(n for n in CASES if n not in BEYOND_ISSUE)
DECODER = dict(B=1, H=16, W=24, ver_dim=18, seg_dim=2, fcdim=256, s8dim=128, s4dim=64, s2dim=32, raw_dim=32)


def _plant_bn(gamma, beta, mean, var):
    """head_twin.make_inputs' BatchNorm channels: 0 -- gamma = 0, beta = -0; 1 -- running_var = 0; 2 -- the large-mean shift;
    3, 4 -- gamma = 0, beta = 1."""
    M = len(gamma)
    gamma[0], beta[0], mean[0] = 0, -0.0, 0.5
    var[1] = 0
    if M >= 3:
        mean[2] = 1e6
        beta[2] = F32(float(mean[2]) * float(gamma[2]) / np.sqrt(float(var[2]) + EPS) + 0.37)
    if M >= 5:
        gamma[3:5], beta[3:5] = 0, 1


def _bn(rng, M):
    gamma, beta = rng.uniform(0.5, 1.5, M).astype(F32), rng.standard_normal(M).astype(F32)
    mean, var = (0.1 * rng.standard_normal(M)).astype(F32), rng.uniform(0.5, 1.5, M).astype(F32)
    _plant_bn(gamma, beta, mean, var)
    return gamma, beta, mean, var


def make_inputs(name):
    """The case's tensors, deterministic, with ``head_twin.make_inputs``' plants where the sizes allow: in image 0 of ``a`` one
    NaN at [0, 0, 1, 1] and one +Inf at [0, C2-1, 2, 2] ([0, C2-1, 1, 1] in a map of fewer than five rows: two rows off the far
    edge, where the float32 and the exact source index pick the same cells; [0, 0, 0, 0] and [0, 1, 0, 0] at 1 x 1), and the
    BatchNorm channels of ``_plant_bn``."""
    c = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20270)
    B, C2, C0, h, w, M, up = (c[k] for k in ("B", "C2", "C0", "h", "w", "M", "up"))
    H, W = (2 * h, 2 * w) if up else (h, w)
    a = rng.standard_normal((B, C2, h, w)).astype(F32)
    skip = rng.standard_normal((B, C0, H, W)).astype(F32)
    weight = (rng.standard_normal((M, C2 + C0, 3, 3)) / np.sqrt(9 * (C2 + C0))).astype(F32)
    gamma, beta, mean, var = _bn(rng, M)
    if h == 1:
        a[0, 0, 0, 0], a[0, 1, 0, 0] = np.nan, np.inf
        a[1], skip[1], weight[0] = np.abs(a[1]), np.abs(skip[1]), -np.abs(weight[0])    # acc < 0 in channel 0 of the finite image
    else:
        assert h >= 4 and w >= 5
        a[0, 0, 1, 1] = np.nan
        a[(0, C2 - 1, 2, 2) if h >= 5 else (0, C2 - 1, 1, 1)] = np.inf
    return dict(c, H=H, W=W, a=a, skip=skip, weight=weight, gamma=gamma, beta=beta, mean=mean, var=var, eps=EPS, slope=0.1)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's inputs with the folded ``scale`` / ``shift`` and the twin's ``out`` [B,M,H,W]: computed once, shared, not to be
    written to."""
    d = make_inputs(name)
    d["scale"], d["shift"] = ht.fold_bn(d["gamma"], d["beta"], d["mean"], d["var"], d["eps"])
    d["out"] = stage(d["a"], d["skip"], d["weight"], d["scale"], d["shift"], d["slope"], up=d["up"])
    return _frozen(d)


@functools.lru_cache(maxsize=None)
def decoder_reference():
    """``decoder_16x24``: the reference's channels throughout on a 16 x 24 image; ``x``, ``x2s``, ``x4s``, ``x8s``, ``xfc``, the
    parameters under the reference's state-dict names (``state``), the folded ones (``params``) and the twin's ``out``.  The
    maps at 1/8 are 2 x 3, so a NaN there would reach every output: the NaN and the +Inf are planted in the image, two pixels
    of image 0; every BatchNorm has ``_plant_bn``'s channels."""
    c = DECODER
    rng = np.random.default_rng(20269)
    B, H, W = c["B"], c["H"], c["W"]
    t = lambda *s: rng.standard_normal(s).astype(F32)                                  # noqa: E731
    d = dict(c, x=t(B, 3, H, W), x2s=t(B, 64, H // 2, W // 2), x4s=t(B, 64, H // 4, W // 4), x8s=t(B, 128, H // 8, W // 8),
             xfc=np.abs(t(B, c["fcdim"], H // 8, W // 8)))
    d["x"][0, 0, 3, 4], d["x"][0, 2, 11, 17] = np.nan, np.inf
    state, params = {}, {}
    sizes = {"conv8s": (128 + c["fcdim"], c["s8dim"]), "conv4s": (64 + c["s8dim"], c["s4dim"]), "conv2s": (64 + c["s4dim"], c["s2dim"]),
             "convraw": (3 + c["s2dim"], c["raw_dim"])}
    for name, (cin, cout) in sizes.items():
        w = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(F32)
        gamma, beta, mean, var = _bn(rng, cout)
        state.update({name + ".0.weight": w, name + ".1.weight": gamma, name + ".1.bias": beta, name + ".1.running_mean": mean,
                      name + ".1.running_var": var, name + ".1.num_batches_tracked": np.zeros((), np.int64)})
        scale, shift = ht.fold_bn(gamma, beta, mean, var, EPS)
        params.update({name + (".weight1" if name == "convraw" else ".weight"): w, name + ".scale": scale, name + ".shift": shift})
    M2 = c["seg_dim"] + c["ver_dim"]
    state["convraw.3.weight"] = (rng.standard_normal((M2, c["raw_dim"], 1, 1)) / np.sqrt(c["raw_dim"])).astype(F32)
    state["convraw.3.bias"] = rng.standard_normal(M2).astype(F32)
    params["convraw.weight2"], params["convraw.bias2"] = state["convraw.3.weight"], state["convraw.3.bias"]
    d["state"], d["params"] = _frozen(state), _frozen(params)
    d["out"] = decoder(d["x"], d["x2s"], d["x4s"], d["x8s"], d["xfc"], params)
    return _frozen(d)
