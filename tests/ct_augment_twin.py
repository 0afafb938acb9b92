"""The numpy twin of clean_pvnet_amd.ct_augment: the contract of DESIGN.md section 19, stage by stage, that the device is held to
byte for byte (tests/test_gpu_ct_augment.py) and that tests/test_ct_augment.py pins to the reference's own code
(tests/golden/ct_augment_*.npz) and to plain binary64 samplers.

numpy evaluates each binary64 / float32 operation below once, in the order written, as the kernels do under
``-ffp-contract=off``.  The two fixed-point samplers and ``invert_affine`` are those of tests/crop_twin.py;
``randint`` is that of tests/augment_twin.py.  ``warpAffine``, ``getAffineTransform``, ``cvtColor`` and ``boundingRect`` below are
also what tests/golden/make_ct_augment_golden.py gives the reference's own code in place of OpenCV, which is not installed where
this is built.
"""
import itertools
import math

import numpy as np

from tests import augment_twin, crop_twin

F32, F64 = np.float32, np.float64
INTER_NEAREST, INTER_LINEAR, COLOR_BGR2GRAY = 0, 1, 6
N_SAMPLE, NORMAL_COLUMNS = 11, (7, 8, 9)
ORDERS = tuple(itertools.permutations(range(3)))
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
MEAN, STD = (0.40789654, 0.44719302, 0.47026115), (0.28863828, 0.27408164, 0.27809835)
EIG_VAL = (0.2141788, 0.01817699, 0.00341571)
EIG_VEC = ((-0.58752847, -0.69563484, 0.41340352), (-0.5832747, 0.00994535, -0.81221408), (-0.56089297, 0.71832671, 0.41158938))
SCALE_RANGE = (0.6, 1.4)
randint = augment_twin.randint


# ------------------------------------------------------------------------------------------------------------ the draws
def draws_for(B, N, seed):
    """A seeded table [B, 11 + 2 N]: uniforms in [0, 1), standard normals in columns 7-9."""
    rng = np.random.default_rng(seed)
    d = np.minimum(rng.random((B, N_SAMPLE + 2 * N)), 1 - 2.0 ** -53)
    d[:, list(NORMAL_COLUMNS)] = rng.standard_normal((B, 3))
    return d


# ------------------------------------------------------------------------------------------------------------ OpenCV's part
def warp_f32(src, M, dsize):
    """[H,W] float32 -> [oh,ow] float32 under the coordinates and weights of the 8-bit bilinear rule, zero border: the sum of
    tap * weight / 1024.  The weights are non-negative, so the result is non-zero iff a tap of non-zero weight is."""
    ow, oh = dsize
    I = crop_twin.invert_affine(M)
    sx, sy, a, b = linear_coords(I, oh, ow)
    t = lambda yy, xx: _tap2(src, yy, xx)          # noqa: E731
    acc = t(sy, sx) * ((32 - a) * (32 - b)) + t(sy, sx + 1) * (a * (32 - b)) + t(sy + 1, sx) * ((32 - a) * b) + t(sy + 1, sx + 1) * (a * b)
    return (acc / 1024.).astype(F32)


def _tap2(img, sy, sx):
    H, W = img.shape[:2]
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return np.where(ok, img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(F64), 0.)


def warpAffine(src, M, dsize, flags=INTER_LINEAR):
    M = np.asarray(M, F64)
    if flags == INTER_NEAREST:
        return nearest_labels(src, crop_twin.invert_affine(M), dsize[1], dsize[0]).astype(src.dtype)
    assert flags == INTER_LINEAR
    if src.dtype == np.uint8 and src.ndim == 3:
        return crop_twin.warp_u8(src, M, dsize)
    assert src.dtype == F32 and src.ndim == 2
    return warp_f32(src, M, dsize)


def getAffineTransform(src, dst):
    """cv2.getAffineTransform of three float32 point pairs: the binary64 solve of the 6 x 6 system."""
    src, dst = np.asarray(src, F64), np.asarray(dst, F64)
    A = np.hstack([src, np.ones((3, 1))])
    return np.stack([np.linalg.solve(A, dst[:, 0]), np.linalg.solve(A, dst[:, 1])])


def cvtColor(image, code):
    """COLOR_BGR2GRAY on a float32 image: (b * 0.114f + g * 0.587f) + r * 0.299f, each operation rounding once."""
    assert code == COLOR_BGR2GRAY and image.dtype == F32
    return (image[..., 0] * F32(0.114) + image[..., 1] * F32(0.587)) + image[..., 2] * F32(0.299)


def boundingRect(mask):
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


# ------------------------------------------------------------------------------------------------------------ the composition
def place_one(mask, H, W, uy, ux):
    """(y_min, x_min, h, w, dst_y, dst_x) of one instance; (0, 0, -1, -1, 0, 0) for an empty mask."""
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return (0, 0, -1, -1, 0, 0)
    y_min, x_min = int(ys.min()), int(xs.min())
    h, w = int(ys.max()) - y_min, int(xs.max()) - x_min
    return (y_min, x_min, h, w, randint(0, H - h, uy), randint(0, W - w, ux))


def compose(bg, inst_img, inst_mask, num, draws):
    """cut_and_paste in the reference's order, instance after instance; pixels outside the canvas are dropped."""
    B, H, W = bg.shape[:3]
    N = inst_img.shape[1]
    img, label, place = bg.copy(), np.zeros((B, H, W), np.uint8), np.zeros((B, N, 6), np.int32)
    for b in range(B):
        for n in range(N):
            m = np.asarray(inst_mask[b, n]) != 0
            rec = place_one(m if n < int(num[b]) else np.zeros_like(m), H, W, draws[b, N_SAMPLE + 2 * n], draws[b, N_SAMPLE + 2 * n + 1])
            place[b, n] = rec
            if rec[2] < 0:
                continue
            ys, xs = np.nonzero(m)
            dy, dx = ys - rec[0] + rec[4], xs - rec[1] + rec[5]
            ok = (dy >= 0) & (dy < H) & (dx >= 0) & (dx < W)
            img[b, dy[ok], dx[ok]] = inst_img[b, n, ys[ok], xs[ok]]
            label[b, dy[ok], dx[ok]] = n + 1
    return {"img": img, "label": label, "place": place}


# ------------------------------------------------------------------------------------------------------------ the host's part
def center_scale(H, W, u, scale_range=SCALE_RANGE, train=True):
    """tless_utils.augment lines 20-41 with numpy's own types: (center [2], scale [2]) as float32."""
    if not train:
        return np.array([W / 2., H / 2.], F32), np.array([max(W, H) * 1.0] * 2, F32)
    scale = np.array([max(H, W) * 1.0] * 2, F32) * (scale_range[0] + (scale_range[1] - scale_range[0]) * float(u[0]))
    assert scale.dtype == F32
    center = np.array([0, 0])
    for i, (size, v) in enumerate(((W, u[1]), (H, u[2]))):
        border = scale[i] // 2 if scale[i] < size else size - scale[i] // 2
        border_r = max(size - border, border + 1)
        center[i] = randint(border, border_r, v)
    return center.astype(F32), scale


def affine(center, scale, rot, size):
    """The closed form of get_affine_transform(center, scale, rot, size) in binary64."""
    dw, dh = size
    cx, cy = F64(center[0]), F64(center[1])
    k = F64(dw) / F64(scale[0])
    cs, sn = (1.0, 0.0) if rot == 0 else (math.cos(math.pi * float(rot) / 180), math.sin(math.pi * float(rot) / 180))
    a, b = k * F64(cs), k * F64(sn)
    return np.array([[a, b, dw * 0.5 - (a * cx + b * cy)], [-b, a, dh * 0.5 - (a * cy - b * cx)]], F64)


def trans_bound(center, scale, size):
    """(linear, translation): how far the closed form may lie from the three-point solve.  The solve's source points are float32:
    src[0] is exact, src[1] is rounded once, src[2] inherits that and rounds twice more, so every coordinate is off by at most
    e = 1.5 ulp32(M), M = |c|_max + scale / 2 their largest magnitude (ulp32(M) <= 2^-23 M).  With S = L Q + E the matrix of the
    two difference vectors (L = scale / 2, Q orthogonal, |E|_2 <= |E|_F <= 2 e) the linear part A = D S^-1 moves by at most
    k (2 e / L) / (1 - 2 e / L), k = dw / scale; the translation dst[0] - A src[0] by that times |cx| + |cy|.  The binary64
    roundings of both routes (a 3 x 3 solve of condition ~ M / L, a dozen operations) add 2^-40 (k M + dw) at the most."""
    c = np.abs(np.asarray(center, F64))
    L = F64(scale[0]) / 2
    M = c.max() + L
    e = 1.5 * 2.0 ** -23 * M
    k = size[0] / F64(scale[0])
    r = 2 * e / L
    noise = 2.0 ** -40 * (k * M + size[0])
    lin = k * r / (1 - r) + noise
    return lin, lin * (c[0] + c[1]) + noise


def colour_params(u):
    """(order, alpha [3] binary64, light [3] binary64) of one sample."""
    order = ORDERS[min(int(math.floor(6 * float(u[3]))), 5)]
    alpha = [1. + (-0.4 + (0.4 - -0.4) * float(u[4 + i])) for i in range(3)]
    ev = np.array(EIG_VAL, F32) * (0.0 + 0.1 * np.asarray(u[7:10], F64))
    vec = np.array(EIG_VEC, F32).astype(F64)
    light = (vec[:, 0] * ev[0] + vec[:, 1] * ev[1]) + vec[:, 2] * ev[2]
    return order, alpha, light


# ------------------------------------------------------------------------------------------------------------ the device's part
def linear_coords(I, oh, ow):
    """(sx, sy, a, b) [oh,ow] of the 8-bit bilinear rule through the inverse map I."""
    y, x = np.arange(oh, dtype=F64)[:, None], np.arange(ow, dtype=F64)[None, :]
    X0, Y0 = crop_twin.sat_rint((I[0, 1] * y + I[0, 2]) * 1024.) + 16, crop_twin.sat_rint((I[1, 1] * y + I[1, 2]) * 1024.) + 16
    X, Y = (X0 + crop_twin.sat_rint(I[0, 0] * x * 1024.)) >> 5, (Y0 + crop_twin.sat_rint(I[1, 0] * x * 1024.)) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def nearest_labels(label, I, oh, ow):
    """[oh,ow]: the label under the nearest rule of uncrop_mask through the inverse map I, 0 outside."""
    I = np.asarray(I, F64)
    y, x = np.arange(oh, dtype=F64)[:, None], np.arange(ow, dtype=F64)[None, :]
    X = (crop_twin.sat_rint((I[0, 1] * y + I[0, 2]) * 1024.) + 512 + crop_twin.sat_rint(I[0, 0] * x * 1024.)) >> 10
    Y = (crop_twin.sat_rint((I[1, 1] * y + I[1, 2]) * 1024.) + 512 + crop_twin.sat_rint(I[1, 0] * x * 1024.)) >> 10
    H, W = label.shape
    ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    return np.where(ok, label[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)], 0)


def _label_tap(label, sy, sx):
    H, W = label.shape
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return np.where(ok, label[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64), 0)


def owners(label, trans_output, oh, ow, N, mode):
    """[N,oh,ow] bool: which output pixels belong to instance i."""
    I = crop_twin.invert_affine(trans_output)
    if mode == "nearest":
        lab = nearest_labels(label, I, oh, ow)
        return np.stack([lab == i + 1 for i in range(N)])
    sx, sy, a, b = linear_coords(I, oh, ow)
    taps = [(_label_tap(label, sy, sx), np.ones_like(a, bool)), (_label_tap(label, sy, sx + 1), a > 0),
            (_label_tap(label, sy + 1, sx), b > 0), (_label_tap(label, sy + 1, sx + 1), (a > 0) & (b > 0))]
    return np.stack([np.any([(t == i + 1) & w for t, w in taps], axis=0) for i in range(N)])


def boxes_of(own, oh, ow):
    out = np.zeros((len(own), 4), np.int32)
    for i, m in enumerate(own):
        x, y, w, h = boundingRect(m)
        if w:
            out[i] = (x, y, min(x + w, ow - 1), min(y + h, oh - 1))
    return out


def tree_sum(v):
    """The tree of train.hpp on 256 binary64 slots: slot j += slot j + s for s = 128, 64, ..., 1."""
    v = np.array(v, F64)
    s = 128
    while s:
        v[:s] = v[:s] + v[s:2 * s]
        s >>= 1
    return v[0]


def grey_mean(orig):
    """float32: the grey level of [ih,iw,3] uint8 summed in binary64 per 64 x 4 tile (lane = row * 64 + column), the tiles per
    slot (tile j, j + 256, ...) and the slots, each in the tree; divided by the count and rounded once."""
    ih, iw = orig.shape[:2]
    gs = cvtColor(orig.astype(F32) / F32(255), COLOR_BGR2GRAY).astype(F64)
    ty, tx = (ih + 3) // 4, (iw + 63) // 64
    pad = np.zeros((ty * 4, tx * 64))
    pad[:ih, :iw] = gs
    parts = [tree_sum(pad[4 * j:4 * j + 4, 64 * i:64 * i + 64].ravel()) for j in range(ty) for i in range(tx)]
    slots = np.zeros(256)
    for i, p in enumerate(parts):
        slots[i % 256] = slots[i % 256] + p
    return F32(tree_sum(slots) / F64(ih * iw))


def colour(orig, u, mean=MEAN, std=STD, train=True, gs_mean=None):
    """[ih,iw,3] uint8 -> [3,ih,iw] float32: color_aug in the drawn order, the lighting vector, the normalisation."""
    x = orig.astype(F32) / F32(255)
    if train:
        order, alpha, light = colour_params(u)
        gs = cvtColor(x, COLOR_BGR2GRAY)
        gm = grey_mean(orig) if gs_mean is None else F32(gs_mean)
        for s, op in enumerate(order):
            a, oma = F32(alpha[s]), F32(1 - alpha[s])
            x = x * a
            if op == CONTRAST:
                x = x + gm * oma
            elif op == SATURATION:
                x = x + (gs * oma)[..., None]
            assert x.dtype == F32
        x = (x.astype(F64) + light).astype(F32)
    x = (x - np.asarray(mean, F32)) / np.asarray(std, F32)
    assert x.dtype == F32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def augment(img, label, draws, *, train=True, input_size=(44, 72), down_ratio=4, scale_range=SCALE_RANGE, rot=0.0, boxes="linear",
            mean=MEAN, std=STD, n_instances=None):
    B, H, W = img.shape[:3]
    ih, iw = (int(input_size[0]), int(input_size[1])) if train else ((H + 31) // 32 * 32, (W + 31) // 32 * 32)
    rot = rot if train else 0.0
    oh, ow = ih // down_ratio, iw // down_ratio
    N = 0 if label is None else n_instances if n_instances is not None else (draws.shape[1] - N_SAMPLE) // 2
    out = {"inp": np.zeros((B, 3, ih, iw), F32), "orig_img": np.zeros((B, ih, iw, 3), np.uint8), "center": np.zeros((B, 2), F32),
           "scale": np.zeros((B, 2), F32), "trans_input": np.zeros((B, 2, 3)), "trans_output": np.zeros((B, 2, 3))}
    if label is not None:
        out["boxes"] = np.zeros((B, N, 4), np.int32)
    for b in range(B):
        u = draws[b] if draws is not None else np.zeros(N_SAMPLE)
        c, s = center_scale(H, W, u, scale_range, train)
        t_in, t_out = affine(c, s, rot, (iw, ih)), affine(c, s, rot, (ow, oh))
        out["center"][b], out["scale"][b], out["trans_input"][b], out["trans_output"][b] = c, s, t_in, t_out
        out["orig_img"][b] = crop_twin.warp_u8(img[b], t_in, (iw, ih))
        out["inp"][b] = colour(out["orig_img"][b], u, mean, std, train)
        if label is not None:
            out["boxes"][b] = boxes_of(owners(label[b], t_out, oh, ow, N, boxes), oh, ow)
    return out


# ------------------------------------------------------------------------------------------------------------ shared inputs
H0, W0, CH, CW, N0 = 30, 50, 12, 14, 3          # the canvas, the cut-outs, the instances of the small cases


def image(seed, H=H0, W=W0):
    return crop_twin.image(seed, H, W)


def cutouts(B, N=N0, h=CH, w=CW, seed=0):
    """(inst_img [B,N,h,w,3] uint8, inst_mask [B,N,h,w] uint8): seeded rectangles with a hole, values 1 or 255."""
    rng = np.random.default_rng(1000 + seed)
    img = rng.integers(0, 256, (B, N, h, w, 3), dtype=np.uint8)
    mask = np.zeros((B, N, h, w), np.uint8)
    for b in range(B):
        for n in range(N):
            y0, x0 = rng.integers(0, h // 2), rng.integers(0, w // 2)
            y1, x1 = rng.integers(y0 + 2, h + 1), rng.integers(x0 + 2, w + 1)
            mask[b, n, y0:y1, x0:x1] = 255 if (b + n) % 2 else 1
            mask[b, n, (y0 + y1) // 2, (x0 + x1) // 2] = 0
            mask[b, n, y0, x0] = 1                                              # (the hole of a 2 x 2 rectangle may be its corner)
    return img, mask


def batch(B, seed, N=N0):
    """(bg, inst_img, inst_mask, cls, num, draws) of a seeded batch on the small shapes."""
    bg = np.stack([image(seed + b) for b in range(B)])
    inst_img, inst_mask = cutouts(B, N, seed=seed)
    rng = np.random.default_rng(2000 + seed)
    cls, num = rng.integers(0, 5, (B, N)), np.full(B, N, np.int64)
    return bg, inst_img, inst_mask, cls, num, draws_for(B, N, 3000 + seed)


def mixed_batch():
    """B = 8 on the small shapes, one required case per sample (tests/test_ct_augment.py names them):
    0 a scale draw with scale < width, colour order 0;  1 a scale draw with scale >= width, order 1;  2 three instances that
    overlap in one pixel, order 2;  3 a single-pixel mask (h = w = 0), an empty mask, order 3;  4 num[b] = 1 < N, order 4;
    5 an alpha of exactly 1 in all steps and a zero lighting vector, order 5;  6 objects in a corner that the warp leaves outside
    the window;  7 a wide object at the right edge whose box ow - 1 clamps, a thin one
    whose box collapses to x2 == x0."""
    B, N = 8, N0
    bg, inst_img, inst_mask, cls, num, d = batch(B, 7)
    d[:, 3] = [(k + 0.5) / 6 for k in range(6)] + [0.1, 0.9]
    d[0, 1] = 0.5
    d[0, 0], d[1, 0] = 0.05, 0.95                                    # scale 50 * 0.64 = 32 < 50 > 30;  50 * 1.36 = 68 >= 50
    full = np.zeros((CH, CW), np.uint8)
    full[2:9, 3:10] = 1
    inst_mask[2, :] = full                                           # three equal masks ...
    d[2, N_SAMPLE:] = np.tile([10.5 / (H0 - 6), 20.5 / (W0 - 6)], N)     # ... at one place: dst = (10, 20)
    inst_mask[3, 0] = 0
    inst_mask[3, 0, 5, 6] = 7                                        # one pixel
    inst_mask[3, 1] = 0                                              # empty
    num[4] = 1
    d[5, 4:7] = 0.5
    d[5, 7:10] = 0.0
    # 6: a small scale centred far from the objects in the top-left corner
    small = np.zeros((CH, CW), np.uint8)
    small[0:3, 0:3] = 1
    inst_mask[6, :] = small
    d[6, N_SAMPLE:] = 0.0                                            # dst = (0, 0)
    d[6, 0], d[6, 1], d[6, 2] = 0.0, 0.999, 0.999                    # scale 30, centre at the far end of its range
    # 7: the identity scale (50: centre x fixed at 25), centre y 15: output x = 0.36 (x - 25) + 9.  Instance 0 spans the cut-out's
    # width and ends at the canvas' last column: x_max + 1 = ow is clamped to ow - 1.  Instance 1 is two columns wide in the last
    # two columns: it owns output column ow - 1 alone and its box collapses to x2 == x0.
    wide, thin = np.zeros((CH, CW), np.uint8), np.zeros((CH, CW), np.uint8)
    wide[4:8, 0:CW] = 1
    thin[4:8, 5:7] = 1
    inst_mask[7, 0], inst_mask[7, 1] = wide, thin
    d[7, N_SAMPLE:N_SAMPLE + 4] = [0.1, 0.999, 0.6, 0.99]          # dst = (2, 36) and (16, 48)
    d[7, 0], d[7, 1], d[7, 2] = 0.5, 0.5, 0.5
    return bg, inst_img, inst_mask, cls, num, d
