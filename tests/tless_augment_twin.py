"""The numpy twin of clean_pvnet_amd.tless_augment: the contract of DESIGN.md section 22, stage by stage, that the device is held
to byte for byte (tests/test_gpu_tless_augment.py) and that tests/test_tless_augment.py pins to the reference's own code
(tests/golden/tless_augment_*.npz).

numpy evaluates each binary64 / float32 operation below once, in the order written, as the kernels do under
``-ffp-contract=off``.  The two fixed-point samplers and ``invert_affine`` are those of tests/crop_twin.py,
``getRotationMatrix2D`` is that of tests/augment_twin.py, ``place_one``, ``boundingRect`` and the colour step those of
tests/ct_augment_twin.py.  ``warpAffine`` below is also what tests/golden/make_tless_augment_golden.py gives the reference's own
code in place of OpenCV, which is not installed where this is built.
"""
import math

import numpy as np

from tests import augment_twin, crop_twin
from tests import ct_augment_twin as ct

F32, F64 = np.float32, np.float64
INTER_NEAREST, INTER_LINEAR = ct.INTER_NEAREST, ct.INTER_LINEAR
COLUMNS = ("scale", "box", "top", "order", "alpha_0", "alpha_1", "alpha_2", "normal_0", "normal_1", "normal_2", "rot", "dst_y", "dst_x", "black")
N_SAMPLE, PER, NORMAL_COLUMNS = 14, 3, (7, 8, 9)
SCALE, BOX, TOP, ROT, DST_Y, DST_X, BLACK = 0, 1, 2, 10, 11, 12, 13
SCALE_TRAIN_RATIO, BOX_TRAIN_RATIO = (1.8, 2.4), (1.0, 1.2)
MEAN, STD = ct.MEAN, ct.STD
getRotationMatrix2D = augment_twin.getRotationMatrix2D
boundingRect, place_one = ct.boundingRect, ct.place_one


def draws_for(B, N, seed):
    """A seeded table [B, 14 + 3 N]: uniforms in [0, 1), standard normals in columns 7-9."""
    rng = np.random.default_rng(seed)
    d = np.minimum(rng.random((B, N_SAMPLE + PER * N)), 1 - 2.0 ** -53)
    d[:, list(NORMAL_COLUMNS)] = rng.standard_normal((B, 3))
    return d


# ------------------------------------------------------------------------------------------------------------ rotate_image
def rotate_side(h, w):
    return math.isqrt(h * h + w * w)


def warpAffine(src, M, dsize, flags=INTER_LINEAR):
    """uint8 [H,W] or [H,W,3] -> [dsize[1], dsize[0](,3)]: the 8-bit fixed-point bilinear rule or the nearest rule, zero border."""
    M = np.asarray(M, F64)
    assert src.dtype == np.uint8
    planes = src if src.ndim == 3 else src[..., None]
    if flags == INTER_NEAREST:
        I = crop_twin.invert_affine(M)
        out = np.stack([ct.nearest_labels(planes[..., c], I, dsize[1], dsize[0]) for c in range(planes.shape[2])], axis=2).astype(np.uint8)
    else:
        assert flags == INTER_LINEAR
        out = crop_twin.warp_u8(planes, M, dsize)
    return out if src.ndim == 3 else out[..., 0]


def rotation(h, w, deg):
    """tless_train_utils.py:154-165: (M [2,3], bound_h, bound_w)."""
    cx, cy = w / 2, h / 2
    M = getRotationMatrix2D((cx, cy), float(deg), 1.)
    abs_cos, abs_sin = abs(M[0, 0]), abs(M[0, 1])
    bound_w, bound_h = int(h * abs_sin + w * abs_cos), int(h * abs_cos + w * abs_sin)
    M[0, 2] += bound_w / 2 - cx
    M[1, 2] += bound_h / 2 - cy
    return M, bound_h, bound_w


def rotate(mat, deg, interp="linear"):
    """(rotated [bound_h, bound_w(,3)], M)."""
    M, bh, bw = rotation(mat.shape[0], mat.shape[1], deg)
    return warpAffine(mat, M, (bw, bh), INTER_LINEAR if interp == "linear" else INTER_NEAREST), M


def rotate_image(img, deg, interp="linear"):
    """The public form: ``out`` zero padded to D x D, ``size`` and ``rot``, for leading dimensions ``deg.shape``."""
    deg = np.asarray(deg, F64)
    lead = deg.shape
    h, w = img.shape[len(lead):len(lead) + 2]
    D = rotate_side(h, w)
    img = img.astype(np.uint8)
    out = np.zeros(lead + (D, D) + img.shape[len(lead) + 2:], np.uint8)
    size, rot = np.zeros(lead + (2,), np.int32), np.zeros(lead + (2, 3))
    for i in np.ndindex(lead):
        r, M = rotate(img[i], deg[i], interp)
        out[i][:r.shape[0], :r.shape[1]] = r
        size[i], rot[i] = r.shape[:2], M
    return {"out": out, "size": size, "rot": rot}


# ------------------------------------------------------------------------------------------------------------ the composition
def _paste(canvas, canvas_mask, img, mask, rec, mask_id):
    """tless_utils.py:94-97; what leaves the canvas is dropped."""
    H, W = canvas_mask.shape
    ys, xs = np.nonzero(mask)
    dy, dx = ys - rec[0] + rec[4], xs - rec[1] + rec[5]
    ok = (dy >= 0) & (dy < H) & (dx >= 0) & (dx < W)
    canvas[dy[ok], dx[ok]] = img[ys[ok], xs[ok]]
    canvas_mask[dy[ok], dx[ok]] = mask_id


def compose_one(bg, img, mask, kpt_2d, other_img, other_mask, u, fused_bg=None, num=None, rot_max=360., ratio=0.8, interp="linear"):
    H, W = bg.shape[:2]
    N = len(other_img)
    num = N if num is None else max(0, min(int(num), N))
    place = np.zeros((1 + N, 6), np.int32)
    # read_data (pvnet.py:60-66) and the first lines of get_training_img (:74-82)
    deg = float(u[ROT]) * float(rot_max)
    r_img, _ = rotate(img, deg, interp)
    r_mask, M = rotate(mask.astype(np.uint8), deg, interp)
    pixel_num = int(r_mask.astype(np.int64).sum())
    kpt = np.asarray(kpt_2d, F64)
    kpt = np.stack([(M[0, 0] * kpt[:, 0] + M[0, 1] * kpt[:, 1]) + M[0, 2], (M[1, 0] * kpt[:, 0] + M[1, 1] * kpt[:, 1]) + M[1, 2]], axis=1)
    train_img, train_mask = bg.copy(), np.zeros((H, W), np.uint8)
    rec = place_one(r_mask, H, W, u[DST_Y], u[DST_X])
    place[0] = rec
    if rec[2] >= 0:
        _paste(train_img, train_mask, r_img, r_mask, rec, 1)
    kpt = (kpt - np.array([rec[1], rec[0]], F64)) + np.array([rec[5], rec[4]], F64)
    # get_fused_image (tless_train_utils.py:94-136)
    fused_img = np.zeros((H, W, 3), np.uint8) if u[BLACK] >= 0.9 else (bg if fused_bg is None else fused_bg).copy()
    fused_mask = np.zeros((H, W), np.uint8)
    for n in range(N):
        c = N_SAMPLE + PER * n
        o_mask = rotate(other_mask[n].astype(np.uint8), float(u[c]) * 360., interp)[0] if n < num else np.zeros((1, 1), np.uint8)
        rec_n = place_one(o_mask, H, W, u[c + 1], u[c + 2])
        place[1 + n] = rec_n
        if rec_n[2] >= 0:
            _paste(fused_img, fused_mask, rotate(other_img[n], float(u[c]) * 360., interp)[0], o_mask, rec_n, 1)
    fused = fused_mask != 0
    # pvnet.py:86-100
    target = train_mask == 1
    on_top = fused_img.copy()
    on_top[target] = train_img[target]
    occluded, occluded_mask = train_img.copy(), train_mask.copy()
    occluded[fused] = fused_img[fused]
    occluded_mask[fused] = 0
    visible = int(occluded_mask.astype(np.int64).sum())
    if rec[2] < 0:
        path, out_img, out_mask = 3, fused_img, train_mask
    elif u[TOP] < 0.5:
        path, out_img, out_mask = 0, on_top, train_mask
    elif F64(visible) / F64(pixel_num) < ratio:
        path, out_img, out_mask = 2, on_top, train_mask
    else:
        path, out_img, out_mask = 1, occluded, occluded_mask
    x, y, w, h = boundingRect(out_mask)
    bbox = [x, y, x + w - 1, y + h - 1] if w else [0, 0, W - 1, H - 1]
    return {"img": out_img, "mask": out_mask, "kpt_2d": kpt, "bbox": np.array(bbox, np.int32), "path": np.int32(path), "place": place,
            "visible": np.array([visible, pixel_num], np.int64), "train_img": train_img, "train_mask": train_mask, "fused_img": fused_img,
            "fused_mask": fused.astype(np.uint8)}


def compose(bg, img, mask, kpt_2d, other_img, other_mask, draws, fused_bg=None, num=None, rot_max=360., ratio=0.8, interp="linear"):
    B = len(bg)
    rot_max = np.broadcast_to(np.asarray(rot_max, F64), (B,))
    outs = [compose_one(bg[b], img[b], mask[b], kpt_2d[b], other_img[b], other_mask[b], draws[b], None if fused_bg is None else fused_bg[b],
                        None if num is None else num[b], rot_max[b], ratio, interp) for b in range(B)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


COMPOSE_KEYS = ("img", "mask", "kpt_2d", "bbox", "path", "place", "visible")


# ------------------------------------------------------------------------------------------------------------ the crop
def ratios(u, scale_train_ratio=SCALE_TRAIN_RATIO, box_train_ratio=BOX_TRAIN_RATIO):
    """(the scale factor as numpy rounds it against a float32 array, the box ratio in binary64)."""
    return (F32(scale_train_ratio[0] + (scale_train_ratio[1] - scale_train_ratio[0]) * float(u[SCALE])),
            box_train_ratio[0] + (box_train_ratio[1] - box_train_ratio[0]) * float(u[BOX]))


def augment_one(img, mask, kpt_2d, bbox, u, input_size=(24, 32), scale_train_ratio=SCALE_TRAIN_RATIO, box_train_ratio=BOX_TRAIN_RATIO, train=True,
                mean=MEAN, std=STD):
    ih, iw = input_size
    x0, y0, x1, y1 = (int(v) for v in bbox)
    factor, box_ratio = ratios(u, scale_train_ratio, box_train_ratio)
    scale = np.array([max(x1 - x0 + 1, y1 - y0 + 1)] * 2, F32) * factor
    assert scale.dtype == F32
    center = np.array([(x0 + x1) / 2, (y0 + y1) / 2], F64)
    a = F64(iw) / F64(scale[0])
    trans = np.array([[a, 0., iw * 0.5 - a * center[0]], [0., a, ih * 0.5 - a * center[1]]], F64)
    rx0, ry0, rx1, ry1 = crop_twin.blank_rect((x0, y0, x1, y1), trans, (iw, ih), box_ratio)
    warped = crop_twin.warp_u8(img, trans, (iw, ih))
    orig = np.zeros_like(warped)
    orig[ry0:ry1 + 1, rx0:rx1 + 1] = warped[ry0:ry1 + 1, rx0:rx1 + 1]
    kpt = np.asarray(kpt_2d, F64)
    kpt = np.stack([(trans[0, 0] * kpt[:, 0] + trans[0, 1] * kpt[:, 1]) + trans[0, 2],
                    (trans[1, 0] * kpt[:, 0] + trans[1, 1] * kpt[:, 1]) + trans[1, 2]], axis=1)
    return {"inp": ct.colour(orig, u, mean, std, train), "orig_img": orig,
            "mask": ct.nearest_labels(mask.astype(np.uint8), crop_twin.invert_affine(trans), ih, iw).astype(np.uint8), "kpt_2d": kpt,
            "trans_input": trans, "center": center, "scale": scale, "box": np.array([rx0, ry0, rx1, ry1], np.int32)}


def augment(img, mask, kpt_2d, bbox, draws, **kw):
    outs = [augment_one(img[b], mask[b], kpt_2d[b], bbox[b], draws[b], **kw) for b in range(len(img))]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


AUGMENT_KEYS = ("inp", "orig_img", "mask", "kpt_2d", "trans_input", "center", "scale", "box")


# ------------------------------------------------------------------------------------------------------------ shared inputs
H0, W0, TH, TW, OH, OW, K0, N0 = 30, 50, 14, 18, 13, 17, 3, 2      # the canvas, the target's cut-out, the distractors' (odd), K, N
INPUT_SIZE = (24, 32)
DEG_345 = math.degrees(math.atan2(3, 4))                          # on a 12 x 16 cut-out h sin + w cos = 20 = D


def cutouts(shape, seed, value=1):
    """(img shape + [3] uint8, mask shape uint8) for shape [.., h, w]: seeded rectangles with a hole, values ``value``."""
    rng = np.random.default_rng(1000 + seed)
    h, w = shape[-2:]
    img = rng.integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    mask = np.zeros(shape, np.uint8)
    for i in np.ndindex(tuple(shape[:-2])):
        y0, x0 = rng.integers(1, h // 2), rng.integers(1, w // 2)
        y1, x1 = rng.integers(y0 + 4, h), rng.integers(x0 + 4, w)
        mask[i][y0:y1, x0:x1] = value
        mask[i][(y0 + y1) // 2, (x0 + x1) // 2] = 0
    return img, mask




def batch(B, seed, N=N0, K=K0, th=TH, tw=TW):
    """(bg, img, mask, kpt_2d, other_img, other_mask, draws) of a seeded batch on the small shapes; every other mask holds 255."""
    bg = np.stack([crop_twin.image(seed + b, H0, W0) for b in range(B)])
    img, mask = cutouts((B, th, tw), seed)
    mask[1::2] *= 255
    other_img, other_mask = cutouts((B, N, OH, OW), seed + 1)
    other_mask[:, 1::2] *= 255
    kpt = np.random.default_rng(2000 + seed).random((B, K, 2)) * [tw, th]
    return bg, img, mask, kpt, other_img, other_mask, draws_for(B, N, 3000 + seed)


def fused_backgrounds(bg):
    """Another image per sample for the fused canvas, so that the two backgrounds differ: the next sample's, upside down."""
    return np.stack([bg[(b + 1) % len(bg)][::-1] for b in range(len(bg))])


MTH, MTW = 12, 16                                                   # the mixed batch's target: a 3-4-5 rectangle, D = 20
DEG_345 = math.degrees(math.atan2(3, 4))                          # there h sin + w cos = 12 * 0.6 + 16 * 0.8 = 20 = D
MIXED_CASES = ("angle 0", "angle 90", "angle 180", "angle 45", "3-4-5", "on top by draw", "occluded and kept", "ratio met exactly",
               "just below the ratio", "fully occluded", "black fused background", "num = 0", "an empty distractor", "an empty target",
               "the target touches its cut-out's border", "the box clips", "a tie in np.round")
MIXED_AUGMENT_KW = dict(input_size=INPUT_SIZE, scale_train_ratio=(1.0, 3.0), box_train_ratio=(1.0, 1.5))


def _rect(shape, y0, y1, x0, x1, value=1):
    m = np.zeros(shape, np.uint8)
    m[y0:y1, x0:x1] = value
    return m


def mixed_batch():
    """One sample per entry of MIXED_CASES, in that order: (bg, img, mask, kpt_2d, other_img, other_mask, draws, compose_kw), to be
    augmented with MIXED_AUGMENT_KW.  The canvas is 30 x 50, the target's cut-out 12 x 16 (so that the 3-4-5 angle exists), the
    distractors' 13 x 17, N = 2, K = 3, ``rot_max`` and ``num`` are [B], ``ratio`` is 0.75.  The occlusion cases use unrotated
    rectangles so that the counts are known: the target is a 4 x 4 square of ones at (10, 20) on the canvas and distractor 0 a
    rectangle whose corner lies there too.  (A rotated cut-out larger than the canvas needs a smaller canvas: ``oversize_batch``.)"""
    B = len(MIXED_CASES)
    bg, img, mask, kpt, other_img, other_mask, d = batch(B, 90, th=MTH, tw=MTW)
    i = {name: k for k, name in enumerate(MIXED_CASES)}
    rot_max, num = np.full(B, 360.), np.full(B, N0, np.int64)
    d[:, TOP], d[:, BLACK] = 0.75, 0.5                                      # occluded, on the background, unless stated
    for name, deg in (("angle 0", 0.), ("angle 90", 90.), ("angle 180", 180.), ("angle 45", 45.), ("3-4-5", DEG_345)):
        rot_max[i[name]], d[i[name], ROT] = deg * 2, 0.5
    d[i["on top by draw"], TOP] = 0.25

    def occlusion(b, cover):
        rot_max[b] = 0.
        mask[b] = _rect((MTH, MTW), 3, 7, 5, 9)
        other_mask[b, 0], other_mask[b, 1] = cover, 0
        d[b, N_SAMPLE] = 0.
        ys, xs = np.nonzero(cover)
        d[b, DST_Y], d[b, DST_X] = 10.5 / (H0 - 3), 20.5 / (W0 - 3)
        d[b, N_SAMPLE + 1], d[b, N_SAMPLE + 2] = 10.5 / (H0 - (ys.max() - ys.min())), 20.5 / (W0 - (xs.max() - xs.min()))
    occlusion(i["occluded and kept"], _rect((OH, OW), 0, 1, 0, 2))          # 14 of 16 visible
    occlusion(i["ratio met exactly"], _rect((OH, OW), 0, 1, 0, 4))          # 12 of 16 = 0.75: kept, the test is strict
    below = _rect((OH, OW), 0, 1, 0, 4)
    below[1, 0] = 1
    occlusion(i["just below the ratio"], below)                             # 11 of 16
    occlusion(i["fully occluded"], _rect((OH, OW), 2, 8, 3, 9, 255))
    d[i["black fused background"], BLACK], d[i["black fused background"], TOP] = 0.95, 0.25
    num[i["num = 0"]] = 0
    other_mask[i["an empty distractor"], 0] = 0
    mask[i["an empty target"]] = 0
    b = i["the target touches its cut-out's border"]
    rot_max[b], mask[b] = 0., _rect((MTH, MTW), 0, MTH, 0, 6, 255)
    mask[b, MTH - 1, MTW - 1] = 255
    # the crop's cases: an unrotated target on top at a known place, no distractors
    for name in ("the box clips", "a tie in np.round"):
        b = i[name]
        rot_max[b], num[b], d[b, TOP] = 0., 0, 0.25
    b = i["the box clips"]                                                  # scale = the box' side: it fills the input's width and
    d[b, SCALE], d[b, BOX] = 0., 0.99                                       # overflows its height, and is magnified by 1.495
    mask[b] = _rect((MTH, MTW), 1, 11, 3, 13)
    b = i["a tie in np.round"]                                              # a 4 x 16 box, scale = 16 * 2 = 32 = iw, a = 1, ratio 1:
    mask[b] = _rect((MTH, MTW), 3, 7, 0, MTW)                               # x0' = 16 - 15 / 2 = 8.5 -> 8, x1' = 23.5 -> 24,
    d[b, SCALE], d[b, BOX] = 0.5, 0.                                        # y0' = 12 - 3 / 2 = 10.5 -> 10, y1' = 13.5 -> 14
    return bg, img, mask, kpt, other_img, other_mask, d, dict(rot_max=rot_max, num=num, ratio=0.75)


def oversize_batch():
    """A rotated cut-out larger than the canvas: a 10 x 12 canvas under the 14 x 18 target with a full mask turned by 45 degrees
    and a full 13 x 17 distractor: both are placed at 0 and their outside is dropped.  (bg, ..., draws, compose_kw)."""
    bg, img, mask, kpt, other_img, other_mask, d = batch(1, 95, N=1)
    bg = np.ascontiguousarray(bg[:, :10, :12])
    mask[:], other_mask[:] = 1, 1
    d[:, ROT], d[:, TOP] = 0.125, 0.75
    return bg, img, mask, kpt, other_img, other_mask, d, dict(rot_max=360., ratio=0.01)
