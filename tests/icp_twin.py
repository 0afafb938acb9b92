"""numpy twin of the arithmetic contract of include/pvnet_icp.h -- one stage of the ICP refinement, binary64, one operation per
line of the contract, the same two fixed-order sums and the same rotation sequence -- plus the seeded scenes of the fixtures.
The render, the meshes and the sensor images come from tests/vsd_twin.py.  The device must equal ``refine`` bit for bit;
tests/golden/make_icp_golden.py holds ``refine`` to the reference's own ``ICPRefiner.refine`` on the fixtures.
"""
import math

import numpy as np

from tests import vsd_twin as vt

STATUS = ("refined", "empty_render", "not_visible", "rotation_limit", "bad_pose", "small_mask", "bad_index")
REFINED, EMPTY_RENDER, NOT_VISIBLE, ROTATION_LIMIT, BAD_POSE, SMALL_MASK, BAD_INDEX = range(7)
SWEEPS = 30
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ------------------------------------------------------------------------------------------------------------------- sums
def tile_sum(v):
    return vt.tile_sum(v)


def stride_sum(v):
    """STRIDE of the header along axis 0: slot j = ((v_j + v_(j+256)) + v_(j+512)) + ..., then one tree over the slots."""
    v = np.asarray(v, np.float64)
    m = v.shape[0]
    nt = max(-(-m // 256), 1)
    a = np.zeros((nt * 256,) + v.shape[1:])
    a[:m] = v
    a = a.reshape((nt, 256) + v.shape[1:])
    acc = np.zeros((256,) + v.shape[1:])
    for t in range(nt):
        acc = acc + a[t]
    s = 128
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


# ----------------------------------------------------------------------------------------------------------------- clouds
def back_project(K, z):
    """x = ((u - cx)*z)/fx, y = ((v - cy)*z)/fy over the whole image: [H,W] each."""
    H, W = z.shape
    us = np.arange(W, dtype=np.float64)[None, :]
    vs = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = ((us - K[0, 2]) * z) / K[0, 0]
        y = ((vs - K[1, 2]) * z) / K[1, 1]
    return x, y


def dist2(x, y, z, c):
    with np.errstate(all="ignore"):
        dx, dy, dz = x - c[0], y - c[1], z - c[2]
        return (dx * dx + dy * dy) + dz * dz


def synthetic_stats(render, K):
    """(n_syn, centroid [3], max_d2, points [n_syn,3] in row-major order) of the float32 render widened to binary64."""
    z = np.asarray(render, np.float32).astype(np.float64)
    x, y = back_project(K, z)
    inc = z != 0.0
    n_syn = int(inc.sum())
    with np.errstate(all="ignore"):
        cen = np.array([np.float64(tile_sum(np.where(inc, a, 0.0))) / np.float64(n_syn) for a in (x, y, z)])
    pts = np.stack([x[inc], y[inc], z[inc]], 1)
    max_d2 = float(dist2(pts[:, 0], pts[:, 1], pts[:, 2], cen).max()) if n_syn else 0.0
    return n_syn, cen, max_d2, pts


def real_points(z_img, mask, K, cen, thr):
    """The kept sensor points [n_real,3] in row-major order: mask == 1, z != 0, sqrt(d2) < thr."""
    z = np.asarray(z_img, np.float64)
    x, y = back_project(K, z)
    with np.errstate(all="ignore"):
        keep = (z != 0.0) & (np.sqrt(dist2(x, y, z, cen)) < thr)
    if mask is not None:
        keep &= np.asarray(mask).astype(np.int64) == 1
    return np.stack([x[keep], y[keep], z[keep]], 1)


def draw(words, count):
    """idx = (word * count) >> 32 on the low 32 bits of each word."""
    w = np.asarray(words).astype(np.uint64) & np.uint64(0xffffffff)
    return ((w * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the fit
def rotation_of(S):
    """Horn's N from S, cyclic Jacobi in the header's order, the quaternion's matrix.  np.float64 scalars throughout."""
    S = np.asarray(S, np.float64)
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (np.float64(v) for v in S.ravel())
    N = np.zeros((4, 4))
    N[0, 0] = (Sxx + Syy) + Szz
    N[1, 1] = (Sxx - Syy) - Szz
    N[2, 2] = (Syy - Sxx) - Szz
    N[3, 3] = (Szz - Sxx) - Syy
    N[0, 1] = N[1, 0] = Syz - Szy
    N[0, 2] = N[2, 0] = Szx - Sxz
    N[0, 3] = N[3, 0] = Sxy - Syx
    N[1, 2] = N[2, 1] = Sxy + Syx
    N[1, 3] = N[3, 1] = Szx + Sxz
    N[2, 3] = N[3, 2] = Syz + Szy
    V = np.eye(4)
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            rotated = False
            for p, q in PAIRS:
                g = abs(N[p, q])
                if g == 0.0 or (abs(N[p, p]) + g == abs(N[p, p]) and abs(N[q, q]) + g == abs(N[q, q])):
                    N[p, q] = N[q, p] = 0.0
                    continue
                rotated = True
                apq = N[p, q]
                theta = (N[q, q] - N[p, p]) / (2.0 * apq)
                r = np.sqrt(theta * theta + one)
                tt = one / (abs(theta) + r)
                if theta < 0.0:
                    tt = -tt
                c = one / np.sqrt(tt * tt + one)
                s = tt * c
                N[p, p] = N[p, p] - tt * apq
                N[q, q] = N[q, q] + tt * apq
                N[p, q] = N[q, p] = 0.0
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = N[k, p], N[k, q]
                        N[k, p] = N[p, k] = c * akp - s * akq
                        N[k, q] = N[q, k] = s * akp + c * akq
                for k in range(4):
                    vkp, vkq = V[k, p], V[k, q]
                    V[k, p] = c * vkp - s * vkq
                    V[k, q] = s * vkp + c * vkq
            if not rotated:
                break
        j = 0
        for k in range(1, 4):
            if N[k, k] > N[j, j]:
                j = k
        w, x, y, z = (np.float64(v) for v in V[:, j])
        nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        return np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]])


def fit(a, b, depth_only=False, no_depth=False):
    """(R [3,3], t [3]) of the pairs a_i -> b_i (best_fit_transform, icp_utils.py:35-80)."""
    n = np.float64(len(a))
    cA, cB = stride_sum(a) / n, stride_sum(b) / n
    if depth_only and not no_depth:
        return np.eye(3), cB - cA
    AA, BB = a - cA, b - cB
    S = stride_sum(AA[:, :, None] * BB[:, None, :])
    R = rotation_of(S)
    t = np.array([cB[k] - ((R[k, 0] * cA[0] + R[k, 1] * cA[1]) + R[k, 2] * cA[2]) for k in range(3)])
    if no_depth and not depth_only:
        t[2] = 0.0
    return R, t


def apply(R, t, s):
    return np.stack([((R[k, 0] * s[:, 0] + R[k, 1] * s[:, 1]) + R[k, 2] * s[:, 2]) + t[k] for k in range(3)], 1)


def nearest(src, dst, chunk=512):
    """(index [n], squared distance [n]): (ex*ex + ey*ey) + ez*ez, the lowest index wins a tie."""
    idx = np.empty(len(src), np.int64)
    d2m = np.empty(len(src))
    for i in range(0, len(src), chunk):
        s = src[i:i + chunk]
        ex, ey, ez = (s[:, k, None] - dst[None, :, k] for k in range(3))
        d2 = (ex * ex + ey * ey) + ez * ez
        j = d2.argmin(1)
        idx[i:i + chunk] = j
        d2m[i:i + chunk] = d2[np.arange(len(s)), j]
    return idx, d2m


def icp(A, B, depth_only=False, no_depth=False, max_iterations=200, tolerance=5e-7, trace=None):
    """(R, t, rounds) of icp (icp_utils.py:83-126).  ``trace`` collects |prev - mean| of every round."""
    src = np.array(A, np.float64)
    n = np.float64(len(A))
    prev = np.float64(0.0)
    rounds = 0
    for _ in range(max_iterations):
        j, d2 = nearest(src, B)
        mean = stride_sum(np.sqrt(d2)) / n
        R, t = fit(src, B[j], depth_only, no_depth)
        src = apply(R, t, src)
        rounds += 1
        step = abs(prev - mean)
        if trace is not None:
            trace.append(float(step))
        prev = mean
        if step < tolerance:
            break
    R, t = fit(A, src, depth_only, no_depth)
    return R, t, rounds


def cos_limit(angle_limit_deg):
    return math.cos(float(angle_limit_deg) * math.pi / 180.)


def refine(z_img, pose, K, pts, faces, size, mask=None, depth_only=False, no_depth=False, max_mean_dist_factor=2.0, n_max=3000,
           max_iterations=200, tolerance=5e-7, angle_limit_deg=20.0, near=100.0, far=10000.0, samples=None, words=None,
           min_mask_pixels=0, render=None, trace=None):
    """One stage for one pose.  ``z_img`` [H,W] binary64 sensor depth in model units; ``samples`` = (idx_syn, idx_real) or
    ``words`` [2,n_max].  Returns (pose [3,4], info dict: status, n_syn, n_real, n, rounds; and ``cos`` when it was tested)."""
    pose = np.array(pose, np.float64)
    K = np.asarray(K, np.float64)
    info = {"status": REFINED, "n_syn": 0, "n_real": 0, "n": 0, "rounds": 0}
    if render is None:
        render = vt.render_depth(pts, faces, pose, K, size, near, far)
    n_syn, cen, max_d2, syn = synthetic_stats(render, K)
    info["n_syn"] = n_syn
    real = np.zeros((0, 3))
    if n_syn:
        real = real_points(z_img, mask, K, cen, np.float64(max_mean_dist_factor) * np.sqrt(np.float64(max_d2)))
    n_real = info["n_real"] = len(real)
    n = min(n_real, n_syn, int(n_max))
    if not np.isfinite(pose).all() or not pose[2, 3] > 0.0:
        info["status"] = BAD_POSE
    elif mask is not None and int((np.asarray(mask).astype(np.int64) == 1).sum()) < min_mask_pixels:
        info["status"] = SMALL_MASK
    elif n_syn == 0:
        info["status"] = EMPTY_RENDER
    elif np.float64(n_real) < np.float64(n_syn) / 20.0:
        info["status"] = NOT_VISIBLE
    if info["status"] != REFINED:
        return pose, info
    info["n"] = n
    if samples is not None:
        i_syn, i_real = (np.asarray(s).astype(np.int64)[:n] for s in samples)
    else:
        i_syn, i_real = draw(words[0][:n], n_syn), draw(words[1][:n], n_real)
    if (i_syn < 0).any() or (i_syn >= n_syn).any() or (i_real < 0).any() or (i_real >= n_real).any():
        info["status"] = BAD_INDEX
        return pose, info
    R, t, rounds = icp(syn[i_syn], real[i_real], depth_only, no_depth, max_iterations, tolerance, trace)
    info["rounds"] = rounds
    if no_depth:
        info["cos"] = float((((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0) / 2.0)
        if info["cos"] < cos_limit(angle_limit_deg):
            info["status"] = ROTATION_LIMIT
            return pose, info
    out = np.empty((3, 4))
    E, te = pose[:, :3], pose[:, 3]
    for k in range(3):
        for l in range(3):
            out[k, l] = E[k, l] if (depth_only and not no_depth) else (R[k, 0] * E[0, l] + R[k, 1] * E[1, l]) + R[k, 2] * E[2, l]
        out[k, 3] = ((R[k, 0] * te[0] + R[k, 1] * te[1]) + R[k, 2] * te[2]) + t[k]
    return out, info


def icp_refine(pose, z_img, mask, K, pts, faces, size, t_scale=1000.0, samples=None, words=None, traces=(None, None), **kw):
    """The two stages of Evaluator.icp_refine for one pose in metres: (pose [3,4], (info1, info2), (stage poses in mm))."""
    p0 = np.array(pose, np.float64)
    mm = np.concatenate([p0[:, :3], p0[:, 3:] * t_scale], 1)
    s1, s2 = samples if samples is not None else (None, None)
    w1, w2 = words if words is not None else (None, None)
    r1, i1 = refine(z_img, mm, K, pts, faces, size, mask=mask, depth_only=True, max_mean_dist_factor=5.0, samples=s1, words=w1,
                    trace=traces[0], **kw)
    r2, i2 = refine(z_img, r1, K, pts, faces, size, mask=mask, no_depth=True, max_mean_dist_factor=2.0, samples=s2, words=w2,
                    trace=traces[1], **kw)
    out = np.concatenate([r2[:, :3], r1[:, 3:] / t_scale], 1)
    if i1["status"] >= BAD_POSE:
        out = p0
    return out, (i1, i2), (r1, r2)


# ------------------------------------------------------------------------------------------------------------- the scenes
_CASES = {}


def regenerate(name, c):
    """What a fixture does not store, rebuilt from its seeds and poses (cached per process): the mesh, the uint16 sensor
    images [n,H,W] (the ground-truth poses of an image rendered into one scene), and the uint8 masks [P,H,W] -- the
    ground-truth render of each pose, cut after the first ``mask_keep`` part of its rows."""
    if name not in _CASES:
        pts, faces = vt.mesh(int(c["mesh_seed"]))
        size = (int(c["size"][0]), int(c["size"][1]))
        P, n = len(c["pose_gt"]), len(c["scene_seed"])
        per = P // n
        gt = vt.render_batch(pts, faces, vt.scaled(c["pose_gt"], float(c["t_scale"])), c["K"], size)
        raw = np.stack([vt.scene_depth(int(c["scene_seed"][i]), gt[i * per:(i + 1) * per], occluder=bool(c["occluder"]))
                        for i in range(n)])
        mask = np.zeros(gt.shape, np.uint8)
        for p in range(P):
            ys = np.nonzero((gt[p] > 0).any(1))[0]
            if len(ys):
                y1 = ys[0] + int(round(float(c["mask_keep"][p]) * (ys[-1] - ys[0] + 1)))
                mask[p, :y1] = gt[p, :y1] > 0
        _CASES[name] = {"pts": pts, "faces": faces, "size": size, "raw": raw, "mask": mask, "per_image": per}
    return _CASES[name]
