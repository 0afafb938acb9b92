"""numpy twin of the two arithmetic contracts of include/pvnet_vsd.h -- the depth rasteriser and the VSD arithmetic -- written
from the contract with every operation explicit, plus the seeded meshes and scenes of the fixtures, an independent ray
caster the rasteriser is checked against, and the one bound the device is held to.

  render_depth   the rasteriser: the device must equal it as float32 bit patterns.
  raycast_depth  binary64 Moeller-Trumbore through (x + 0.5, y + 0.5): no snapping, no clipping, no fill rule.  Snapping to
                 1/256 px moves a vertex by at most sqrt(2)/512 px < 1/256 px, so the two may disagree on coverage only at
                 samples within 1/256 px of a projected edge of a near-clipped triangle (``edge_band``); elsewhere the
                 depths differ by the float32 rounding of two binary64 evaluations of the same plane, 2**-23 relative.
  vsd_pair       misc.py:42-60, visibility.py:6-29 and vsd_utils.py:5-48 in the header's order; masks, counts and the
                 'step' error equal the reference's bit for bit (tests/golden/make_vsd_golden.py).
  tlinear        the fixed-order sum of the header.  Bound on the error e (u = 2**-53): two sums of the m = inter costs
                 c_k in [0, 1], S = sum c_k, taken in any two orders differ by at most 2*gamma_(m-1)*S <= 2.02*m*u*S (the
                 zeros of the pixels outside the intersection add exactly); e = (sum + integer) / union adds two roundings
                 on each side, 4.04*u*|e|:   |e_got - e_want| <= (2.02*m*S/union + 4.04*|e_want|) * u.
  lattice_soup, partition_mesh, size_class_mesh, clip_mesh, rules_images
                 constructed inputs (data only) that put an edge exactly through a sample, a piece exactly on the size at
                 which the sweep changes its path, a vertex exactly on the near plane or the snap limit, a visibility
                 difference exactly on delta and a cost exactly on tau -- what seeded, noisy scenes meet only by chance.
"""
import numpy as np

U = 2.0 ** -53
SNAP_LIMIT = 2.0 ** 28
TLESS_K = np.array([[1075.65091572, 0.0, 360.0], [0.0, 1073.90347929, 270.0], [0.0, 0.0, 1.0]])       # 720 x 540


def camera(scale=1.0, skew=0.0):
    """The T-LESS camera for an image ``scale`` times 720 x 540."""
    K = TLESS_K.copy()
    K[:2] *= scale
    K[0, 1] = skew
    return K


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose(w, t):
    return np.concatenate([rodrigues(w), np.asarray(t, np.float64).reshape(3, 1)], 1)


def scaled(P, t_scale):
    """[R | t * t_scale]: the evaluator's ``pose[:, 3:] * 1000`` (tless_test/pvnet.py:84, :91)."""
    P = np.array(P, np.float64)
    P[..., 3] = P[..., 3] * t_scale
    return P


def mesh(seed, nu=48, nv=24, R=60.0, r=25.0):
    """A seeded closed mesh with self-occlusion, in millimetres: a torus of 2 * nu * nv triangles with jittered vertices and
    randomly flipped faces (nothing is culled), one of its triangles replaced by three long ones that meet in a far apex --
    the mix of a few large and many small triangles of a CAD model.  float32 points [N,3], int32 faces [F,3]."""
    rng = np.random.RandomState(seed)
    a = 2 * np.pi * np.arange(nu) / nu
    b = 2 * np.pi * np.arange(nv) / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    pts = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], -1).reshape(-1, 3)
    pts = pts + rng.uniform(-0.4, 0.4, pts.shape)
    idx = lambda i, j: (i % nu) * nv + (j % nv)                                       # noqa: E731
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            faces.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    faces = np.array(faces, np.int64)
    k = int(rng.randint(len(faces)))
    tri = faces[k]
    c = pts[tri].mean(0)
    out = c - np.array([R * c[0], R * c[1], 0.0]) / np.hypot(c[0], c[1])              # away from the tube's centre line
    apex = c + 110.0 * out / np.linalg.norm(out) + rng.uniform(-30, 30, 3)
    pts = np.concatenate([pts, apex[None]])
    d = len(pts) - 1
    faces = np.concatenate([np.delete(faces, k, 0), [(tri[0], tri[1], d), (tri[1], tri[2], d), (tri[2], tri[0], d)]])
    flip = rng.rand(len(faces)) < 0.5
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return pts.astype(np.float32), faces.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the rasteriser
def eye_space(pts, P):
    """X = ((r00*x + r01*y) + r02*z) + t0 and rows 1, 2 alike: binary64 [N,3]."""
    m = np.asarray(pts, np.float32).astype(np.float64)
    P = np.asarray(P, np.float64)
    return np.stack([((P[i, 0] * m[:, 0] + P[i, 1] * m[:, 1]) + P[i, 2] * m[:, 2]) + P[i, 3] for i in range(3)], 1)


def _snap(K, X, Y, Z):
    """(U, V, ok): u = (fx*X + s*Y)/Z + cx, v = (fy*Y)/Z + cy, floor(256*. + 0.5); ok is False beyond 2**28 and for NaN."""
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    with np.errstate(all="ignore"):
        u = (fx * X + s * Y) / Z + cx
        v = (fy * Y) / Z + cy
        Ud, Vd = np.floor(256.0 * u + 0.5), np.floor(256.0 * v + 0.5)
        ok = (np.abs(Ud) <= SNAP_LIMIT) & (np.abs(Vd) <= SNAP_LIMIT)
    Ui = np.where(ok, Ud, 0.0).astype(np.int64)
    Vi = np.where(ok, Vd, 0.0).astype(np.int64)
    return Ui, Vi, ok


def _clip(K, p, q, near):
    """The snapped vertex where the edge from the inside vertex p to the outside vertex q meets Z = near."""
    with np.errstate(all="ignore"):
        t = (near - p[2]) / (q[2] - p[2])
        X = p[0] + t * (q[0] - p[0])
        Y = p[1] + t * (q[1] - p[1])
    Ui, Vi, ok = _snap(K, np.float64(X), np.float64(Y), np.float64(near))
    return int(Ui), int(Vi), bool(ok)


def _pieces(K, ev, sn, inside, near):
    """The one or two clipped pieces of a triangle as lists of three (U, V, ok); ``ev`` [3,3] eye-space vertices, ``sn`` the
    three snapped ones, ``inside`` the three Z >= near flags."""
    k = int(inside.sum())
    if k == 3:
        return [list(sn)]
    if k == 1:
        a = int(np.argmax(inside))
        b, c = (a + 1) % 3, (a + 2) % 3
        return [[sn[a], _clip(K, ev[a], ev[b], near), _clip(K, ev[a], ev[c], near)]]
    c = int(np.argmin(inside))
    a, b = (c + 1) % 3, (c + 2) % 3
    bc, ac = _clip(K, ev[b], ev[c], near), _clip(K, ev[a], ev[c], near)
    return [[sn[a], sn[b], bc], [sn[a], bc, ac]]


def _edge(a, b, px, py):
    dx, dy = b[0] - a[0], b[1] - a[1]
    E = dx * (py - a[1])[:, None] - dy * (px - a[0])[None, :]
    owns = dy > 0 or (dy == 0 and dx > 0)
    return (E > 0) | ((E == 0) & owns)


def render_depth(pts, faces, P, K, size, near=100.0, far=10000.0):
    """One pose: [H,W] float32, 0 = background.  The contract of include/pvnet_vsd.h, one operation per line of it."""
    W, H = size
    K = np.asarray(K, np.float64)
    P = np.asarray(P, np.float64)
    out = np.zeros((H, W), np.float32)
    if not np.isfinite(P).all():
        return out
    near, far = np.float64(near), np.float64(far)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    E = eye_space(pts, P)
    n = len(E)
    with np.errstate(invalid="ignore"):
        ins = E[:, 2] >= near
    Us, Vs, oks = _snap(K, E[:, 0], E[:, 1], E[:, 2])
    oks = oks & ins
    img = np.full((H, W), np.inf, np.float32)
    for f in np.asarray(faces, np.int64):
        if (f < 0).any() or (f >= n).any():
            continue
        inside = ins[f]
        if not inside.any():
            continue
        ev = E[f]
        a, b = ev[1] - ev[0], ev[2] - ev[0]
        n0, n1, n2 = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
        num = (n0 * ev[0, 0] + n1 * ev[0, 1]) + n2 * ev[0, 2]
        sn = [(int(Us[i]), int(Vs[i]), bool(oks[i])) for i in f]
        for pc in _pieces(K, ev, sn, inside, near):
            if not all(v[2] for v in pc):
                continue
            (U0, V0, _), (U1, V1, _), (U2, V2, _) = pc
            area2 = (U1 - U0) * (V2 - V0) - (V1 - V0) * (U2 - U0)
            if area2 == 0:
                continue
            if area2 < 0:
                U1, V1, U2, V2 = U2, V2, U1, V1
            xmin, xmax = max(-((128 - min(U0, U1, U2)) // 256), 0), min((max(U0, U1, U2) - 128) // 256, W - 1)
            ymin, ymax = max(-((128 - min(V0, V1, V2)) // 256), 0), min((max(V0, V1, V2) - 128) // 256, H - 1)
            if xmin > xmax or ymin > ymax:
                continue
            xs, ys = np.arange(xmin, xmax + 1, dtype=np.int64), np.arange(ymin, ymax + 1, dtype=np.int64)
            px, py = 256 * xs + 128, 256 * ys + 128
            v0, v1, v2 = (U0, V0), (U1, V1), (U2, V2)
            cov = _edge(v0, v1, px, py) & _edge(v1, v2, px, py) & _edge(v2, v0, px, py)
            if not cov.any():
                continue
            with np.errstate(all="ignore"):
                dy = (((ys.astype(np.float64) + 0.5) - cy) / fy)[:, None]
                dx = (((xs.astype(np.float64) + 0.5) - cx)[None, :] - s * dy) / fx
                den = (n0 * dx + n1 * dy) + n2
                Z = num / den
                keep = cov & (den != 0.0) & (Z >= near) & (Z <= far)
                z32 = Z.astype(np.float32)
            sub = img[ymin:ymax + 1, xmin:xmax + 1]
            sub[keep] = np.minimum(sub[keep], z32[keep])
    out[np.isfinite(img)] = img[np.isfinite(img)]
    return out


def render_batch(pts, faces, poses, K, size, near=100.0, far=10000.0):
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    K = np.asarray(K, np.float64)
    return np.stack([render_depth(pts, faces, P, K if K.ndim == 2 else K[i], size, near, far) for i, P in enumerate(poses)])


# ---------------------------------------------------------------------------------------------------- the independent renderer
def _clip_polygon(ev, near):
    """Sutherland-Hodgman against Z >= near: the eye-space polygon (0, 3 or 4 vertices)."""
    out = []
    for i in range(3):
        p, q = ev[i], ev[(i + 1) % 3]
        pin, qin = p[2] >= near, q[2] >= near
        if pin:
            out.append(p)
        if pin != qin:
            t = (near - p[2]) / (q[2] - p[2])
            out.append(p + t * (q - p))
    return out


def raycast_depth(pts, faces, P, K, size, near=100.0, far=10000.0):
    """(depth [H,W] binary64 with 0 = background, band [H,W] bool).  ``band`` marks the samples within 1/256 px of a
    projected edge of a near-clipped triangle -- the only samples where a rasteriser that snaps to 1/256 px may differ."""
    W, H = size
    K = np.asarray(K, np.float64)
    P = np.asarray(P, np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    ev_all = np.asarray(pts, np.float32).astype(np.float64) @ P[:, :3].T + P[:, 3]
    depth = np.full((H, W), np.inf)
    band = np.zeros((H, W), bool)
    for f in np.asarray(faces, np.int64):
        ev = ev_all[f]
        poly = _clip_polygon(ev, near)
        if not poly:
            continue
        uv = np.array([[(fx * v[0] + s * v[1]) / v[2] + cx, fy * v[1] / v[2] + cy] for v in poly])
        x0, x1 = int(max(np.floor(uv[:, 0].min()) - 2, 0)), int(min(np.ceil(uv[:, 0].max()) + 2, W - 1))
        y0, y1 = int(max(np.floor(uv[:, 1].min()) - 2, 0)), int(min(np.ceil(uv[:, 1].max()) + 2, H - 1))
        if x0 > x1 or y0 > y1:
            continue
        sx, sy = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        # the ray through the sample: origin 0, direction d with d_z = 1
        dyv = (sy - cy) / fy
        d = np.stack([(sx - cx - s * dyv) / fx, dyv, np.ones_like(sx)], -1)
        e1, e2 = ev[1] - ev[0], ev[2] - ev[0]
        h = np.cross(d, e2)
        a = h @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / a
            sv = -ev[0]
            u = inv * (h @ sv)
            q = np.cross(sv, e1)
            v = inv * (d @ q)
            t = inv * (e2 @ q)
            hit = (a != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= near) & (t <= far)
        sub = depth[y0:y1 + 1, x0:x1 + 1]
        sub[hit] = np.minimum(sub[hit], t[hit])
        for i in range(len(poly)):                                                   # distance of the samples to each edge
            pa, pb = uv[i], uv[(i + 1) % len(poly)]
            ab = pb - pa
            L2 = float(ab @ ab)
            w = np.clip(((sx - pa[0]) * ab[0] + (sy - pa[1]) * ab[1]) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(sx)
            dist = np.hypot(sx - (pa[0] + w * ab[0]), sy - (pa[1] + w * ab[1]))
            band[y0:y1 + 1, x0:x1 + 1] |= dist <= 1.0 / 256.0
    depth[~np.isfinite(depth)] = 0.0
    return depth, band


# ------------------------------------------------------------------------------------------------------------------ the scene
def scene_depth(seed, renders, occluder=True):
    """A seeded uint16 sensor image in units of 0.1 mm from the ground-truth renders [g,H,W] (mm): the nearest rendered
    surface or a background plane, Gaussian noise, a closer occluder over part of the object, holes."""
    rng = np.random.RandomState(seed)
    r = np.asarray(renders, np.float64)
    H, W = r.shape[1:]
    obj = np.where(r > 0, r, np.inf).min(0)
    d = np.where(np.isfinite(obj), obj, 1200.0) + rng.randn(H, W) * 2.0
    ys, xs = np.nonzero(np.isfinite(obj))
    if occluder and len(ys):
        y0, y1, x0, x1 = ys.min(), ys.max(), xs.min(), xs.max()
        oy, ox = y0 + (y1 - y0) // 2, x0 + (x1 - x0) // 3
        d[oy:y1 + 3, x0:ox] = max(obj[np.isfinite(obj)].min() - 60.0, 20.0) + rng.randn(*d[oy:y1 + 3, x0:ox].shape)
    d[rng.rand(H, W) < 0.03] = 0.0
    if len(ys):
        cy_, cx_ = int(ys.mean()), int(xs.mean())
        d[cy_:cy_ + max(H // 40, 2), cx_:cx_ + max(W // 20, 2)] = 0.0
    return np.clip(np.rint(d * 10.0), 0, 65535).astype(np.uint16)


# -------------------------------------------------------------------------------------------------------------------- VSD
def dist_image(depth, K):
    """Xs = ((x - cx)*depth)*(1/fx), Ys alike, sqrt((Xs*Xs + Ys*Ys) + depth*depth): binary64 [H,W]."""
    depth = np.asarray(depth).astype(np.float64)
    H, W = depth.shape
    xs = np.arange(W, dtype=np.float64)[None, :]
    ys = np.arange(H, dtype=np.float64)[:, None]
    Xs = ((xs - K[0, 2]) * depth) * (1.0 / K[0, 0])
    Ys = ((ys - K[1, 2]) * depth) * (1.0 / K[1, 1])
    return np.sqrt((Xs * Xs + Ys * Ys) + depth * depth)


def visible(dist_test, dist_model, delta):
    valid = (dist_test > 0) & (dist_model > 0)
    d_diff = dist_model.astype(np.float32) - dist_test.astype(np.float32)
    return (d_diff <= np.float32(delta)) & valid


def tile_sum(values):
    """The header's fixed-order sum of a flat binary64 array: tiles of 256, a binary tree per tile, tiles ascending."""
    v = np.asarray(values, np.float64).ravel()
    nt = -(-len(v) // 256)
    a = np.zeros(nt * 256)
    a[:len(v)] = v
    a = a.reshape(nt, 256)
    s = 128
    while s:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for t in a[:, 0]:
        total = total + t
    return float(total)


def vsd_pair(depth_est, depth_gt, depth_test, K, delta=15.0, tau=20.0, cost="step"):
    """One pair: ``depth_test`` in model units, binary64.  dict with e, union, inter, cost (the step count), visib_gt,
    visib_est and, for 'tlinear', cost_sum and m."""
    dist_test, dist_gt, dist_est = dist_image(depth_test, K), dist_image(depth_gt, K), dist_image(depth_est, K)
    vg = visible(dist_test, dist_gt, delta)
    ve = visible(dist_test, dist_est, delta) | (vg & (dist_est > 0))
    inter, union = vg & ve, vg | ve
    c = np.where(inter, np.abs(dist_gt - dist_est), 0.0)
    n_union, n_inter = int(union.sum()), int(inter.sum())
    n_cost = int((inter & (c >= tau)).sum())
    out = {"union": n_union, "inter": n_inter, "cost": n_cost, "visib_gt": vg, "visib_est": ve}
    if cost == "step":
        out["e"] = (n_cost + (n_union - n_inter)) / float(n_union) if n_union else 1.0
    else:
        cl = c * (1.0 / tau)
        cl = np.where(cl > 1.0, 1.0, cl)
        ssum = tile_sum(cl)
        out["cost_sum"], out["m"] = ssum, n_inter
        out["e"] = float((np.float64(ssum) + np.float64(n_union - n_inter)) / np.float64(n_union)) if n_union else 1.0
    return out


def tlinear_bound(e_want, m, cost_sum, union):
    """The largest |e_got - e_want| allowed with 'tlinear' (module docstring)."""
    if union == 0:
        return 0.0
    return (2.02 * m * abs(cost_sum) / union + 4.04 * abs(e_want)) * U


def sensor_depth(raw, depth_scale=0.1):
    """float64(raw) * depth_scale."""
    return np.asarray(raw).astype(np.float64) * depth_scale


def any_pair_hit(e, thresh=0.3, gt_valid=None):
    """tless_test/pvnet.py:100-103 for one image: e [p,g]."""
    h = np.asarray(e) < thresh
    if gt_valid is not None:
        h = h & np.asarray(gt_valid, bool)[None, :]
    return bool(h.any())


_CASES = {}


def regenerate(name, c):
    """What a fixture does not store, rebuilt from its seeds and poses (cached per process): the mesh, the renders of the
    predicted [n,p,H,W] and ground-truth [n,g,H,W] poses and the uint16 sensor images [n,H,W]."""
    if name not in _CASES:
        pts, faces = mesh(int(c["mesh_seed"]))
        size = (int(c["size"][0]), int(c["size"][1]))
        n, p = c["pose_est"].shape[:2]
        g = c["pose_gt"].shape[1]
        near, far, ts = float(c["near"]), float(c["far"]), float(c["t_scale"])
        est = render_batch(pts, faces, scaled(c["pose_est"], ts), c["K"], size, near, far).reshape(n, p, size[1], size[0])
        gt = render_batch(pts, faces, scaled(c["pose_gt"], ts), c["K"], size, near, far).reshape(n, g, size[1], size[0])
        raw = np.stack([scene_depth(int(c["scene_seed"][i]), gt[i]) for i in range(n)])
        _CASES[name] = {"pts": pts, "faces": faces, "size": size, "est": est, "gt": gt, "raw": raw}
    return _CASES[name]


# ------------------------------------------------------------------------------------- constructed inputs: exact boundary cases
# Data builders only.  Everything below lies on a lattice on which the contract's arithmetic is exact, so that an edge
# function is exactly zero, a visibility difference exactly delta and a cost exactly tau by construction, not by chance.
LATTICE_K = np.array([[128.0, 0.0, 0.0], [0.0, 128.0, 0.0], [0.0, 0.0, 1.0]])
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
LATTICE_NEAR, LATTICE_FAR = 1.0, 16.0


def lattice_points(u, v, Z):
    """float32 [N,3] points that LATTICE_K and the identity pose project to (u, v) exactly: u, v multiples of 1/2 px with a
    few bits, Z a power of two, X = u*Z/128 -- every operation of the contract is exact and U = 256*u."""
    u, v, Z = (np.asarray(a, np.float64) for a in (u, v, Z))
    p = np.stack([u * Z / 128.0, v * Z / 128.0, Z + 0.0 * u], -1)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p)
    return p32


def boundary_image(U, V, faces, size):
    """[H,W] bool: some face has the sample on the boundary of its closed triangle -- with the face oriented to positive
    area every integer edge function is >= 0 and one is == 0.  ``U``, ``V`` are the snapped coordinates of the vertices."""
    W, H = size
    px = (256 * np.arange(W, dtype=np.int64) + 128)[None, :]
    py = (256 * np.arange(H, dtype=np.int64) + 128)[:, None]
    out = np.zeros((H, W), bool)
    for f in np.asarray(faces, np.int64):
        x, y = [int(U[i]) for i in f], [int(V[i]) for i in f]
        area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area2 == 0:
            continue
        if area2 < 0:
            x[1], x[2], y[1], y[2] = x[2], x[1], y[2], y[1]
        E = [(x[(k + 1) % 3] - x[k]) * (py - y[k]) - (y[(k + 1) % 3] - y[k]) * (px - x[k]) for k in range(3)]
        out |= (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0) & ((E[0] == 0) | (E[1] == 0) | (E[2] == 0))
    return out


def lattice_soup(seed, size, n_vertices=30, n_faces=40):
    """A seeded triangle soup whose vertices project to multiples of 1/2 px in [-4, W+4) x [-4, H+4) at Z in {2, 4, 8}; the
    faces are random index triples (degenerate rows and repeated indices occur).  dict with pts, faces, K, pose, near, far
    and ``boundary``, the image of the samples that lie on the boundary of some face."""
    W, H = size
    rng = np.random.RandomState(seed)
    u = rng.randint(-8, 2 * (W + 4), n_vertices) / 2.0
    v = rng.randint(-8, 2 * (H + 4), n_vertices) / 2.0
    Z = 2.0 ** rng.randint(1, 4, n_vertices)
    faces = rng.randint(0, n_vertices, (n_faces, 3)).astype(np.int32)
    U, V = np.rint(256 * u).astype(np.int64), np.rint(256 * v).astype(np.int64)
    return {"pts": lattice_points(u, v, Z), "faces": faces, "K": LATTICE_K.copy(), "pose": IDENTITY.copy(), "size": (W, H),
            "near": LATTICE_NEAR, "far": LATTICE_FAR, "boundary": boundary_image(U, V, faces, size)}


def partition_mesh(seed, size):
    """A rectangle cut into cells by grid lines that lie alternately on sample centres (k + 0.5) and on integers, each cell
    split by a random diagonal into two triangles of random winding, at Z = 4.  ``closed_form`` is written by hand from the
    header's ownership rule, not rendered.  A piece is oriented to positive area with y pointing down, so its edges run
    top: left to right (dy = 0, dx > 0, owns), right: downwards (dy > 0, owns), bottom: right to left and left: upwards
    (neither owns).  The union is therefore 4.0 on the samples with x_left < x + 0.5 <= x_right and
    y_top <= y + 0.5 < y_bottom, and 0 elsewhere."""
    W, H = size
    rng = np.random.RandomState(seed)

    def lines(limit):
        at = [0.5 if rng.rand() < 0.5 else 1.0]
        while at[-1] + 2.5 <= limit - 1:
            at.append(at[-1] + (1.5 if rng.rand() < 0.5 else 2.5))       # an odd number of half pixels: centre, integer, ...
        return np.array(at)

    gx, gy = lines(W), lines(H)
    nx, ny = len(gx), len(gy)
    uu, vv = np.meshgrid(gx, gy)
    pts = lattice_points(uu.ravel(), vv.ravel(), np.full(nx * ny, 4.0))
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            pair = [(a, b, c), (a, c, d)] if rng.rand() < 0.5 else [(a, b, d), (b, c, d)]
            for t in pair:
                t = t[::-1] if rng.rand() < 0.5 else t
                k = int(rng.randint(3))
                faces.append(t[k:] + t[:k])
    xs, ys = np.arange(W) + 0.5, np.arange(H) + 0.5
    inside = ((gy[0] <= ys) & (ys < gy[-1]))[:, None] & ((gx[0] < xs) & (xs <= gx[-1]))[None, :]
    return {"pts": pts, "faces": np.array(faces, np.int32), "K": LATTICE_K.copy(), "pose": IDENTITY.copy(), "size": (W, H),
            "near": LATTICE_NEAR, "far": LATTICE_FAR, "closed_form": np.where(inside, np.float32(4.0), np.float32(0.0)),
            "lines": (gx, gy)}


def size_class_mesh():
    """The size classes of the sweep on a 130 x 70 image (17 x 9 = 153 blocks of 8x8): named faces first, then a seeded mix
    of pieces of at most 32 samples (swept by a lane) and of more (swept by the wave), 300 faces in all.  ``named`` maps a
    name to its face row."""
    W, H = 130, 70
    u, v, Z, faces, named = [], [], [], [], {}

    def tri(name, *vs):
        named[name] = len(faces)
        faces.append(tuple(range(len(u), len(u) + 3)))
        for (a, b, z) in vs:
            u.append(a), v.append(b), Z.append(z)

    big = 2.0 ** 19                                                                  # snapped: 2**27
    tri("whole", (-big, -big, 8.0), (big, -big, 8.0), (0.0, big, 4.0))               # covers every sample, 153 blocks
    # the right angle at the bottom right: the last sample of the box in row-major order, the 32nd or 33rd, is covered
    tri("box32", (10.5, 14.0, 2.0), (18.0, 14.0, 2.0), (18.0, 10.5, 2.0))            # 8 x 4 samples: the lane's largest
    tri("box33", (30.5, 13.0, 2.0), (41.0, 13.0, 2.0), (41.0, 10.5, 2.0))            # 11 x 3 samples: the wave's smallest
    tri("sliver", (0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (130.0, 70.0, 2.0))              # corner to corner, one pixel wide
    tri("blocks65", (0.0, 40.0, 4.0), (104.0, 40.0, 4.0), (104.0, 0.0, 4.0))         # 13 x 5 blocks: one past a wave's 64
    tri("limit", (2.0 ** 20, 30.0, 2.0), (-10.0, 20.0, 2.0), (-10.0, 40.0, 2.0))     # |U| = 2**28 exactly: kept
    tri("beyond", (2.0 ** 20 + 0.5, 55.0, 2.0), (-10.0, 50.0, 2.0), (-10.0, 60.0, 2.0))    # one lattice step more: dropped
    tri("beyond_v", (60.0, -(2.0 ** 20) - 0.5, 2.0), (50.0, 80.0, 2.0), (70.0, 80.0, 2.0))
    # wave-swept pieces with a block whose only inside sample is its extreme corner, exactly on an edge that owns its line:
    # the largest edge function over that block is 0, and the block must not be rejected
    tri("corner_col", (24.5, 44.0, 2.0), (24.5, 56.0, 2.0), (12.0, 50.0, 2.0))        # right edge on a block's first column
    tri("corner_row", (100.0, 47.5, 2.0), (120.0, 47.5, 2.0), (110.0, 60.0, 2.0))    # top edge on a block's last row
    tri("corner_slant", (42.5, 49.5, 2.0), (58.5, 65.5, 2.0), (38.5, 65.5, 2.0))     # a slanted edge through block corners
    rng = np.random.RandomState(11)
    while len(faces) < 300:
        reach = 8 if len(faces) % 2 else 40                                          # half pixels: at most 5 x 5 samples, or many
        cu, cv = rng.randint(0, 2 * W), rng.randint(0, 2 * H)
        z = 2.0 if reach == 8 else 4.0
        tri("soup%d" % len(faces), *[((cu + rng.randint(0, reach + 1)) / 2.0, (cv + rng.randint(0, reach + 1)) / 2.0,
                                      z * 2.0 ** rng.randint(0, 2)) for _ in range(3)])
    return {"pts": lattice_points(u, v, Z), "faces": np.array(faces, np.int32), "K": LATTICE_K.copy(), "pose": IDENTITY.copy(),
            "size": (W, H), "near": LATTICE_NEAR, "far": LATTICE_FAR, "named": named}


def clip_mesh():
    """Near-plane clipping on the lattice: near = 4 and vertices at Z in {2, 4, 8}, so a vertex lies outside, exactly on the
    plane (inside) or inside.  Named fans whose faces share clipped edges, a seeded soup with zero to three vertices
    inside, and two fronto-parallel quads, one at Z == far and one at the next float32 above it."""
    W, H = 29, 23
    near, far = 4.0, 8.0
    u, v, Z, faces = [], [], [], []

    def vert(a, b, z):
        u.append(a), v.append(b), Z.append(z)
        return len(u) - 1

    # a fan around an outside centre: every rim edge is whole, every spoke is clipped and shared by two faces
    c = vert(8.0, 8.0, 2.0)
    rim = [vert(8.0 + dx, 8.0 + dy, z) for dx, dy, z in ((-6.5, -5.0, 8.0), (5.5, -6.0, 4.0), (7.0, 4.5, 8.0), (-1.0, 7.5, 8.0),
                                                           (-7.0, 3.0, 4.0))]
    for k in range(5):
        f = (c, rim[k], rim[(k + 1) % 5])
        faces.append(f if k % 2 else f[::-1])                                        # two inside: two pieces each
    # a fan around an inside centre with an outside rim: one inside, one piece each; rim vertex 2 lies on the plane
    c = vert(21.0, 8.5, 8.0)
    rim = [vert(21.0 + dx, 8.5 + dy, z) for dx, dy, z in ((-5.0, -6.5, 2.0), (6.0, -4.0, 2.0), (6.5, 5.5, 4.0), (-4.5, 6.0, 2.0))]
    for k in range(4):
        f = (rim[k], rim[(k + 1) % 4], c)
        faces.append(f if k % 2 else (f[1], f[2], f[0]))
    rng = np.random.RandomState(23)
    n0 = len(u)
    for _ in range(24):
        vert(rng.randint(-8, 2 * (W + 4)) / 2.0, rng.randint(-8, 2 * (H + 4)) / 2.0, 2.0 ** rng.randint(1, 4))
    for _ in range(80):
        faces.append(tuple(int(i) for i in rng.randint(n0, n0 + 24, 3)))
    pts = [lattice_points(u, v, Z)]
    n = len(u)
    for z in (np.float32(far), np.nextafter(np.float32(far), np.float32(np.inf))):    # kept (Z <= far), dropped
        x0, x1 = (1.5, 12.0) if z == np.float32(far) else (15.0, 27.5)
        quad = np.array([[x0, 15.0], [x1, 15.0], [x1, 22.5], [x0, 22.5]]) * np.float64(z) / 128.0
        pts.append(np.concatenate([quad, np.full((4, 1), np.float64(z))], 1).astype(np.float32))
        faces += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
        n += 4
    return {"pts": np.concatenate(pts), "faces": np.array(faces, np.int32), "K": LATTICE_K.copy(), "pose": IDENTITY.copy(),
            "size": (W, H), "near": near, "far": far, "far_quads": (len(faces) - 4, len(faces) - 2)}


def piece_boxes(m):
    """Per face of a constructed mesh ``m``: the number of vertices inside the near plane and, per clipped piece that is
    swept, (samples in its clamped bounding box, blocks of 8x8 its box touches) -- what decides the path the sweep takes."""
    W, H = m["size"]
    K, near = m["K"], np.float64(m["near"])
    E = eye_space(m["pts"], m["pose"])
    ins = E[:, 2] >= near
    Us, Vs, oks = _snap(K, E[:, 0], E[:, 1], E[:, 2])
    oks = oks & ins
    out = []
    for f in np.asarray(m["faces"], np.int64):
        boxes = []
        if ins[f].any():
            sn = [(int(Us[i]), int(Vs[i]), bool(oks[i])) for i in f]
            for pc in _pieces(K, E[f], sn, ins[f], near):
                (U0, V0, _), (U1, V1, _), (U2, V2, _) = pc
                if not all(q[2] for q in pc) or (U1 - U0) * (V2 - V0) - (V1 - V0) * (U2 - U0) == 0:
                    continue
                xmin, xmax = max(-((128 - min(U0, U1, U2)) // 256), 0), min((max(U0, U1, U2) - 128) // 256, W - 1)
                ymin, ymax = max(-((128 - min(V0, V1, V2)) // 256), 0), min((max(V0, V1, V2) - 128) // 256, H - 1)
                if xmin <= xmax and ymin <= ymax:
                    boxes.append(((xmax - xmin + 1) * (ymax - ymin + 1),
                                  ((xmax >> 3) - (xmin >> 3) + 1) * ((ymax >> 3) - (ymin >> 3) + 1)))
        out.append((int(ins[f].sum()), boxes))
    return out


def block_corner_samples(m, k):
    """For face ``k`` of a constructed mesh with every vertex inside: the covered samples (x, y) that are the extreme
    corner of an 8x8 block of the wave sweep at which an edge function that owns its line has its largest value over the
    block, and that value is 0 -- the block holds covered samples only because `largest < 0` rejects and `<= 0` would.
    Integer arithmetic on the snapped coordinates, the block clamped to the piece's box as the sweep does."""
    W, H = m["size"]
    E = eye_space(m["pts"], m["pose"])
    f = np.asarray(m["faces"], np.int64)[k]
    assert (E[f, 2] >= m["near"]).all()
    Us, Vs, oks = _snap(m["K"], E[f, 0], E[f, 1], E[f, 2])
    assert oks.all()
    v = [(int(Us[i]), int(Vs[i])) for i in range(3)]
    if (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) - (v[1][1] - v[0][1]) * (v[2][0] - v[0][0]) < 0:
        v[1], v[2] = v[2], v[1]
    xmin, xmax = max(-((128 - min(q[0] for q in v)) // 256), 0), min((max(q[0] for q in v) - 128) // 256, W - 1)
    ymin, ymax = max(-((128 - min(q[1] for q in v)) // 256), 0), min((max(q[1] for q in v) - 128) // 256, H - 1)
    edges = [(v[i], v[(i + 1) % 3]) for i in range(3)]

    def fn(e, x, y):
        (ax, ay), (bx, by) = e
        return (bx - ax) * (256 * y + 128 - ay) - (by - ay) * (256 * x + 128 - ax)

    out = []
    for by_ in range(ymin >> 3, (ymax >> 3) + 1):
        for bx_ in range(xmin >> 3, (xmax >> 3) + 1):
            x0, x1, y0, y1 = max(8 * bx_, xmin), min(8 * bx_ + 7, xmax), max(8 * by_, ymin), min(8 * by_ + 7, ymax)
            for e in edges:
                dx, dy = e[1][0] - e[0][0], e[1][1] - e[0][1]
                cx_, cy_ = (x0 if dy > 0 else x1), (y1 if dx > 0 else y0)          # where this edge function is largest
                owns = dy > 0 or (dy == 0 and dx > 0)
                if owns and fn(e, cx_, cy_) == 0 and all(fn(o, cx_, cy_) > 0 or (fn(o, cx_, cy_) == 0 and (
                        o[1][1] - o[0][1] > 0 or (o[1][1] == o[0][1] and o[1][0] > o[0][0]))) for o in edges):
                    out.append((cx_, cy_))
    return sorted(set(out))


def next32(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def prev32(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


RULES_K = np.diag([2.0 ** 60, 2.0 ** 60, 1.0])                  # dist == depth exactly
RULES_DELTA, RULES_TAU = 15.0, 20.0
_T30 = 2.0 ** -30
# (test, gt, est, visib_gt, visib_est) with delta = 15: the masks are written by hand from visibility.py:6-29
RULES_TABLE = (
    (1000.0, 1015.0, 1015.0, 1, 1),                             # a difference of exactly delta: visible
    (1000.0, next32(1015.0), 1015.0, 0, 1),                     # one float32 step more: not
    (1000.0, 1015.0, next32(1015.0), 1, 1),                     # est is visible only through visib_gt
    (1000.0 - _T30, 1015.0, 1015.0, 1, 1),                      # exactly delta in float32; more than delta in binary64
    (1000.0 + _T30, 1015.0, 1015.0, 1, 1),
    (0.0, 1000.0, 1000.0, 0, 0),                                # no sensor reading
    (1000.0, 0.0, 1000.0, 0, 1),
    (1000.0, 1000.0, 0.0, 1, 0),
    (0.0, 0.0, 0.0, 0, 0),
    (1000.0, 1010.0, 1100.0, 1, 1),                             # est is visible only through visib_gt and dist_est > 0
    (1000.0, 1100.0, 1010.0, 0, 1),
    (1000.0, 1100.0, 1100.0, 0, 0),
    (1000.0, 1000.0, 1020.0, 1, 1),                             # a cost of exactly tau counts
    (1000.0, 1000.0, prev32(1020.0), 1, 1),                     # one float32 step less does not
    (1000.0, 1000.0, next32(1020.0), 1, 1),
    (1000.0, 1020.0, 1000.0, 0, 1),
)
RULES_F64_ROWS = (3, 4)                                         # the rows that need a binary64 sensor image


def _rules_fill(rng, n, test=None):
    """Seeded (test, gt, est) [n]: non-negative multiples of 1/8 below 4096, the differences on and next to delta and tau."""
    steps_v = np.array([-30.0, -15.125, -15.0, -14.875, 0.0, 14.875, 15.0, 15.125, 30.0])
    steps_c = np.array([-40.0, -20.125, -20.0, -19.875, 0.0, 19.875, 20.0, 20.125, 40.0])
    if test is None:
        test = 1000.0 + rng.randint(0, 801, n) / 8.0
        test[rng.rand(n) < 0.1] = 0.0
    gt = np.where(test > 0, test, 1000.0) + steps_v[rng.randint(0, 9, n)]
    est = gt + steps_c[rng.randint(0, 9, n)]
    gt[rng.rand(n) < 0.1] = 0.0
    est[rng.rand(n) < 0.1] = 0.0
    return test, gt, est


def rules_images():
    """name -> (depth_test [H,W] f64, depth_gt [g,H,W] f32, depth_est [p,H,W] f32) under RULES_K:
      f64    3 x 100 (two tiles of 256 pixels, the second partial), p = g = 2; pair (0, 0) starts with RULES_TABLE
      f32    the same without the two rows that need binary64: every value is a float32 and a multiple of 1/8
      small  1 x 37, a single partial tile, p = g = 1, the table of ``f32`` first
      zero   3 x 100, every image zero: union == 0
    ``rules_uint16`` gives the sensor image of all but ``f64`` as uint16 at depth_scale 0.125."""
    out = {}
    for name, (H, W), pg, rows in (("f64", (3, 100), 2, range(len(RULES_TABLE))),
                                   ("f32", (3, 100), 2, [k for k in range(len(RULES_TABLE)) if k not in RULES_F64_ROWS]),
                                   ("small", (1, 37), 1, [k for k in range(len(RULES_TABLE)) if k not in RULES_F64_ROWS])):
        rng = np.random.RandomState(77)
        test, gt0, est0 = _rules_fill(rng, H * W)
        gts, ests = [gt0], [est0]
        for _ in range(pg - 1):
            _, g, e = _rules_fill(rng, H * W, test)
            gts.append(g), ests.append(e)
        for j, k in enumerate(rows):
            test[j], gts[0][j], ests[0][j] = RULES_TABLE[k][:3]
        gt, est = np.stack(gts).reshape(pg, H, W), np.stack(ests).reshape(pg, H, W)
        for a in (test, gt, est):
            assert (a >= 0).all() and (a < 4096).all()
        assert np.array_equal(gt.astype(np.float32).astype(np.float64), gt) and np.array_equal(est.astype(np.float32), est)
        out[name] = (test.reshape(H, W), gt.astype(np.float32), est.astype(np.float32))
    out["zero"] = (np.zeros((3, 100)), np.zeros((1, 3, 100), np.float32), np.zeros((1, 3, 100), np.float32))
    return out


def rules_uint16(depth_test):
    """The sensor image as uint16 in units of 1/8 (depth_scale = 0.125): the same numbers."""
    raw = np.asarray(depth_test, np.float64) * 8.0
    assert np.array_equal(raw, np.rint(raw)) and raw.max() < 65536
    return raw.astype(np.uint16)
