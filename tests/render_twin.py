"""numpy twin of the "Colour renders" contract of include/pvnet_vote.h, written from the contract with every operation explicit,
plus an independent ray caster that also reports which face it hit and where.

  render_color   one image: the geometry of tests/vsd_twin.py (its eye space, snapping, clip pieces and edge functions are
                 imported, not restated), the 64-bit ownership key and the shading lines in the header's order.  The device must
                 equal it byte for byte in img, label, depth, face and area.
  render_batch   the same for [B,M] poses.
  raycast        binary64 Moeller-Trumbore through (x + 0.5, y + 0.5) as vsd_twin.raycast_depth, extended to return the nearest
                 hit's face and barycentrics and the second-nearest depth: no snapping, no clipping pieces, no fill rule, no keys.
  shade_reference  a binary64 evaluation of the shading from the ray caster's hit: the barycentrics are Moeller-Trumbore's, not
                 the contract's cross products.
"""
import numpy as np

from tests import vsd_twin

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_M, MAX_FACES = 255, 1 << 24


def vertex_colors(seed, n):
    """Seeded uint8 colours [n,3]."""
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


def _object(ranges, o, N, F):
    """The range row of object ``o`` as the device tests it, or None: no instance."""
    if o < 0 or o >= len(ranges):
        return None
    v0, vn, f0, fn = (int(v) for v in ranges[o])
    if v0 < 0 or vn < 0 or v0 + vn > N or f0 < 0 or fn < 0 or f0 + fn > F:
        return None
    return v0, vn, f0, fn


def raster_keys(pts, faces, poses, K, size, ranges, obj, near, far):
    """The key image [H,W] uint64 of one image and the eye-space vertices of each instance (None where it draws nothing)."""
    W, H = size
    K = np.asarray(K, np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    near, far = np.float64(near), np.float64(far)
    keys = np.full((H, W), EMPTY, np.uint64)
    eyes = []
    for m, P in enumerate(np.asarray(poses, np.float64)):
        rng = _object(ranges, int(obj[m]), len(pts), len(faces))
        if rng is None or not np.isfinite(P).all():
            eyes.append(None)
            continue
        v0, vn, f0, fn = rng
        E = vsd_twin.eye_space(pts[v0:v0 + vn], P)
        eyes.append(E)
        with np.errstate(invalid="ignore"):
            ins = E[:, 2] >= near
        Us, Vs, oks = vsd_twin._snap(K, E[:, 0], E[:, 1], E[:, 2])
        oks = oks & ins
        for fi, f in enumerate(np.asarray(faces[f0:f0 + fn], np.int64)):
            if (f < 0).any() or (f >= vn).any():
                continue
            inside = ins[f]
            if not inside.any():
                continue
            ev = E[f]
            a, b = ev[1] - ev[0], ev[2] - ev[0]
            n0, n1, n2 = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
            num = (n0 * ev[0, 0] + n1 * ev[0, 1]) + n2 * ev[0, 2]
            sn = [(int(Us[i]), int(Vs[i]), bool(oks[i])) for i in f]
            tag = np.uint64((m << 24) | fi)
            for pc in vsd_twin._pieces(K, ev, sn, inside, near):
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
                c0, c1, c2 = (U0, V0), (U1, V1), (U2, V2)
                cov = vsd_twin._edge(c0, c1, px, py) & vsd_twin._edge(c1, c2, px, py) & vsd_twin._edge(c2, c0, px, py)
                if not cov.any():
                    continue
                with np.errstate(all="ignore"):
                    dy = (((ys.astype(np.float64) + 0.5) - cy) / fy)[:, None]
                    dx = (((xs.astype(np.float64) + 0.5) - cx)[None, :] - s * dy) / fx
                    den = (n0 * dx + n1 * dy) + n2
                    Z = num / den
                    keep = cov & (den != 0.0) & (Z >= near) & (Z <= far)
                    z32 = Z.astype(np.float32)
                key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tag
                sub = keys[ymin:ymax + 1, xmin:xmax + 1]
                sub[keep] = np.minimum(sub[keep], key[keep])
    return keys, eyes


def to_u8(v):
    """0 for v < 0 or NaN, 255 for v > 255, else floor(v + 0.5)."""
    with np.errstate(invalid="ignore"):
        r = np.floor(v + 0.5)
        r = np.where(v > 255.0, 255.0, r)
        r = np.where(v >= 0.0, r, 0.0)
    return r.astype(np.uint8)


def shade(E, C, K, x, y, ambient):
    """The shading lines of the header for arrays of owned pixels: E [P,3,3] the owners' eye-space vertices in face-row order,
    C [P,3,3] their uint8 colours, x, y [P].  Returns (rgb [P,3] uint8, Zd [P] binary64)."""
    K = np.asarray(K, np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    v0, v1, v2 = E[:, 0], E[:, 1], E[:, 2]
    a, b = v1 - v0, v2 - v0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    num = (n[:, 0] * v0[:, 0] + n[:, 1] * v0[:, 1]) + n[:, 2] * v0[:, 2]
    with np.errstate(all="ignore"):
        dy = ((y.astype(np.float64) + 0.5) - cy) / fy
        dx = (((x.astype(np.float64) + 0.5) - cx) - s * dy) / fx
        den = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2]
        Zd = num / den
        P = np.stack([dx * Zd, dy * Zd, Zd], 1)
        q = P - v0
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        qb = np.stack([q[:, 1] * b[:, 2] - q[:, 2] * b[:, 1], q[:, 2] * b[:, 0] - q[:, 0] * b[:, 2], q[:, 0] * b[:, 1] - q[:, 1] * b[:, 0]], 1)
        aq = np.stack([a[:, 1] * q[:, 2] - a[:, 2] * q[:, 1], a[:, 2] * q[:, 0] - a[:, 0] * q[:, 2], a[:, 0] * q[:, 1] - a[:, 1] * q[:, 0]], 1)
        w1 = ((qb[:, 0] * n[:, 0] + qb[:, 1] * n[:, 1]) + qb[:, 2] * n[:, 2]) / nn
        w2 = ((aq[:, 0] * n[:, 0] + aq[:, 1] * n[:, 1]) + aq[:, 2] * n[:, 2]) / nn
        w0 = (1.0 - w1) - w2
        Cd = C.astype(np.float64)
        c = (w0[:, None] * Cd[:, 0] + w1[:, None] * Cd[:, 1]) + w2[:, None] * Cd[:, 2]
        pp = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]
        diffuse = np.abs(num) / np.sqrt(nn * pp)
        t = np.float64(ambient) + diffuse
        light = np.where(t > 1.0, 1.0, t)
        v = light[:, None] * c
    return to_u8(v), Zd


def render_color(pts, colors, faces, poses, K, size, ranges=None, obj=None, bg=None, bg_color=(0, 0, 0), near=10.0, far=10000.0,
                 ambient=0.5):
    """One image of M instances: dict with img [H,W,3] uint8, label [H,W] uint8, depth [H,W] float32, face [H,W] int32 and area
    [M] int32.  ``poses`` [M,3,4]; ``obj`` [M] (default 0); ``ranges`` [O,4] (default one object)."""
    W, H = size
    pts, colors, faces = np.asarray(pts, np.float32), np.asarray(colors, np.uint8), np.asarray(faces, np.int32)
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    M = len(poses)
    assert 1 <= M <= MAX_M
    ranges = np.array([[0, len(pts), 0, len(faces)]], np.int32) if ranges is None else np.asarray(ranges, np.int32)
    assert int(ranges[:, 3].max()) <= MAX_FACES
    obj = np.zeros(M, np.int32) if obj is None else np.asarray(obj, np.int32)
    keys, eyes = raster_keys(pts, faces, poses, K, size, ranges, obj, near, far)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(bg_color, np.uint8) if bg is None else np.asarray(bg, np.uint8)
    label, depth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.float32)
    face, area = np.full((H, W), -1, np.int32), np.zeros(M, np.int32)
    ys, xs = np.nonzero(keys != EMPTY)
    if len(ys):
        k = keys[ys, xs]
        m = ((k >> np.uint64(24)) & np.uint64(0xFF)).astype(np.int64)
        f = (k & np.uint64(0xFFFFFF)).astype(np.int64)
        E, C = np.empty((len(k), 3, 3)), np.empty((len(k), 3, 3), np.uint8)
        for mm in np.unique(m):
            v0, vn, f0, fn = _object(ranges, int(obj[mm]), len(pts), len(faces))
            sel = m == mm
            rows = faces[f0:f0 + fn].astype(np.int64)[f[sel]]
            E[sel] = eyes[mm][rows]
            C[sel] = colors[v0:v0 + vn][rows]
        rgb, Zd = shade(E, C, K, xs, ys, ambient)
        z32 = Zd.astype(np.float32)
        assert np.array_equal(z32.view(np.uint32).astype(np.uint64), k >> np.uint64(32))      # depth equals the key's high word
        img[ys, xs], label[ys, xs], depth[ys, xs], face[ys, xs] = rgb, (m + 1).astype(np.uint8), z32, f.astype(np.int32)
        area = np.bincount(m, minlength=M).astype(np.int32)
    return {"img": img, "label": label, "depth": depth, "face": face, "area": area}


def render_batch(pts, colors, faces, poses, K, size, ranges=None, obj=None, bg=None, **kw):
    """[B,M] poses (or [B,3,4]): the stacked dict.  ``K`` [3,3] or [B,3,3], ``obj`` [B,M], ``bg`` [B,H,W,3]."""
    poses = np.asarray(poses, np.float64)
    if poses.ndim == 3:
        poses = poses[:, None]
    K = np.asarray(K, np.float64)
    outs = [render_color(pts, colors, faces, poses[b], K if K.ndim == 2 else K[b], size, ranges, None if obj is None else np.asarray(obj)[b],
                         None if bg is None else bg[b], **kw) for b in range(len(poses))]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def concat(meshes):
    """[(pts, colors, faces)] -> (pts, colors, faces, ranges), as SceneRenderer concatenates them."""
    rows, v0, f0 = [], 0, 0
    for p, c, f in meshes:
        rows.append((v0, len(p), f0, len(f)))
        v0, f0 = v0 + len(p), f0 + len(f)
    return (np.concatenate([m[0] for m in meshes]).astype(np.float32), np.concatenate([m[1] for m in meshes]).astype(np.uint8),
            np.concatenate([m[2] for m in meshes]).astype(np.int32), np.array(rows, np.int32))


# ---------------------------------------------------------------------------------------------------- the independent renderer
def raycast(pts, faces, P, K, size, near=100.0, far=10000.0):
    """dict: depth [H,W] binary64 (0 = background), second [H,W] (the next hit's depth, inf when there is none), face [H,W] (-1),
    u, v [H,W] (the hit is (1 - u - v) v0 + u v1 + v v2) and band [H,W] bool, the samples within 1/256 px of a projected edge of
    a near-clipped triangle -- the only ones where a rasteriser that snaps to 1/256 px may differ in coverage."""
    W, H = size
    K = np.asarray(K, np.float64)
    P = np.asarray(P, np.float64)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    ev_all = np.asarray(pts, np.float32).astype(np.float64) @ P[:, :3].T + P[:, 3]
    depth, second = np.full((H, W), np.inf), np.full((H, W), np.inf)
    face = np.full((H, W), -1, np.int64)
    bu, bv = np.zeros((H, W)), np.zeros((H, W))
    band = np.zeros((H, W), bool)
    for fi, f in enumerate(np.asarray(faces, np.int64)):
        ev = ev_all[f]
        poly = vsd_twin._clip_polygon(ev, near)
        if not poly:
            continue
        uv = np.array([[(fx * p[0] + s * p[1]) / p[2] + cx, fy * p[1] / p[2] + cy] for p in poly])
        x0, x1 = int(max(np.floor(uv[:, 0].min()) - 2, 0)), int(min(np.ceil(uv[:, 0].max()) + 2, W - 1))
        y0, y1 = int(max(np.floor(uv[:, 1].min()) - 2, 0)), int(min(np.ceil(uv[:, 1].max()) + 2, H - 1))
        if x0 > x1 or y0 > y1:
            continue
        sx, sy = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
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
        win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        nearer = hit & (t < depth[win])
        behind = hit & ~nearer
        second[win] = np.where(nearer, depth[win], np.where(behind, np.minimum(second[win], t), second[win]))
        depth[win] = np.where(nearer, t, depth[win])
        face[win] = np.where(nearer, fi, face[win])
        bu[win], bv[win] = np.where(nearer, u, bu[win]), np.where(nearer, v, bv[win])
        for i in range(len(poly)):
            pa, pb = uv[i], uv[(i + 1) % len(poly)]
            ab = pb - pa
            L2 = float(ab @ ab)
            w = np.clip(((sx - pa[0]) * ab[0] + (sy - pa[1]) * ab[1]) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(sx)
            dist = np.hypot(sx - (pa[0] + w * ab[0]), sy - (pa[1] + w * ab[1]))
            band[win] |= dist <= 1.0 / 256.0
    depth[~np.isfinite(depth)] = 0.0
    return {"depth": depth, "second": second, "face": face, "u": bu, "v": bv, "band": band, "eye": ev_all}


def shade_reference(rc, faces, colors, K, ambient):
    """The colour before rounding [H,W,3] binary64 from the ray caster's hits: Moeller-Trumbore's barycentrics, the hit point
    depth * (dx, dy, 1), the unit normal and the unit direction to the camera origin."""
    K = np.asarray(K, np.float64)
    H, W = rc["face"].shape
    out = np.zeros((H, W, 3))
    ys, xs = np.nonzero(rc["face"] >= 0)
    rows = np.asarray(faces, np.int64)[rc["face"][ys, xs]]
    E, C = rc["eye"][rows], np.asarray(colors, np.float64)[rows]
    u, v = rc["u"][ys, xs], rc["v"][ys, xs]
    c = (1.0 - u - v)[:, None] * C[:, 0] + u[:, None] * C[:, 1] + v[:, None] * C[:, 2]
    n = np.cross(E[:, 1] - E[:, 0], E[:, 2] - E[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    dyv = (ys + 0.5 - K[1, 2]) / K[1, 1]
    ray = np.stack([(xs + 0.5 - K[0, 2] - K[0, 1] * dyv) / K[0, 0], dyv, np.ones(len(ys))], 1)
    ray /= np.linalg.norm(ray, axis=1)[:, None]
    light = np.minimum(ambient + np.abs((n * ray).sum(1)), 1.0)
    out[ys, xs] = light[:, None] * c
    return out
