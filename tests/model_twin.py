"""numpy twin of the three contracts of include/pvnet_vote.h's "Model metadata" section, with the operation order explicit:
farthest point sampling in float32, the diameter in binary64, the bounds.  The CPU tests pin this twin to the fixtures made by
the reference's own ``farthest_point_sampling.cpp`` and ``calc_pts_diameter`` (tests/golden/make_model_golden.py); the GPU
tests hold the device to the twin as bytes.  The clouds are made from seeds here, and the case table both test files use is
at the end.  Nothing here is a tolerance: every comparison on top of this module is exact."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
TILE = 1024                        # PVV_MODEL_TILE: points per workgroup of the tiled kernels
ONE_BLOCK_LANES = 1024             # the ONE_BLOCK workgroup: above it a lane holds more than one point


# ------------------------------------------------------------------------------------------------ the contracts
def _d2(p, q):
    """((p.x-q.x)^2 + (p.y-q.y)^2) + (p.z-q.z)^2 for every row of p, one rounding per operation, in the dtype of p."""
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == p.dtype
    return d


def _pick(md, chosen):
    """The lowest unchosen index of the largest min_dist if that is > 0, otherwise 0."""
    m = np.where(chosen, md.dtype.type(-1), md)
    j = int(np.argmax(m))                                                           # argmax returns the first maximum
    return j if m[j] > 0 else 0


def _fps(p, sn, start, big):
    n = p.shape[0]
    md, chosen = np.full(n, big, p.dtype), np.zeros(n, bool)
    if start is None:
        c = (p.max(0) + p.min(0)) * p.dtype.type(0.5)
        d = _d2(p, c)
        md = np.where(big < d, big, d)
        cur = _pick(md, chosen)
    else:
        assert 0 <= start < n
        cur = int(start)
    idx = np.zeros(sn, np.int32)
    for k in range(sn):
        chosen[cur] = True
        idx[k] = cur
        if k < sn - 1:
            d = _d2(p, p[cur])
            md = np.where(~chosen & (d < md), d, md)
            cur = _pick(md, chosen)
    return idx


def fps(points, sn, start=None):
    """The indices of the contract: float32; ``start`` None is the centre start."""
    return _fps(np.ascontiguousarray(points, F32), int(sn), start, F32(FLT_MAX))


def fps_binary64(points, sn, start=None):
    """The same selection rule evaluated in binary64: what the float32 twin must give on clouds whose distances are far
    enough apart that no float32 rounding changes an order."""
    return _fps(np.ascontiguousarray(points, np.float64), int(sn), start, np.float64(np.finfo(np.float64).max))


def diameter(points, chunk=256):
    """sqrt of the largest (dx*dx + dy*dy) + dz*dz over all pairs, binary64; float32 input is widened exactly."""
    p = np.ascontiguousarray(points).astype(np.float64)
    best = np.float64(0.0)
    for i0 in range(0, p.shape[0], chunk):
        q = p[i0:i0 + chunk]
        dx, dy, dz = q[:, None, 0] - p[None, i0:, 0], q[:, None, 1] - p[None, i0:, 1], q[:, None, 2] - p[None, i0:, 2]
        best = max(best, ((dx * dx + dy * dy) + dz * dz).max())
    return np.float64(np.sqrt(best))


def bounds(points):
    p = np.asarray(points)
    return p.min(0), p.max(0)


def corners(points):
    """tools/handle_custom_dataset.py:26-40 restated: x slowest, min before max."""
    lo, hi = bounds(points)
    return np.array([[(lo, hi)[i >> 2 & 1][0], (lo, hi)[i >> 1 & 1][1], (lo, hi)[i & 1][2]] for i in range(8)], np.asarray(points).dtype)


def center(points):
    lo, hi = bounds(points)
    return (hi + lo) / 2


# ------------------------------------------------------------------------------------------------ the clouds
KINDS = ("gauss", "lattice", "repeated", "planar")


def cloud(kind, n, seed):
    """A seeded float32 cloud of n points.
    gauss     anisotropic Gaussian of LINEMOD scale (metres)
    lattice   integer coordinates in [0, 6): many equal distances (the tie rule) and equal points
    repeated  ceil(n / 50) distinct points, each up to 50 times, shuffled: sampling more than that many reaches the index-0 rule
    planar    z = 0.25 for every point"""
    rng = np.random.RandomState(seed)
    if kind == "gauss":
        return (rng.randn(n, 3) * np.array([0.04, 0.03, 0.02])).astype(F32)
    if kind == "lattice":
        return rng.randint(0, 6, (n, 3)).astype(F32)
    if kind == "repeated":
        base = (rng.randn((n + 49) // 50, 3) * 0.05).astype(F32)
        return base[rng.permutation(np.arange(n) // 50)]
    if kind == "planar":
        m = (rng.randn(n, 3) * 0.05).astype(F32)
        m[:, 2] = 0.25
        return m
    raise KeyError(kind)


def planted(n, seed, ia, ib, dtype=F32):
    """A Gaussian cloud inside the unit ball's tenth with the extreme pair planted at indices ia and ib (ia == ib, n == 1: one
    far point).  The coordinates are not representable in float32 when dtype is float64, so that the widening matters."""
    rng = np.random.RandomState(seed)
    m = np.clip(rng.randn(n, 3) * 0.03, -0.1, 0.1).astype(dtype)
    far = np.asarray(rng.uniform(0.5, 1.0, 3), dtype)
    m[ia] = far
    m[ib] = -far
    return m


# ------------------------------------------------------------------------------------------------ the case table
# The smallest sizes at which the kernels can go wrong: a wave (64), a workgroup of the tiled kernels (256), the ONE_BLOCK
# workgroup (1024: above it a lane holds several points), a tile (1024) and a last partial tile after two full ones.
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2 * TILE + 17)


def sample_counts(n):
    return (1, 2, 8, n + 3)


def starts(n):
    """None is the centre start."""
    return [None] + sorted({0, n // 2, n - 1})


def kind_seed(kind, n):
    return 1000 * KINDS.index(kind) + n


_want = {}


def reference(kind, n, start):
    """The twin's indices for the largest sample count of the table (8 for n < 5, else n + 3); a smaller count is their prefix (a round never looks at
    sn except to stop).  Computed once and shared; the arrays are not writeable."""
    key = (kind, n, start)
    if key not in _want:
        idx = fps(cloud(kind, n, kind_seed(kind, n)), max(sample_counts(n)), start)
        idx.setflags(write=False)
        _want[key] = idx
    return _want[key]


# Where the extreme pair sits in the diameter cases, by size: (name, ia, ib).
def plant_places(n):
    places = [("ends", 0, n - 1)]
    if n > 2 * TILE + 1:
        places += [("last_partial_tile", 2 * TILE + 1, n - 2), ("one_tile", TILE + 5, 2 * TILE - 3)]
    if n > 3 * TILE:
        places += [("two_middle_tiles", TILE + 7, 2 * TILE + 9)]
    return places


DIAMETER_SIZES = (1, 2, 65, 257, 1024, 1025, 2 * TILE + 17, 3 * TILE + 17)

# The fixtures of tests/golden/make_model_golden.py: name -> (kind, n, seed, sn), or the points themselves when tiny.
A, B = [0.25, -0.5, 1.0], [-1.5, 0.125, 0.75]
GOLDEN = {
    "gauss_n700": ("gauss", 700, 1, 8),
    "gauss_n2500": ("gauss", 2500, 2, 20),
    "lattice_n1100": ("lattice", 1100, 3, 12),
    "repeated_n600": ("repeated", 600, 4, 20),
    "planar_n300": ("planar", 300, 5, 8),
    "sn_gt_n": ("gauss", 5, 6, 9),
    "one_point": (np.array([A], F32), 3),
    "abba": (np.array([A, B, B, A], F32), 6),
}


def golden_points(name):
    c = GOLDEN[name]
    return (c[0], c[1]) if len(c) == 2 else (cloud(c[0], c[1], c[2]), c[3])
