"""Model metadata on the MI355X (clean_pvnet_amd.model): the sampled indices, the diameter and the bounds equal the numpy twin
(tests/model_twin.py, itself held to the reference's own results in tests/test_model.py) as bytes, on a side stream as on the
default stream, with ONE_BLOCK and TILED forced at every wave, workgroup and tile seam; a ragged batch never reads its padding;
the reference's own indices and diameters (tests/golden/model_*.npz) come out; the drop-in import path returns the twin's
points."""
import os

import numpy as np
import pytest

from tests import model_twin as twin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def on_both_streams(f):
    """f() on a side stream and on the default stream: the two results are the same bytes; returns them as numpy."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = f()
    side.synchronize()
    a, b = a.cpu().numpy(), f().cpu().numpy()
    assert a.tobytes() == b.tobytes(), "the side stream's result differs from the default stream's"
    return a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
        w = np.argwhere(got != want) if got.shape == want.shape else []
        print("%s: got %s %s, want %s %s; %d differ, first at %s: %r vs %r"
              % (what, got.dtype, got.shape, want.dtype, want.shape, len(w), tuple(w[0]) if len(w) else None,
                 got[tuple(w[0])] if len(w) else None, want[tuple(w[0])] if len(w) else None))
        return False
    return True


def _paths(model):
    return (("ONE_BLOCK", model.ONE_BLOCK), ("TILED", model.TILED))


# ------------------------------------------------------------------------------------------------------------ 1. FPS
@pytest.mark.parametrize("n", twin.SIZES)
def test_fps_equals_the_twin_in_both_forms(pkg, gpu, n):
    from clean_pvnet_amd import model
    bad = []
    for kind in twin.KINDS:
        pts = _t(gpu, twin.cloud(kind, n, twin.kind_seed(kind, n)))
        for start in twin.starts(n):
            want = twin.reference(kind, n, start)
            for sn in twin.sample_counts(n):
                got = {}
                for name, path in _paths(model):
                    got[name] = on_both_streams(lambda: model.farthest_point_sampling(pts, sn, start is None, start, path=path))
                    if not _same(got[name], want[:sn], "%s n=%d start=%s sn=%d %s" % (kind, n, start, sn, name)):
                        bad.append((kind, start, sn, name))
                assert got["ONE_BLOCK"].tobytes() == got["TILED"].tobytes() or bad
    assert not bad, bad


def test_fps_auto_takes_the_form_the_size_asks_for(pkg, gpu):
    from clean_pvnet_amd import model
    for n in (65, model.ONE_BLOCK_MAX + 1):                                         # AUTO: ONE_BLOCK, then TILED (9 tiles)
        p = twin.cloud("gauss", n, 3)
        got = on_both_streams(lambda: model.farthest_point_sampling(_t(gpu, p), 8))
        assert _same(got, twin.fps(p, 8), "auto n=%d" % n)
    p = twin.cloud("lattice", model.ONE_BLOCK_MAX, 4)                               # the largest ONE_BLOCK cloud: eight points per lane
    got = on_both_streams(lambda: model.farthest_point_sampling(_t(gpu, p), 8, False, model.ONE_BLOCK_MAX - 1, path=model.ONE_BLOCK))
    assert _same(got, twin.fps(p, 8, model.ONE_BLOCK_MAX - 1), "one block, full")
    with pytest.raises(ValueError, match="8192"):
        model.farthest_point_sampling(_t(gpu, twin.cloud("gauss", model.ONE_BLOCK_MAX + 1, 3)), 8, path=model.ONE_BLOCK)


def test_fps_ragged_batch_never_reads_its_padding(pkg, gpu):
    from clean_pvnet_amd import model
    N = 2 * twin.TILE + 17
    lens = [1, 64, 65, 1025, N]
    clouds = [twin.cloud(twin.KINDS[b % 4], v, 50 + b) for b, v in enumerate(lens)]
    batch = np.full((5, N, 3), np.nan, np.float32)
    for b, c in enumerate(clouds):
        batch[b, :len(c)] = c
    dev = _t(gpu, batch)
    for sn in (8, 70):
        for name, path in _paths(model):
            for start in (None, [0, 63, 32, 1024, N - 1]):
                got = on_both_streams(lambda: model.farthest_point_sampling(dev, sn, start is None, start, n=lens, path=path))
                assert got.shape == (5, sn)
                for b, c in enumerate(clouds):
                    s = None if start is None else start[b]
                    single = model.farthest_point_sampling(_t(gpu, c), sn, s is None, s, path=path).cpu().numpy()
                    assert single.shape == (sn,) and _same(got[b], single, "ragged %s sn=%d cloud %d" % (name, sn, b))
                    assert _same(got[b], twin.fps(c, sn, s), "ragged twin %s sn=%d cloud %d" % (name, sn, b))


@pytest.mark.parametrize("name", list(twin.GOLDEN))
def test_fps_gives_the_references_own_indices(pkg, gpu, name):
    from clean_pvnet_amd import model
    g = np.load(os.path.join(GOLDEN, "model_%s.npz" % name))
    pts, sn = twin.golden_points(name)
    dev = _t(gpu, pts)
    for pname, path in _paths(model) + (("AUTO", model.AUTO),):
        got = on_both_streams(lambda: model.farthest_point_sampling(dev, sn, True, path=path))
        assert _same(got, g["idx_center"], "%s centre %s" % (name, pname))
        got = on_both_streams(lambda: model.farthest_point_sampling(dev, sn, False, int(g["start"]), path=path))
        assert _same(got, g["idx_random"], "%s start %s" % (name, pname))


def test_fps_draws_a_start_on_the_host_when_none_is_given(pkg, gpu):
    from clean_pvnet_amd import model
    p = twin.cloud("gauss", 300, 8)
    got = model.farthest_point_sampling(_t(gpu, p), 6, init_center=False).cpu().numpy()
    assert 0 <= got[0] < 300 and _same(got, twin.fps(p, 6, int(got[0])), "random start")


# ------------------------------------------------------------------------------------------------------------ 2. the diameter
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", twin.DIAMETER_SIZES)
def test_diameter_equals_the_twin(pkg, gpu, n, dtype):
    from clean_pvnet_amd import model
    for place, ia, ib in twin.plant_places(n):
        p = twin.planted(n, 7 * n + ia, ia, ib, dtype)
        got = on_both_streams(lambda: model.diameter(_t(gpu, p)[None]))
        want = twin.diameter(p)
        print("n=%d %s %s: device %.17g twin %.17g" % (n, np.dtype(dtype).name, place, got[0], want))
        assert _same(got, np.array([want]), "diameter n=%d %s" % (n, place))
        assert n == 1 or want > 1.7                                                  # the planted pair: twice a vector of three coordinates >= 0.5
    same = np.full((n, 3), 0.3, dtype)
    assert _same(on_both_streams(lambda: model.diameter(_t(gpu, same)[None])), np.zeros(1), "all points equal, n=%d" % n)
    if n == 1:
        assert _same(model.diameter(_t(gpu, twin.planted(1, 3, 0, 0, dtype))[None]).cpu().numpy(), np.zeros(1), "one point")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_diameter_ragged_batch_never_reads_its_padding(pkg, gpu, dtype):
    from clean_pvnet_amd import model
    N = 2 * twin.TILE + 17
    lens = [1, 64, 65, 1025, N]
    clouds = [twin.planted(v, 60 + b, 0, v // 2, dtype) for b, v in enumerate(lens)]
    batch = np.full((5, N, 3), 1e30, dtype)                                         # would win if it were read
    for b, c in enumerate(clouds):
        batch[b, :len(c)] = c
    got = on_both_streams(lambda: model.diameter(_t(gpu, batch), n=lens))
    assert _same(got, np.array([twin.diameter(c) for c in clouds]), "ragged diameter")
    lo, hi = model.bounds(_t(gpu, batch), n=lens)
    assert np.array_equal(lo.cpu().numpy(), np.stack([c.min(0) for c in clouds]))
    assert np.array_equal(hi.cpu().numpy(), np.stack([c.max(0) for c in clouds]))


@pytest.mark.parametrize("name", list(twin.GOLDEN))
def test_diameter_gives_the_references_own_value(pkg, gpu, name):
    from clean_pvnet_amd import model
    g = np.load(os.path.join(GOLDEN, "model_%s.npz" % name))
    pts, _ = twin.golden_points(name)
    for p in (pts, pts.astype(np.float64)):
        got = on_both_streams(lambda: model.diameter(_t(gpu, p)[None]))
        assert _same(got, g["diameter"].reshape(1), "%s %s" % (name, p.dtype))


# ------------------------------------------------------------------------------------------------------------ 3. the box
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounds_corners_and_centre_equal_numpy(pkg, gpu, dtype):
    import torch
    from clean_pvnet_amd import model
    for n in (1, 65, 257, 1025, 2 * twin.TILE + 17):
        clouds = np.stack([twin.planted(n, 80 + b, b % n, (n - 1 - b) % n, dtype) for b in range(3)])
        dev = _t(gpu, clouds)
        lo, hi = model.bounds(dev)
        assert lo.dtype == hi.dtype == dev.dtype and tuple(lo.shape) == (3, 3)
        lo = on_both_streams(lambda: model.bounds(dev)[0])
        hi = on_both_streams(lambda: model.bounds(dev)[1])
        assert np.array_equal(lo, clouds.min(1)) and np.array_equal(hi, clouds.max(1))
        corner = on_both_streams(lambda: model.model_corners(dev))
        centre = on_both_streams(lambda: model.model_center(dev))
        assert corner.dtype == centre.dtype == np.dtype(dtype)
        for b in range(3):
            assert np.array_equal(corner[b], twin.corners(clouds[b])), (n, b)       # the row order of get_model_corners
            assert np.array_equal(centre[b], twin.center(clouds[b])), (n, b)
    assert isinstance(lo, np.ndarray) and torch.cuda.is_available()


def test_model_meta_equals_its_parts(pkg, gpu):
    from clean_pvnet_amd import model
    N = 2 * twin.TILE + 17
    lens = [700, N, 65]
    batch = np.full((3, N, 3), np.nan, np.float32)
    for b, v in enumerate(lens):
        batch[b, :v] = twin.cloud("gauss", v, 90 + b)
    dev = _t(gpu, batch)
    meta = model.model_meta(dev, 8, n=lens)
    assert sorted(meta) == ["center_3d", "corner_3d", "diameter", "fps_3d", "fps_idx"]
    idx = model.farthest_point_sampling(dev, 8, n=lens).cpu().numpy()
    assert _same(meta["fps_idx"].cpu().numpy(), idx, "fps_idx")
    assert _same(meta["fps_3d"].cpu().numpy(), np.stack([batch[b][idx[b]] for b in range(3)]), "fps_3d")
    assert _same(meta["corner_3d"].cpu().numpy(), model.model_corners(dev, lens).cpu().numpy(), "corner_3d")
    assert _same(meta["center_3d"].cpu().numpy(), model.model_center(dev, lens).cpu().numpy(), "center_3d")
    assert _same(meta["diameter"].cpu().numpy(), model.diameter(dev, lens).cpu().numpy(), "diameter")
    for b, v in enumerate(lens):                                                    # and the parts are the twin's
        assert _same(idx[b], twin.fps(batch[b, :v], 8), "meta fps %d" % b)
        assert meta["diameter"][b].item() == twin.diameter(batch[b, :v])
        assert np.array_equal(meta["corner_3d"][b].cpu().numpy(), twin.corners(batch[b, :v]))


# ------------------------------------------------------------------------------------------------------------ 4. the drop-in path
def test_drop_in_fps_utils_returns_the_twins_points(pkg, gpu):
    from lib.csrc.fps import fps_utils
    pts = twin.cloud("gauss", 5841, 11).astype(np.float64)                          # a .ply's coordinates arrive as they are stored
    got = fps_utils.farthest_point_sampling(pts, 8, True)
    p32 = pts.astype(np.float32)
    assert got.dtype == np.float32 and _same(got, p32[twin.fps(p32, 8)], "fps_utils, centre start")
    assert len(np.unique(p32, axis=0)) == len(p32)                                  # no duplicates: the first point names its index
    got = fps_utils.farthest_point_sampling(pts, 8)                                 # init_center=False: a random first sample
    first = np.flatnonzero((p32 == got[0]).all(1))
    assert len(first) == 1 and _same(got, p32[twin.fps(p32, 8, int(first[0]))], "fps_utils, random start")
