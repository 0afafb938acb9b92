"""The batched depth rasteriser and VSD (include/pvnet_vsd.h, clean_pvnet_amd.vsd) without a GPU: the numpy twin of the
rasteriser's contract against an independent ray caster, the twin's VSD arithmetic against fixtures made by the reference's
own functions (tests/golden/make_vsd_golden.py), the library's exports and its host-side argument checks.  The GPU tests
(tests/test_gpu_vsd.py) then hold the device to the twin bit for bit."""
import os

import numpy as np
import pytest

from tests import capi
from tests import vsd_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("vsd_720", "vsd_360", "vsd_near")
RULES = "vsd_rules"                                  # constructed images, stored whole (make_vsd_golden.py::make_rules)
SOUP_SIZES = ((37, 29), (5, 4), (67, 3), (1, 1))     # the sizes tests/test_gpu_vsd_rules.py renders the lattice soups at


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_module_imports(pkg):
    from clean_pvnet_amd import vsd
    assert vsd.COSTS == {"step": 0, "tlinear": 1} and callable(vsd.render_depth) and callable(vsd.vsd)
    assert callable(vsd.vsd_from_depth)


# --------------------------------------------------------------------------------- 1. the twin against an independent renderer
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_rasteriser_against_the_ray_caster(name):
    """Coverage equal on every sample farther than 1/256 px from every projected edge of a near-clipped triangle (snapping
    moves a vertex by at most sqrt(2)/512 px), depth within 2**-23 relative there (float32 rounding), and those samples are
    at least 98 % of the covered ones -- a condition on the fixture, not a tolerance."""
    c = load(name)
    r = twin.regenerate(name, c)
    near, far = float(c["near"]), float(c["far"])
    poses = np.concatenate([twin.scaled(c["pose_est"], float(c["t_scale"])).reshape(-1, 3, 4),
                            twin.scaled(c["pose_gt"], float(c["t_scale"])).reshape(-1, 3, 4)])
    renders = np.concatenate([r["est"].reshape((-1,) + r["est"].shape[2:]), r["gt"].reshape((-1,) + r["gt"].shape[2:])])
    checked = 0
    for P, got in zip(poses, renders):
        want, band = twin.raycast_depth(r["pts"], r["faces"], P, c["K"], r["size"], near, far)
        cov_t, cov_r = got > 0, want > 0
        covered = int((cov_t | cov_r).sum())
        if covered == 0:
            assert not band.any() or not cov_t.any()
            continue
        excluded = int(((cov_t | cov_r) & band).sum())
        ok = ~band
        diff_cov = int((cov_t != cov_r)[ok].sum())
        both = ok & cov_t & cov_r
        rel = np.abs(got.astype(np.float64)[both] - want[both]) / want[both]
        print("%s: covered %d, excluded %d (%.2f %%), coverage differences %d, largest relative depth difference %.3g" %
              (name, covered, excluded, 100.0 * excluded / covered, diff_cov, rel.max() if rel.size else 0.0))
        assert excluded <= 0.02 * covered
        assert diff_cov == 0
        assert rel.size and rel.max() <= 2.0 ** -23
        checked += 1
    assert checked >= 2


def test_near_fixture_straddles_the_near_plane_and_mesh_mixes_sizes():
    c = load("vsd_near")
    pts, faces = twin.mesh(int(c["mesh_seed"]))
    Z = twin.eye_space(pts, twin.scaled(c["pose_gt"], float(c["t_scale"]))[0, 0])[:, 2]
    ins = Z[faces] >= float(c["near"])
    assert (ins.sum(1) == 1).any() and (ins.sum(1) == 2).any() and (ins.sum(1) == 0).any() and (ins.sum(1) == 3).any()
    assert len(faces) == 2 * 48 * 24 + 2
    e = pts[faces].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(e[:, 1] - e[:, 0], e[:, 2] - e[:, 0]), axis=1)
    assert area.max() > 10 * np.median(area)                             # the three long triangles of the apex


def test_twin_rasteriser_rules():
    """The fill rule on a shared edge, the half-pixel sample, depth of a fronto-parallel plane, and bad input."""
    K = np.array([[100.0, 0.0, 0.0], [0.0, 100.0, 0.0], [0.0, 0.0, 1.0]])
    P = twin.pose([0, 0, 0], [0, 0, 0])
    # a square [0.02, 0.06]^2 at Z = 2 -> pixels u, v in [1, 3]: samples 1.5 and 2.5 inside; split along a diagonal
    q = np.array([[0.02, 0.02, 2], [0.06, 0.02, 2], [0.06, 0.06, 2], [0.02, 0.06, 2]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    img = twin.render_depth(q, f, P, K, (5, 4), near=1.0, far=10.0)
    want = np.zeros((4, 5), np.float32)
    want[1:3, 1:3] = 2.0
    np.testing.assert_array_equal(img, want)
    one = twin.render_depth(q, f[:1], P, K, (5, 4), near=1.0, far=10.0) > 0
    two = twin.render_depth(q, f[1:], P, K, (5, 4), near=1.0, far=10.0) > 0
    assert not (one & two).any() and (one | two).sum() == 4              # every sample of the diagonal has one owner
    np.testing.assert_array_equal(twin.render_depth(q, f[:, ::-1], P, K, (5, 4), near=1.0, far=10.0), want)   # no culling
    # a square whose edges pass exactly through the samples (u, v in [1.5, 3.5]): left / top edges own, right / bottom do not
    q2 = np.array([[0.03, 0.03, 2], [0.07, 0.03, 2], [0.07, 0.07, 2], [0.03, 0.07, 2]], np.float32)
    img2 = twin.render_depth(q2, f, P, K, (5, 4), near=1.0, far=10.0)
    assert (img2 > 0).sum() == 4
    # outside [near, far], a bad face row, a non-finite pose
    assert not twin.render_depth(q, f, P, K, (5, 4), near=2.5, far=10.0).any()
    assert not twin.render_depth(q, f, P, K, (5, 4), near=0.5, far=1.5).any()
    bad = np.array([[0, 1, 2], [0, 2, 4], [-1, 2, 3]], np.int32)
    np.testing.assert_array_equal(twin.render_depth(q, bad, P, K, (5, 4), near=1.0, far=10.0) > 0, one)
    Pn = P.copy()
    Pn[1, 2] = np.nan
    assert not twin.render_depth(q, f, Pn, K, (5, 4), near=1.0, far=10.0).any()


# ------------------------------------------------------------------------------------- 2. the twin's VSD against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_twin_vsd_reproduces_the_reference_fixture(name):
    """Masks bit for bit, counts equal, 'step' e bit for bit, 'tlinear' e within vsd_twin.tlinear_bound (derived in the
    twin's docstring from the two summation orders; nothing in it is measured)."""
    c = load(name)
    r = twin.regenerate(name, c)
    n, p = c["pose_est"].shape[:2]
    g = c["pose_gt"].shape[1]
    delta, tau = float(c["delta"]), float(c["tau"])
    for i in range(n):
        depth = twin.sensor_depth(r["raw"][i], float(c["depth_scale"]))
        for a in range(p):
            for b in range(g):
                step = twin.vsd_pair(r["est"][i, a], r["gt"][i, b], depth, c["K"], delta, tau, "step")
                np.testing.assert_array_equal(np.packbits(step["visib_gt"]), c["visib_gt_bits"][i, b])
                np.testing.assert_array_equal(np.packbits(step["visib_est"]), c["visib_est_bits"][i, a, b])
                assert [step["union"], step["inter"], step["cost"]] == c["counts"][i, a, b].tolist()
                assert step["e"] == c["e_step"][i, a, b], (name, i, a, b)
                tl = twin.vsd_pair(r["est"][i, a], r["gt"][i, b], depth, c["K"], delta, tau, "tlinear")
                want = float(c["e_tlinear"][i, a, b])
                bound = twin.tlinear_bound(want, tl["m"], float(c["cost_sum"][i, a, b]), tl["union"])
                print("%s[%d,%d,%d] tlinear got %.17g want %.17g |diff| %.3g bound %.3g" %
                      (name, i, a, b, tl["e"], want, abs(tl["e"] - want), bound))
                assert abs(tl["e"] - want) <= bound


def test_fixtures_hold_the_cases_the_checks_need():
    big, half, close = load("vsd_720"), load("vsd_360"), load("vsd_near")
    assert tuple(big["size"]) == (720, 540) and big["e_step"].shape == (1, 2, 2)
    assert big["e_step"][0, 0, 0] < 0.3 and big["e_step"][0, 1, 1] > 0.9                       # a hit, and a prediction far off
    assert half["e_step"].shape == (2, 2, 2) and half["counts"][1, 1, 1, 0] == 0 and half["e_step"][1, 1, 1] == 1.0
    assert close["counts"][0, 0, 0, 0] > 0
    for name, c in (("vsd_720", big), ("vsd_360", half), ("vsd_near", close)):
        for k in ("e_step", "e_tlinear"):
            assert (np.abs(c[k] - 0.3) > 1e-6 * 0.3).all()
        raw = twin.regenerate(name, c)["raw"]
        assert raw.dtype == np.uint16 and (raw == 0).any() and (raw > 0).any()
    assert twin.any_pair_hit(big["e_step"][0]) and not twin.any_pair_hit(big["e_step"][0, 1:])
    assert not twin.any_pair_hit(big["e_step"][0], gt_valid=[False, True])


@pytest.mark.skipif(not os.path.exists("/root/reference/lib/utils/vsd/vsd_utils.py"),
                    reason="the reference tree exists only in the build container")
def test_vsd_fixtures_are_reproducible_from_the_reference():
    """tests/golden/make_vsd_golden.py, run here against the reference where it lies, regenerates every committed fixture
    with identical content (it never rewrites an existing file without --force)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_vsd_golden.py")], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if " exists," in l]
    assert sorted(l.split()[0] for l in lines) == sorted(FIXTURES + (RULES,)), out.stdout
    assert all(l.endswith("identical content") for l in lines), out.stdout


# ------------------------------------------------------------------------------------- 3. constructed inputs: exact boundaries
def _render(m, faces=None):
    return twin.render_depth(m["pts"], m["faces"] if faces is None else faces, m["pose"], m["K"], m["size"], m["near"], m["far"])


@pytest.mark.parametrize("seed", range(6))
def test_twin_on_lattice_soups_against_the_ray_caster(seed):
    """Half-pixel lattice soups put edges exactly through sample centres.  Off the samples that lie on the boundary of some
    closed triangle the twin and the ray caster agree on coverage, and on depth within 2**-23 relative (float32 rounding).
    Conditions on the input, not tolerances: the boundary samples are at most 10 % of the covered ones (measured 2.8 % to
    6.1 % on seeds 0..5), at least 20, and the twin covers some of them and not others."""
    m = twin.lattice_soup(seed, (37, 29))
    got = _render(m)
    want, _ = twin.raycast_depth(m["pts"], m["faces"], m["pose"], m["K"], m["size"], m["near"], m["far"])
    cov_t, cov_r, bnd = got > 0, want > 0, m["boundary"]
    covered, on = int((cov_t | cov_r).sum()), int(((cov_t | cov_r) & bnd).sum())
    both = ~bnd & cov_t & cov_r
    rel = np.abs(got.astype(np.float64)[both] - want[both]) / want[both]
    diff_cov = int((cov_t != cov_r)[~bnd].sum())
    print("soup %d: covered %d, boundary %d (%.1f %%; %d covered by the twin, %d not), coverage differences %d, largest "
          "relative depth difference %.3g" % (seed, covered, on, 100.0 * on / covered, int((bnd & cov_t).sum()),
                                              int((bnd & ~cov_t).sum()), diff_cov, rel.max()))
    assert on <= 0.10 * covered and int(bnd.sum()) >= 20
    assert (bnd & cov_t).any() and (bnd & ~cov_t).any()
    assert diff_cov == 0
    assert rel.size and rel.max() <= 2.0 ** -23
    f = m["faces"]
    assert (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 0] == f[:, 2]).any()       # repeated indices occur


@pytest.mark.parametrize("seed", (1, 4))
def test_twin_partition_equals_its_closed_form(seed):
    """The union of a partition is its outer rectangle under the ownership rule, as bytes; and every sample inside it
    belongs to exactly one triangle, every sample outside to none.  The two seeds put each outer line once on sample
    centres and once on integers."""
    m = twin.partition_mesh(seed, (26, 19))
    want = m["closed_form"]
    np.testing.assert_array_equal(_render(m).view(np.uint32), want.view(np.uint32))
    owners = sum((_render(m, m["faces"][k:k + 1]) > 0).astype(np.int64) for k in range(len(m["faces"])))
    np.testing.assert_array_equal(owners, (want > 0).astype(np.int64))
    assert (want > 0).any() and (want == 0).any() and set(np.unique(want)) == {0.0, 4.0}


def test_partition_seeds_put_every_outer_line_on_both_kinds_of_coordinate():
    ends = [np.array([g[0] for g in twin.partition_mesh(s, (26, 19))["lines"]] + [g[-1] for g in twin.partition_mesh(s, (26, 19))["lines"]])
            for s in (1, 4)]
    on_centre = np.stack([e % 1.0 == 0.5 for e in ends])                 # [seed, (left, top, right, bottom)]
    assert on_centre.any(0).all() and (~on_centre).any(0).all()


def test_constructed_meshes_keep_their_promises():
    """The builders' promises, checked from the snapped coordinates: the sizes at which the sweep changes its path."""
    m = twin.size_class_mesh()
    boxes = twin.piece_boxes(m)
    named = {k: boxes[i] for k, i in m["named"].items()}
    assert m["size"] == (130, 70) and len(m["faces"]) > 256 and len(m["faces"]) % 256 != 0
    assert named["box32"][1] == [(32, 2)] and named["box33"][1][0][0] == 33                  # kSmall = 32: the last lane-swept size
    for name, (x, y) in (("box32", (17, 13)), ("box33", (40, 12))):                          # and the box's last sample is covered
        assert _render(m, m["faces"][m["named"][name]][None])[y, x] == 2.0 and _render(m)[y, x] == 2.0
    assert named["whole"][1] == [(130 * 70, 153)] and named["sliver"][1] == [(130 * 70, 153)]
    assert named["blocks65"][1][0][1] == 65                                                  # one block past a wave's 64
    assert named["limit"][1] and not named["beyond"][1] and not named["beyond_v"][1]
    E = twin.eye_space(m["pts"], m["pose"])
    U, V, ok = twin._snap(m["K"], E[:, 0], E[:, 1], E[:, 2])
    f = m["faces"]
    assert np.abs(U[f[m["named"]["limit"]]]).max() == 2 ** 28 and ok[f[m["named"]["limit"]]].all()
    assert not ok[f[m["named"]["beyond"]]].all() and not ok[f[m["named"]["beyond_v"]]].all()
    assert np.abs(U[f[m["named"]["whole"]]]).max() == 2 ** 27 and np.abs(V[f[m["named"]["whole"]]]).max() == 2 ** 27
    first = [b for _, bs in boxes[:256] for b in bs]
    assert sum(1 for s, _ in first if s <= 32) >= 64 and sum(1 for s, _ in first if s > 32) >= 64
    img = _render(m)
    assert (img > 0).all()                                               # the whole-image triangle lies behind everything
    # blocks of a wave-swept piece in which an owning edge function is largest, and exactly 0, at a covered corner sample
    # that nothing hides: rejecting a block at `largest <= 0` instead of `< 0` loses these samples
    kinds = set()
    for name in ("corner_col", "corner_row", "corner_slant"):
        k = m["named"][name]
        assert named[name][1][0][0] > 32                                 # swept by the wave, block by block
        corners = twin.block_corner_samples(m, k)
        assert len(corners) >= 2
        alone, without = _render(m, m["faces"][k][None]), _render(m, np.delete(m["faces"], k, 0))
        for x, y in corners:
            assert alone[y, x] == 2.0 and img[y, x] == 2.0 and without[y, x] != 2.0                  # covered and frontmost
            kinds.add((x % 8 == 0, y % 8 == 7))
    assert {(True, False), (False, True), (True, True)} <= kinds        # a first column, a last row, a block's corner
    assert not twin.block_corner_samples(m, m["named"]["blocks65"]) and not twin.block_corner_samples(m, m["named"]["whole"])
    alone = _render(m, m["faces"][m["named"]["whole"]][None])
    assert (alone > 0).all() and (alone >= img).all() and (alone == img).sum() > 1000 and (alone > img).sum() > 1000
    # near clipping
    c = twin.clip_mesh()
    cb = twin.piece_boxes(c)
    inside = [k for k, _ in cb]
    assert {0, 1, 2, 3} <= set(inside)
    assert any(len(b) == 2 for _, b in cb)
    for w in range(0, len(cb), 64):                                      # a wave with a second piece in some lanes only
        second = [len(b) == 2 for _, b in cb[w:w + 64]]
        assert any(second) and not all(second)
    assert (twin.eye_space(c["pts"], c["pose"])[:, 2] == c["near"]).any()
    kept, dropped = c["far_quads"]
    assert (_render(c, c["faces"][kept:kept + 2]) == np.float32(c["far"])).sum() >= 50
    assert not _render(c, c["faces"][dropped:dropped + 2]).any() and cb[dropped][1]          # swept, every sample beyond far
    assert c["pts"][c["faces"][dropped], 2].min() == np.nextafter(np.float32(c["far"]), np.float32(np.inf))
    edges = {}
    for k, (n_in, _) in enumerate(cb):                                   # clipped edges (one end inside) shared by two faces
        r = c["faces"][k]
        if len(set(r.tolist())) == 3 and n_in in (1, 2):
            for a, b in ((r[0], r[1]), (r[1], r[2]), (r[2], r[0])):
                Za, Zb = c["pts"][a, 2], c["pts"][b, 2]
                if (Za >= c["near"]) != (Zb >= c["near"]):
                    edges.setdefault((min(a, b), max(a, b)), []).append(k)
    assert sum(1 for v in edges.values() if len(v) >= 2) >= 9            # the nine spokes of the two fans
    # the scalar tail of the resolve pass: P*H*W % 4 takes every value over the sizes the device tests use
    sizes = [(1,) + s for s in SOUP_SIZES] + [(1, 26, 19), (1,) + c["size"], (1,) + m["size"], (3, 37, 29)]
    assert {P * W * H % 4 for P, W, H in sizes} == {0, 1, 2, 3}


def test_twin_vsd_reproduces_the_rules_fixture():
    """The stored constructed images through twin.vsd_pair: masks and counts equal to the reference's, 'step' e bit for
    bit, 'tlinear' e within tlinear_bound; the stored images are what the builder builds; and the table's leading pixels
    give exactly the masks written out by hand in vsd_twin.RULES_TABLE."""
    c = load(RULES)
    built = twin.rules_images()
    assert sorted(c["cases"].tolist()) == sorted(built) == ["f32", "f64", "small", "zero"]
    K, delta, tau = c["K"], float(c["delta"]), float(c["tau"])
    assert (delta, tau) == (twin.RULES_DELTA, twin.RULES_TAU) == (15.0, 20.0)
    for name in built:
        depth, gt, est = c[name + "_test"], c[name + "_gt"], c[name + "_est"]
        for got, want in zip((depth, gt, est), built[name]):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(twin.dist_image(depth, K), depth)          # the camera makes distance equal depth
        for a in range(len(est)):
            for b in range(len(gt)):
                step = twin.vsd_pair(est[a], gt[b], depth, K, delta, tau, "step")
                np.testing.assert_array_equal(np.packbits(step["visib_gt"]), c[name + "_visib_gt_bits"][b])
                np.testing.assert_array_equal(np.packbits(step["visib_est"]), c[name + "_visib_est_bits"][a, b])
                assert [step["union"], step["inter"], step["cost"]] == c[name + "_counts"][a, b].tolist()
                assert step["e"] == c[name + "_e_step"][a, b], (name, a, b)
                tl = twin.vsd_pair(est[a], gt[b], depth, K, delta, tau, "tlinear")
                want = float(c[name + "_e_tlinear"][a, b])
                bound = twin.tlinear_bound(want, tl["m"], float(c[name + "_cost_sum"][a, b]), tl["union"])
                print("%s[%d,%d] counts %s step %.17g tlinear got %.17g want %.17g |diff| %.3g bound %.3g" %
                      (name, a, b, c[name + "_counts"][a, b].tolist(), step["e"], tl["e"], want, abs(tl["e"] - want), bound))
                assert abs(tl["e"] - want) <= bound
    assert c["zero_counts"].tolist() == [[[0, 0, 0]]] and c["zero_e_step"][0, 0] == 1.0 == c["zero_e_tlinear"][0, 0]
    # the table, by hand
    for name, rows in (("f64", list(range(len(twin.RULES_TABLE)))),
                       ("f32", [k for k in range(len(twin.RULES_TABLE)) if k not in twin.RULES_F64_ROWS])):
        n = len(rows)
        table = [twin.RULES_TABLE[k] for k in rows]
        assert c[name + "_test"].ravel()[:n].tolist() == [float(t[0]) for t in table]
        assert c[name + "_gt"][0].ravel()[:n].tolist() == [float(t[1]) for t in table]
        assert c[name + "_est"][0].ravel()[:n].tolist() == [float(t[2]) for t in table]
        vg = np.unpackbits(c[name + "_visib_gt_bits"][0])[:n].tolist()
        ve = np.unpackbits(c[name + "_visib_est_bits"][0, 0])[:n].tolist()
        assert vg == [t[3] for t in table] and ve == [t[4] for t in table], (name, vg, ve)
    assert [t[3] for t in twin.RULES_TABLE] == [1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0]
    assert [t[4] for t in twin.RULES_TABLE] == [1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1]
    # what the rows are there for: binary64 visibility would lose the row 2**-30 below, and the three rows around tau cost
    # 1, 0, 1 under 'step'
    t, g, e = (np.array([r[k] for r in twin.RULES_TABLE], np.float64) for k in range(3))
    assert not (g[3] - t[3] <= delta) and np.float32(g[3]) - np.float32(t[3]) <= np.float32(delta)
    assert (np.abs(g[12:15] - e[12:15]) >= tau).tolist() == [True, False, True]
    raw = twin.rules_uint16(c["f32_test"])
    assert raw.dtype == np.uint16 and np.array_equal(twin.sensor_depth(raw, 0.125), c["f32_test"])
    assert c["f64_test"].size == 300 and c["small_test"].size == 37      # two tiles with a partial second; one partial tile


# ------------------------------------------------------------------------------------------- 4. the library and its arguments
def test_vsd_library_exports_what_the_header_declares():
    names = capi.declared("vsd")
    assert names == {"pvs_render_workspace_bytes", "pvs_render_depth_batched", "pvs_vsd_workspace_bytes", "pvs_vsd_batched"}
    L = capi.load("vsd")
    for n in names:
        assert hasattr(L, n)
    exported = capi.exported("vsd")                              # and nothing else is exported
    assert {e for e in exported if not e.startswith("_")} == names, exported


def test_workspace_sizes_and_argument_errors():
    """Bad arguments are refused before anything is launched (no GPU is needed to be told so)."""
    L = capi.load("vsd")
    assert L.pvs_render_workspace_bytes(0, 100) == 0 and L.pvs_render_workspace_bytes(3, 0) == 0
    assert L.pvs_render_workspace_bytes(3, 100) == 3 * 100 * 32          # three binary64 and two int32 per (pose, vertex)
    assert L.pvs_vsd_workspace_bytes(2, 2, 2, 540, 720, 0) == 0          # 'step': integers only
    assert L.pvs_vsd_workspace_bytes(2, 2, 2, 540, 720, 1) == 8 * 8 * -(-540 * 720 // 256)
    assert L.pvs_vsd_workspace_bytes(0, 2, 2, 540, 720, 1) == 0
    render = L.pvs_render_depth_batched
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 100.0, 1e4, None) == 0      # no pose: nothing to do
    assert render(None, None, None, None, None, None, 2, 5, 4, 0, 64, 48, 100.0, 1e4, None) == -1     # null pointers
    assert render(None, None, None, None, None, None, -1, 5, 4, 0, 64, 48, 100.0, 1e4, None) == -1
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 0, 48, 100.0, 1e4, None) == -1      # empty image
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 16385, 100.0, 1e4, None) == -1  # beyond PVS_MAX_SIDE
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 0.0, 1e4, None) == -1       # near must be positive
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, 100.0, 50.0, None) == -1    # far < near
    assert render(None, None, None, None, None, None, 0, 5, 4, 0, 64, 48, float("nan"), 1e4, None) == -1
    vsd = L.pvs_vsd_batched
    args = lambda n, kind=0, cost=0, H=48, W=64: (None, None, None, kind, 0.1, None, 0, 15.0, 20.0, cost, None, None, None,   # noqa: E731
                                                  n, 2, 2, H, W, None)
    assert vsd(*args(0)) == 0
    assert vsd(*args(1)) == -1                                           # null pointers
    assert vsd(*args(0, kind=3)) == -1 and vsd(*args(0, cost=2)) == -1 and vsd(*args(0, H=0)) == -1
    assert vsd(*args(20000)) == -1                                       # more pairs than a grid dimension holds


def test_no_cpu_fallback(pkg):
    import torch
    from clean_pvnet_amd import vsd
    pts, faces = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)
    P, K = torch.eye(3, 4, dtype=torch.float64)[None], torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.render_depth(pts, faces, P, K, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.vsd(P[None], P[None], torch.zeros(1, 8, 8, dtype=torch.uint16), K, pts, faces)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.vsd_from_depth(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint16), K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vsd.VsdEvaluator(np.zeros((5, 3), np.float32), np.zeros((2, 3), np.int32), (8, 8), device="cpu")
