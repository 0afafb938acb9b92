"""Colour renders (clean_pvnet_amd.render, include/pvnet_vote.h, "Colour renders") without a GPU: the module, the header, the
symbols and the host-side refusals are there; the numpy twin of the contract (tests/render_twin.py) gives, for a single object, the
depth of the depth rasteriser's twin (tests/vsd_twin.py) as bytes; it agrees with an independent ray caster on owner, label and
colour wherever the two can be compared; closed forms of the shading hold; the ownership rule decides ties by instance and face.
The GPU tests (tests/test_gpu_render.py) then hold the device to the twin byte for byte."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import capi
from tests import render_twin as twin
from tests import vsd_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
SYMBOLS = {"pvv_render_workspace_bytes", "pvv_render_color"}
TITLE = "Colour renders"


# ------------------------------------------------------------------------------------------------ 1. the module and the library
def test_module_imports(pkg):
    from clean_pvnet_amd import render
    assert callable(render.render_color) and callable(render.SceneRenderer)
    assert (render.MAX_M, render.MAX_FACES, render.MAX_SIDE) == (255, 1 << 24, 16384) == (twin.MAX_M, twin.MAX_FACES, 16384)
    r, nmax, fmax = render.check_ranges(None, 10, 7)
    assert r.tolist() == [[0, 10, 0, 7]] and (nmax, fmax) == (10, 7)
    with pytest.raises(ValueError):
        render.check_ranges([[0, 11, 0, 7]], 10, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        import torch
        render.render_color(torch.zeros(3, 3), torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int32),
                            torch.zeros(1, 3, 4), torch.eye(3), (8, 8))


def test_header_declares_and_library_exports_the_entry_points():
    raw = open(HEADER).read()
    assert SYMBOLS <= capi.declared()
    assert SYMBOLS <= capi.exported()
    assert "#define PVV_ABI_VERSION 8" in raw                                      # additive: the version did not move
    # the newest section: behind every section but the two whose place at the end other tests pin
    assert raw.index("Detector augmentation") < raw.index(TITLE) < raw.index("Detector training")
    section = raw[raw.index(TITLE):raw.index("Detector training")]
    assert SYMBOLS <= set(re.findall(r"\b(pvv_[a-z0-9_]+)\s*\(", section))
    for cite in ("lib/utils/linemod/opengl_renderer.py:171-179", "lib/datasets/tless/opengl_renderer.py:150-156",
                 "lib/utils/linemod/opengl_backend.py:21-67", ":243-247", "linemod_to_coco.py:184"):
        assert cite in section
    for name, value in (("MAX_M", "255"), ("MAX_FACES", "(1 << 24)"), ("MAX_SIDE", "16384")):
        assert "#define PVV_RENDER_%s %s" % (name, value) in raw
    import lib
    table = lib.load_build().HIP_LIBS
    assert len(table) == 7 and list(table)[-1] == "icp"


def test_workspace_sizes_are_the_stated_values():
    L = capi.load()
    assert L.pvv_abi_version() == 8
    up = lambda v: (v + 255) // 256 * 256                                          # noqa: E731
    assert L.pvv_render_workspace_bytes(2, 3, 301, 45, 70) == up(32 * 2 * 3 * 301) + up(8 * 2 * 45 * 70)
    assert L.pvv_render_workspace_bytes(32, 4, 5841, 480, 640) == up(32 * 32 * 4 * 5841) + 8 * 32 * 480 * 640
    assert L.pvv_render_workspace_bytes(1, 1, 1, 1, 1) == 512
    for args, word in (((1, 256, 10, 8, 8), b"M in [1, 255]"), ((1, 0, 10, 8, 8), b"M in [1, 255]"), ((0, 1, 10, 8, 8), b"B >= 1"),
                       ((300, 255, 10, 8, 8), b"65535"), ((1, 1, 10, 16385, 8), b"16384"), ((1, 1, 10, 8, 16385), b"16384"),
                       ((1, 1, 10, 0, 8), b"16384"), ((1, 1, 0, 8, 8), b"vertex count")):
        assert L.pvv_render_workspace_bytes(*args) == 0 and word in L.pvv_last_error(), args


def test_bad_arguments_return_minus_one_before_any_launch():
    L = capi.load()
    x = 256                                                                         # a pointer that is not NULL: never dereferenced
    bgc = (ctypes.c_uint8 * 3)(0, 0, 0)

    def call(**kw):
        a = dict(pts=x, colors=x, faces=x, N=100, F=50, ranges=x, O=1, Nmax=100, Fmax=50, pose=x, obj=None, K=x, K_batched=0, bg=None,
                 bgc=bgc, B=1, M=1, H=8, W=8, near=10.0, far=100.0, ambient=0.5, ws=x, ws_bytes=1 << 20, img=x, label=x, depth=x, area=x,
                 face=None, stream=None)
        a.update(kw)
        return L.pvv_render_color(*a.values())

    for kw, word in ((dict(M=256), b"M in [1, 255]"), (dict(F=(1 << 24) + 1, Fmax=(1 << 24) + 1), b"2^24"), (dict(W=16385), b"16384"),
                     (dict(H=16385), b"16384"), (dict(pts=None), b"NULL"), (dict(colors=None), b"NULL"), (dict(faces=None), b"NULL"),
                     (dict(ranges=None), b"NULL"), (dict(pose=None), b"NULL"), (dict(K=None), b"NULL"), (dict(ws=None), b"NULL"),
                     (dict(img=None), b"NULL"), (dict(label=None), b"NULL"), (dict(depth=None), b"NULL"), (dict(area=None), b"NULL"),
                     (dict(bgc=None), b"NULL"), (dict(near=0.0), b"near"), (dict(far=5.0), b"near"), (dict(ambient=float("nan")), b"ambient"),
                     (dict(Nmax=101), b"Nmax <= N"), (dict(O=0), b"one object"), (dict(depth=264), b"aligned"), (dict(ws=272), b"aligned")):
        assert call(**kw) == -1 and word in L.pvv_last_error(), (kw, L.pvv_last_error())
    assert call(ws_bytes=512) == -2 and b"workspace smaller" in L.pvv_last_error()


# ------------------------------------------------------------------------------------------------ 2. the depth rasteriser's twin
def _single_object_cases():
    pts, faces = vsd_twin.mesh(5, nu=24, nv=12)
    yield "mesh", pts, faces, vsd_twin.pose([0.7, -0.4, 0.3], [10.0, -5.0, 420.0]), vsd_twin.camera(0.125, skew=0.3), (90, 68), 100.0, 10000.0
    for name, m in (("clip", vsd_twin.clip_mesh()), ("size_class", vsd_twin.size_class_mesh()), ("partition", vsd_twin.partition_mesh(4, (37, 26)))):
        yield name, m["pts"], m["faces"], m["pose"], m["K"], m["size"], m["near"], m["far"]


@pytest.mark.parametrize("case", list(_single_object_cases()), ids=lambda c: c[0])
def test_single_object_depth_equals_the_depth_twin_as_bytes(case):
    name, pts, faces, P, K, size, near, far = case
    got = twin.render_color(pts, twin.vertex_colors(1, len(pts)), faces, P[None], K, size, near=near, far=far)
    want = vsd_twin.render_depth(pts, faces, P, K, size, near, far)
    assert want.any() and got["depth"].dtype == np.float32 and got["depth"].tobytes() == want.tobytes()
    assert np.array_equal(got["label"], (want > 0).astype(np.uint8)) and np.array_equal(got["face"] >= 0, want > 0)
    assert got["area"].tolist() == [int((want > 0).sum())]


# ------------------------------------------------------------------------------------------------ 3. the independent ray caster
def test_owner_label_and_colour_equal_the_ray_casters():
    pts, faces = vsd_twin.mesh(3, nu=24, nv=12)
    colors = twin.vertex_colors(8, len(pts))
    P, K, size, near, far, ambient = vsd_twin.pose([0.9, 0.5, -0.2], [4.0, -3.0, 400.0]), vsd_twin.camera(96 / 720.0), (96, 72), 100.0, 10000.0, 0.35
    got = twin.render_color(pts, colors, faces, P[None], K, size, near=near, far=far, ambient=ambient)
    rc = twin.raycast(pts, faces, P, K, size, near, far)
    want = twin.shade_reference(rc, faces, colors, K, ambient)
    covered = (got["label"] > 0) | (rc["face"] >= 0)
    distinct = rc["depth"].astype(np.float32) != rc["second"].astype(np.float32)
    compared = covered & ~rc["band"] & distinct
    frac = np.floor(want) + 0.5
    excepted = compared[..., None] & (np.abs(want - frac) <= 1e-6)
    print("covered %d, compared %d (%.1f %%), excepted channels %d" % (covered.sum(), compared.sum(), 100.0 * compared.sum() / covered.sum(),
                                                                       excepted.sum()))
    assert compared.sum() >= 0.9 * covered.sum() and covered.sum() > 800
    assert np.array_equal(got["face"][compared], rc["face"][compared]) and (got["label"][compared] == 1).all()
    assert (got["label"][~covered] == 0).all()
    rel = np.abs(got["depth"][compared].astype(np.float64) - rc["depth"][compared]) / rc["depth"][compared]
    assert rel.max() <= 2.0 ** -23
    rounded = np.floor(np.clip(want, 0, 255) + 0.5)
    diff = np.abs(got["img"].astype(np.float64) - rounded)
    plain = compared[..., None] & ~excepted
    assert (diff[np.broadcast_to(plain, diff.shape)] == 0).all() and (diff[excepted] <= 1).all()
    assert len(np.unique(got["img"][compared])) > 100                             # a shaded, coloured image, not a constant


# ------------------------------------------------------------------------------------------------ 4. closed forms
def _triangle(colors, Z=4.0, f=128.0, cx=0.0, cy=0.0):
    """A fronto-parallel triangle at depth Z that projects to (4.5, 3.5), (22.5, 6.5), (10.5, 21.5) under the focal length f and
    the principal point (cx, cy): its centroid is the sample of pixel (12, 10).  Every coordinate is exact in float32."""
    u, v = np.array([4.5, 22.5, 10.5]), np.array([3.5, 6.5, 21.5])
    p = np.stack([(u - cx) * Z / f, (v - cy) * Z / f, np.full(3, Z)], 1)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32), np.asarray(colors, np.uint8), np.array([[0, 1, 2]], np.int32)


def test_a_fronto_parallel_triangle_at_the_principal_point_has_the_vertex_colour():
    pts, colors, faces = _triangle([[200, 100, 30]] * 3, f=16.0, cx=12.5, cy=10.5)
    K = np.array([[16.0, 0.0, 12.5], [0.0, 16.0, 10.5], [0.0, 0.0, 1.0]])         # the principal point is the sample of pixel (12, 10)
    out = twin.render_color(pts, colors, faces, vsd_twin.IDENTITY[None], K, (30, 24), near=1.0, far=16.0, ambient=0.5)
    assert out["label"][10, 12] == 1 and out["img"][10, 12].tolist() == [200, 100, 30]   # diffuse = 1
    out0 = twin.render_color(pts, colors, faces, vsd_twin.IDENTITY[None], K, (30, 24), near=1.0, far=16.0, ambient=0.0)
    assert out0["img"][10, 12].tolist() == [200, 100, 30]
    y, x = 12, 15                                                                   # off axis: the light falls at an angle
    assert out0["label"][y, x] == 1
    dx, dy = (x + 0.5 - 12.5) / 16.0, (y + 0.5 - 10.5) / 16.0
    cos = 1.0 / np.sqrt(dx * dx + dy * dy + 1.0)
    want = [np.floor(c * cos + 0.5) for c in (200, 100, 30)]
    assert all(abs(c * cos - np.floor(c * cos) - 0.5) > 1e-6 for c in (200, 100, 30)) and cos < 0.9995
    assert out0["img"][y, x].tolist() == want and want != [200, 100, 30]


def test_three_vertex_colours_meet_in_their_mean_at_the_centroid():
    cols = np.array([[255, 0, 10], [0, 240, 20], [30, 60, 210]], np.uint8)
    pts, colors, faces = _triangle(cols)
    for ambient in (0.0, 0.5):
        out = twin.render_color(pts, colors, faces, vsd_twin.IDENTITY[None], vsd_twin.LATTICE_K, (30, 24), near=1.0, far=16.0, ambient=ambient)
        assert out["label"][10, 12] == 1
        dx, dy = 12.5 / 128.0, 10.5 / 128.0
        light = min(ambient + 1.0 / np.sqrt(dx * dx + dy * dy + 1.0), 1.0)
        want = cols.astype(np.float64).mean(0) * light
        assert np.abs(out["img"][10, 12].astype(np.float64) - want).max() <= 1.0, (out["img"][10, 12], want)


# ------------------------------------------------------------------------------------------------ 5. ownership
def test_coincident_triangles_go_to_the_lower_face_and_the_lower_instance():
    pts, _c, _f = _triangle([[0, 0, 0]] * 3)
    red, blue = [[250, 0, 0]] * 3, [[0, 0, 250]] * 3
    kw = dict(near=1.0, far=16.0, ambient=1.0)
    # two faces of one object over the same three positions
    out = twin.render_color(np.concatenate([pts, pts]), np.array(red + blue, np.uint8), np.array([[0, 1, 2], [3, 4, 5]], np.int32),
                            vsd_twin.IDENTITY[None], vsd_twin.LATTICE_K, (30, 24), **kw)
    cov = out["label"] > 0
    assert cov.sum() > 50 and (out["face"][cov] == 0).all() and (out["img"][cov] == [250, 0, 0]).all()
    flipped = twin.render_color(np.concatenate([pts, pts]), np.array(blue + red, np.uint8), np.array([[0, 1, 2], [3, 4, 5]], np.int32),
                                vsd_twin.IDENTITY[None], vsd_twin.LATTICE_K, (30, 24), **kw)
    assert (flipped["img"][cov] == [0, 0, 250]).all() and np.array_equal(flipped["depth"], out["depth"])
    # two objects, one face each, at the same pose: instance 0 wins whichever object it is
    p2, c2, f2, ranges = twin.concat([(pts, np.array(red, np.uint8), np.array([[0, 1, 2]])), (pts, np.array(blue, np.uint8), np.array([[0, 1, 2]]))])
    poses = np.stack([vsd_twin.IDENTITY, vsd_twin.IDENTITY])
    for obj, colour in (([0, 1], [250, 0, 0]), ([1, 0], [0, 0, 250])):
        o = twin.render_color(p2, c2, f2, poses, vsd_twin.LATTICE_K, (30, 24), ranges=ranges, obj=obj, **kw)
        assert np.array_equal(o["label"] > 0, cov) and (o["label"][cov] == 1).all() and (o["img"][cov] == colour).all()
        assert o["area"].tolist() == [int(cov.sum()), 0]


def test_permuting_instances_changes_only_the_label_numbering():
    a, b = vsd_twin.mesh(1, nu=12, nv=8), vsd_twin.mesh(2, nu=12, nv=8)
    pts, colors, faces, ranges = twin.concat([(a[0], twin.vertex_colors(1, len(a[0])), a[1]), (b[0], twin.vertex_colors(2, len(b[0])), b[1])])
    K, size = vsd_twin.camera(0.1), (72, 54)
    poses = np.stack([vsd_twin.pose([0.3, 0.2, 0.1], [-15.0, 5.0, 420.0]), vsd_twin.pose([-0.8, 0.1, 0.5], [20.0, -4.0, 470.0]),
                      vsd_twin.pose([0.1, 1.1, -0.4], [5.0, 10.0, 380.0])])
    obj = np.array([0, 1, 1])
    kw = dict(ranges=ranges, near=100.0, far=10000.0)
    alone = [twin.render_color(pts, colors, faces, poses[m:m + 1], K, size, obj=obj[m:m + 1], **kw)["depth"] for m in range(3)]
    for i in range(3):
        for j in range(i + 1, 3):
            both = (alone[i] > 0) & (alone[j] > 0)
            assert both.any() and (alone[i][both] != alone[j][both]).all()          # they overlap and their depths never tie
    base = twin.render_color(pts, colors, faces, poses, K, size, obj=obj, **kw)
    assert set(np.unique(base["label"])) == {0, 1, 2, 3}
    perm = np.array([2, 0, 1])                                                      # new instance k is old instance perm[k]
    got = twin.render_color(pts, colors, faces, poses[perm], K, size, obj=obj[perm], **kw)
    for k in ("img", "depth", "face"):
        assert got[k].tobytes() == base[k].tobytes(), k
    renumber = np.zeros(4, np.uint8)
    renumber[perm + 1] = np.arange(1, 4)
    assert np.array_equal(got["label"], renumber[base["label"]]) and got["area"].tolist() == base["area"][perm].tolist()


def test_areas_sum_to_the_covered_count_on_the_partition():
    m = vsd_twin.partition_mesh(9, (41, 29))
    n = len(m["faces"]) // 2
    ranges = np.array([[0, len(m["pts"]), 0, n], [0, len(m["pts"]), n, len(m["faces"]) - n]], np.int32)      # the faces as two objects
    out = twin.render_color(m["pts"], twin.vertex_colors(3, len(m["pts"])), m["faces"], np.stack([m["pose"]] * 2), m["K"], m["size"],
                            ranges=ranges, obj=[0, 1], near=m["near"], far=m["far"])
    covered = int((m["closed_form"] > 0).sum())
    assert covered > 0 and np.array_equal(out["depth"], m["closed_form"])
    assert int(out["area"].sum()) == covered and (out["area"] > 0).all()
    assert np.array_equal(np.bincount(out["label"].ravel(), minlength=3)[1:], out["area"])
