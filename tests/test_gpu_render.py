"""Colour renders on the MI355X (clean_pvnet_amd.render) against the numpy twin (tests/render_twin.py, itself pinned in
tests/test_render.py): img, label, depth, face and area as bytes; the near clip; the ties of coincident triangles; reruns and
batch independence; with one instance the depth bits of the depth rasteriser (clean_pvnet_amd.vsd.render_depth), which is what
holds the two rasterisers (one coverage code, two sinks) together; and the hand-off of the outputs to the augmentation modules.

The shapes are the smallest at which these kernels can go wrong: 70 x 45 (neither side a multiple of 8 or 4, 2 x 3150 pixels = 1575
groups of four over two blocks of the shading pass with a block that spans both images), a mesh of 194 faces and one of 300 (two
face tiles) with pieces swept by a lane and pieces swept by the wave, and 29 x 23 = 667 pixels, whose last group holds three."""
import functools

import numpy as np
import pytest

from tests import render_twin as twin
from tests import vsd_twin

pytestmark = pytest.mark.gpu
KEYS = ("img", "label", "depth", "face", "area")
SIZE = (70, 45)


def _t(gpu, a):
    import torch
    return torch.tensor(np.asarray(a), device=gpu)


def _render(gpu, s, sel=slice(None), bg=None, **kw):
    """The device's outputs as numpy for the images ``sel`` of scene ``s``."""
    from clean_pvnet_amd import render
    K = s["K"] if s["K"].ndim == 2 else s["K"][sel]
    out = render.render_color(_t(gpu, s["pts"]), _t(gpu, s["colors"]), _t(gpu, s["faces"]), _t(gpu, s["pose"][sel]), _t(gpu, K), s["size"],
                              ranges=s["ranges"], obj=None if s["obj"] is None else _t(gpu, s["obj"][sel]),
                              bg=None if bg is None else _t(gpu, bg[sel]), near=s["near"], far=s["far"], ambient=s["ambient"],
                              return_face=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _want(s, bg=None, **kw):
    return twin.render_batch(s["pts"], s["colors"], s["faces"], s["pose"], s["K"], s["size"], s["ranges"], s["obj"], bg, near=s["near"],
                             far=s["far"], ambient=s["ambient"], **kw)


def _assert_same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        diff = np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)
        print("%s: %s: %d of %d bytes differ" % (what, k, diff.sum(), diff.size))
    assert all(got[k].tobytes() == want[k].tobytes() for k in KEYS), what


@functools.lru_cache(maxsize=None)
def _scene():
    """B = 2, M = 3 on 70 x 45: image 0 holds the torus twice around an empty slot (obj = -1) under a camera with skew, image 1
    the size-class mesh twice and a torus whose pose is not finite, under the lattice camera with skew."""
    torus, sc = vsd_twin.mesh(6, nu=12, nv=8), vsd_twin.size_class_mesh()
    pts, colors, faces, ranges = twin.concat([(torus[0], twin.vertex_colors(1, len(torus[0])), torus[1]),
                                              (sc["pts"], twin.vertex_colors(2, len(sc["pts"])), sc["faces"])])
    K0, K1 = vsd_twin.camera(0.1, skew=0.4), vsd_twin.LATTICE_K.copy()
    K0[0, 2], K0[1, 2], K1[0, 1] = 35.0, 22.0, 0.5
    bad = vsd_twin.pose([0.2, 0.1, 0.0], [0.0, 0.0, 400.0])
    bad[1, 2] = np.nan
    shifted = vsd_twin.pose([0.0, 0.0, 0.05], [0.06, -0.03, 0.5])
    pose = np.stack([np.stack([vsd_twin.pose([0.4, 0.3, 0.1], [-12.0, 4.0, 400.0]), vsd_twin.pose([0.1, 0.2, 0.3], [0.0, 0.0, 300.0]),
                               vsd_twin.pose([-0.7, 0.2, 0.6], [14.0, -3.0, 440.0])]),
                     np.stack([sc["pose"], shifted, bad])])
    obj = np.array([[0, -1, 0], [1, 1, 0]], np.int32)
    s = {"pts": pts, "colors": colors, "faces": faces, "ranges": ranges, "pose": pose, "obj": obj, "K": np.stack([K0, K1]), "size": SIZE,
         "near": 1.0, "far": 10000.0, "ambient": 0.4}
    rng = np.random.RandomState(12)
    s["bg"] = rng.randint(0, 256, (2, SIZE[1], SIZE[0], 3)).astype(np.uint8)
    s["want"], s["want_bg"] = _want(s, bg_color=(7, 130, 255)), _want(s, s["bg"])
    return s


# ------------------------------------------------------------------------------------------------------------ 1. against the twin
def test_the_scene_holds_what_it_is_for():
    s = _scene()
    w = s["want"]
    assert SIZE[0] % 4 and SIZE[1] % 4 and (SIZE[0] * SIZE[1] * 2) % 4 == 0 and (SIZE[0] * SIZE[1]) % 1024
    assert w["area"][0, 1] == 0 and w["area"][1, 2] == 0 and (w["area"][0, [0, 2]] > 100).all() and (w["area"][1, :2] > 100).all()
    assert set(np.unique(w["label"][0])) == {0, 1, 3} and set(np.unique(w["label"][1])) == {1, 2}
    sc = vsd_twin.size_class_mesh()
    boxes = [n for _inside, bs in vsd_twin.piece_boxes({**sc, "K": s["K"][1], "size": SIZE, "near": s["near"]}) for n, _blocks in bs]
    assert min(boxes) <= 32 < max(boxes)                                           # pieces for a lane and pieces for the wave
    assert w["face"].max() >= 256                                                  # an owner from the second tile of faces
    assert (w["img"][w["label"] == 0] == [7, 130, 255]).all() and np.array_equal(s["want_bg"]["img"][w["label"] == 0], s["bg"][w["label"] == 0])


def test_two_meshes_equal_the_twin_without_a_background(pkg, gpu):
    s = _scene()
    _assert_same(_render(gpu, s, bg_color=(7, 130, 255)), s["want"], "scene")


def test_two_meshes_equal_the_twin_over_a_background(pkg, gpu):
    s = _scene()
    _assert_same(_render(gpu, s, bg=s["bg"]), s["want_bg"], "scene over bg")
    odd = np.concatenate([np.zeros(3, np.uint8), s["bg"].ravel()])                 # a background that is not 4-byte aligned
    import torch
    from clean_pvnet_amd import render
    bg = torch.tensor(odd, device=gpu)[3:].view(2, SIZE[1], SIZE[0], 3)
    got = render.render_color(_t(gpu, s["pts"]), _t(gpu, s["colors"]), _t(gpu, s["faces"]), _t(gpu, s["pose"]), _t(gpu, s["K"]), SIZE,
                              ranges=s["ranges"], obj=_t(gpu, s["obj"]), bg=bg, near=s["near"], far=s["far"], ambient=s["ambient"])
    assert "face" not in got and got["img"].cpu().numpy().tobytes() == s["want_bg"]["img"].tobytes()


def test_the_size_classes_equal_the_twin_on_their_own_camera(pkg, gpu):
    """130 x 70 under the lattice camera: a piece of exactly 32 samples (the lane's largest) and one of 33 (the wave's smallest)."""
    m = vsd_twin.size_class_mesh()
    boxes = [n for _inside, bs in vsd_twin.piece_boxes(m) for n, _blocks in bs]
    assert 32 in boxes and 33 in boxes
    s = {"pts": m["pts"], "colors": twin.vertex_colors(2, len(m["pts"])), "faces": m["faces"], "ranges": None, "pose": m["pose"][None, None],
         "obj": None, "K": m["K"], "size": m["size"], "near": m["near"], "far": m["far"], "ambient": 0.3}
    _assert_same(_render(gpu, s), _want(s), "size classes")


# ------------------------------------------------------------------------------------------------------------ 2. the near clip
@functools.lru_cache(maxsize=None)
def _clip_scene():
    m = vsd_twin.clip_mesh()
    pose = np.stack([m["pose"], vsd_twin.pose([0.05, -0.08, 0.02], [0.03, 0.02, 0.4])])[:, None]
    return {"pts": m["pts"], "colors": twin.vertex_colors(4, len(m["pts"])), "faces": m["faces"], "ranges": None, "pose": pose, "obj": None,
            "K": m["K"], "size": m["size"], "near": m["near"], "far": m["far"], "ambient": 0.5}


def test_the_near_clip_equals_the_twin(pkg, gpu):
    s = _clip_scene()
    want = _want(s)
    assert (want["area"] > 50).all() and (s["size"][0] * s["size"][1] * 2) % 4 == 2   # the last group of the batch holds two pixels
    _assert_same(_render(gpu, s), want, "clip")
    one = {**s, "pose": s["pose"][:1]}
    assert (s["size"][0] * s["size"][1]) % 4 == 3
    _assert_same(_render(gpu, one), _want(one), "clip, one image")


# ------------------------------------------------------------------------------------------------------------ 3. ties
def test_coincident_triangles_go_to_the_lower_face_and_the_lower_instance(pkg, gpu):
    tri = vsd_twin.lattice_points([4.5, 22.5, 10.5], [3.5, 6.5, 21.5], [4.0, 4.0, 4.0])
    red, blue = np.array([[250, 0, 0]] * 3, np.uint8), np.array([[0, 0, 250]] * 3, np.uint8)
    base = {"K": vsd_twin.LATTICE_K, "size": (30, 24), "near": 1.0, "far": 16.0, "ambient": 1.0}
    faces2 = {**base, "pts": np.concatenate([tri, tri]), "colors": np.concatenate([red, blue]), "faces": np.array([[0, 1, 2], [3, 4, 5]], np.int32),
              "ranges": None, "obj": None, "pose": vsd_twin.IDENTITY[None, None]}
    want = _want(faces2)
    cov = want["label"] > 0
    assert cov.sum() > 50 and (want["face"][cov] == 0).all() and (want["img"][cov] == [250, 0, 0]).all()
    _assert_same(_render(gpu, faces2), want, "two faces")
    p, c, f, ranges = twin.concat([(tri, red, np.array([[0, 1, 2]])), (tri, blue, np.array([[0, 1, 2]]))])
    for obj, colour in (([[0, 1]], [250, 0, 0]), ([[1, 0]], [0, 0, 250])):
        inst2 = {**base, "pts": p, "colors": c, "faces": f, "ranges": ranges, "obj": np.array(obj, np.int32),
                 "pose": np.stack([vsd_twin.IDENTITY, vsd_twin.IDENTITY])[None]}
        want = _want(inst2)
        assert (want["label"][cov] == 1).all() and (want["img"][cov] == colour).all() and want["area"].tolist() == [[int(cov.sum()), 0]]
        _assert_same(_render(gpu, inst2), want, "two instances %s" % (obj,))


# ------------------------------------------------------------------------------------------------------------ 4. reruns, batches
def test_reruns_and_single_images_give_the_same_bytes(pkg, gpu):
    s = _scene()
    first, again = _render(gpu, s, bg=s["bg"]), _render(gpu, s, bg=s["bg"])
    for k in KEYS:
        assert first[k].tobytes() == again[k].tobytes(), k
    for b in range(2):
        alone = _render(gpu, s, slice(b, b + 1), bg=s["bg"])
        for k in KEYS:
            assert alone[k].tobytes() == first[k][b:b + 1].tobytes(), (b, k)


# ------------------------------------------------------------------------------------------------------------ 5. the depth rasteriser
def _depth_cases():
    torus = vsd_twin.mesh(6, nu=12, nv=8)
    K = vsd_twin.camera(0.1, skew=0.4)
    poses = np.stack([vsd_twin.pose([0.4, 0.3, 0.1], [-12.0, 4.0, 400.0]), vsd_twin.pose([-0.7, 0.2, 0.6], [14.0, -3.0, 140.0])])
    yield "torus", torus[0], torus[1], poses, K, SIZE, 100.0, 10000.0              # the second pose crosses the near plane
    for name, m in (("size_class", vsd_twin.size_class_mesh()), ("clip", vsd_twin.clip_mesh())):
        yield name, m["pts"], m["faces"], m["pose"][None], m["K"], m["size"], m["near"], m["far"]


@pytest.mark.parametrize("case", list(_depth_cases()), ids=lambda c: c[0])
def test_one_instance_has_the_depth_bits_of_the_depth_rasteriser(pkg, gpu, case):
    from clean_pvnet_amd import render, vsd
    name, pts, faces, poses, K, size, near, far = case
    P, F, T, Kt = _t(gpu, pts), _t(gpu, faces), _t(gpu, poses), _t(gpu, K)
    want = vsd.render_depth(P, F, T, Kt, size, near, far)
    got = render.render_color(P, _t(gpu, twin.vertex_colors(5, len(pts))), F, T, Kt, size, near=near, far=far)
    assert bool((want > 0).any()) and got["depth"].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert bool(((got["label"] > 0) == (want > 0)).all())
    assert got["area"].cpu().numpy().ravel().tolist() == (want > 0).flatten(1).sum(1).cpu().numpy().tolist()


# ------------------------------------------------------------------------------------------------------------ 6. the hand-off
def test_outputs_feed_the_augmentation_modules_as_they_are(pkg, gpu):
    import torch
    from clean_pvnet_amd import augment, ct_augment, render
    s = _scene()
    r = render.SceneRenderer([(s["pts"][:s["ranges"][0, 1]], s["colors"][:s["ranges"][0, 1]], s["faces"][:s["ranges"][0, 3]]),
                              (s["pts"][s["ranges"][1, 0]:], s["colors"][s["ranges"][1, 0]:], s["faces"][s["ranges"][1, 2]:])],
                             SIZE, device=gpu, near=s["near"], far=s["far"], ambient=s["ambient"], return_face=True)
    assert np.array_equal(r.ranges, s["ranges"])
    out = r(_t(gpu, s["pose"]), obj=_t(gpu, s["obj"]), K=_t(gpu, s["K"]), bg=_t(gpu, s["bg"]))
    _assert_same({k: v.cpu().numpy() for k, v in out.items()}, s["want_bg"], "SceneRenderer")
    assert out["img"].dtype == torch.uint8 and out["label"].dtype == torch.uint8 and out["img"].is_contiguous() and out["label"].is_contiguous()
    a = ct_augment.ct_augment(out["img"], out["label"], None, train=False, n_instances=3)
    assert tuple(a["inp"].shape) == (2, 3, 64, 96) and tuple(a["orig_img"].shape) == (2, 64, 96, 3) and tuple(a["boxes"].shape) == (2, 3, 4)
    boxes = a["boxes"].cpu().numpy()
    assert (boxes[0, 1] == 0).all() and (boxes[1, 2] == 0).all() and (boxes[0, 0, 2:] > boxes[0, 0, :2]).all()   # the empty slots have no box
    kpt = torch.tensor([[[20.0, 15.0], [40.5, 30.25]]] * 2, device=gpu)
    p = augment.pvnet_augment(out["img"], out["label"], kpt, (32, 40), augment.draws(2, generator=torch.Generator().manual_seed(3)))
    assert tuple(p["img"].shape) == (2, 32, 40, 3) and tuple(p["mask"].shape) == (2, 32, 40) and tuple(p["kpt_2d"].shape) == (2, 2, 2)
    assert p["img"].dtype == torch.uint8 and p["mask"].dtype == torch.uint8
