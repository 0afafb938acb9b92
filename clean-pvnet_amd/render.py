"""Shaded colour images, instance labels and depth of a batch of scenes on the device (``libpvnet_vote.so``, the section "Colour
renders" of include/pvnet_vote.h).

The reference makes PVNet's synthetic training images off line, one pose at a time, through an OpenGL context:
``OpenGLRenderer.render(..., render_type='rgb')`` (lib/utils/linemod/opengl_renderer.py:171-179,
lib/datasets/tless/opengl_renderer.py:150-156) draws the PLY's vertex colours with the shaders of
lib/utils/linemod/opengl_backend.py:21-67 and reads the frame back (:243-247); its ``fuse`` step then pastes several such renders
over each other.  Here ``render_color`` rasterises every instance of every image of a batch in HIP with exact occlusion between
them, shades the pixel's owner and writes the tensors the rest of the package consumes: ``img`` [B,H,W,3] uint8 and ``label``
[B,H,W] uint8 go into ``ct_augment.ct_compose`` / ``ct_augment.ct_augment``, ``augment.pvnet_augment`` and
``train.pvnet_loss(kpt_2d=...)`` as they are.  ``area`` [B,M] counts the pixels each instance owns, so that the reference's
"drop masks under 400 pixels" (linemod_to_coco.py:184) needs no read-back per image.

The arithmetic contract is in the header and DESIGN.md section 20; tests/render_twin.py is the numpy twin the device equals byte
for byte.  CUDA tensors in and out, the current stream, a workspace from the caching allocator, nothing read back, no CPU
fallback.
"""
import ctypes

import numpy as np

from . import _native

_lib = _native.bind("render", "libpvnet_vote.so", last_error="pvv_last_error")

MAX_M, MAX_FACES, MAX_SIDE = 255, 1 << 24, 16384          # PVV_RENDER_MAX_M, PVV_RENDER_MAX_FACES, PVV_RENDER_MAX_SIDE


def check_ranges(ranges, N, F):
    """``ranges`` as a host int32 array [O,4] = (first vertex, vertex count, first face, face count), checked against a mesh of
    ``N`` vertices and ``F`` faces; None is one object covering everything.  Returns (ranges, Nmax, Fmax)."""
    r = np.array([[0, N, 0, F]], np.int32) if ranges is None else np.ascontiguousarray(np.asarray(ranges), dtype=np.int32)
    if r.ndim != 2 or r.shape[1] != 4 or r.shape[0] < 1:
        raise ValueError("clean_pvnet_amd.render: ranges must be a host int array [O >= 1, 4], got %s" % (r.shape,))
    r64 = r.astype(np.int64)
    if (r64 < 0).any() or (r64[:, 0] + r64[:, 1] > N).any() or (r64[:, 2] + r64[:, 3] > F).any() or (r64[:, 1] < 1).any():
        raise ValueError("clean_pvnet_amd.render: every row of ranges must lie inside the mesh (%d vertices, %d faces) and hold a vertex" % (N, F))
    Fmax = int(r64[:, 3].max())
    if Fmax > MAX_FACES:
        raise ValueError("clean_pvnet_amd.render: an object may have at most 2^24 faces, got %d" % Fmax)
    return r, int(r64[:, 1].max()), Fmax


def render_color(pts, colors, faces, pose, K, size, *, ranges=None, obj=None, bg=None, bg_color=(0, 0, 0), near=10., far=10000.,
                 ambient=0.5, return_face=False):
    """Colour images, instance labels and depth of ``B`` scenes of ``M`` instances each (replaces one
    ``OpenGLRenderer.render(..., 'rgb')`` per pose, opengl_renderer.py:171-179, and the pasting of ``fuse``).
    :param pts:      [N,3] CUDA tensor, the vertices of every object (taken as float32)
    :param colors:   [N,3] uint8 CUDA tensor, the vertex colours, in the channel order the caller wants out
    :param faces:    [F,3] CUDA tensor (taken as int32), indices local to their object as each PLY has them; a row with an index
                     outside [0, vertex count of the object) is skipped on the device
    :param pose:     [B,M,3,4] or [B,3,4] CUDA tensor [R | t] (taken as binary64), t in the units of ``pts``; an instance with a
                     non-finite entry draws nothing
    :param K:        [3,3] or [B,3,3] CUDA tensor
    :param size:     (W, H)
    :param ranges:   [O,4] host int32 (first vertex, vertex count, first face, face count) per object; None: one object
    :param obj:      [B,M] int32 CUDA tensor, the object of each instance; None: 0 everywhere; a value outside [0, O) is no
                     instance (checked on the device)
    :param bg:       [B,H,W,3] uint8 CUDA tensor behind the objects, or None for ``bg_color``
    :param ambient:  light = min(ambient + diffuse, 1)
    :return: dict: ``img`` [B,H,W,3] uint8, ``label`` [B,H,W] uint8 (0 background, m + 1 instance m), ``depth`` [B,H,W] float32
             (eye-space Z, 0 background), ``area`` [B,M] int32 and, with ``return_face``, ``face`` [B,H,W] int32 (the owner's
             face index inside its object, -1 background)."""
    import torch
    for t, what in ((pts, "pts"), (colors, "colors"), (faces, "faces"), (pose, "pose"), (K, "K")):
        _native.need_cuda(t, what, "render")
    W, H = int(size[0]), int(size[1])
    if not (0 < W <= MAX_SIDE and 0 < H <= MAX_SIDE):
        raise ValueError("clean_pvnet_amd.render: size = (W, H) must lie in [1, %d], got %r" % (MAX_SIDE, (W, H)))
    if not (float(near) > 0.0 and float(far) >= float(near) and float(ambient) >= 0.0):
        raise ValueError("clean_pvnet_amd.render: 0 < near <= far and ambient >= 0 are required, got near=%r far=%r ambient=%r" % (near, far, ambient))
    if colors.dtype != torch.uint8:
        raise TypeError("clean_pvnet_amd.render: colors must be uint8, got %s" % colors.dtype)
    dev = pose.device
    md = pts.to(device=dev, dtype=torch.float32).contiguous()
    cl = colors.to(device=dev).contiguous()
    fc = faces.to(device=dev, dtype=torch.int32).contiguous()
    ps = pose.to(dtype=torch.float64)
    if ps.dim() == 3:
        ps = ps[:, None]
    ps = ps.contiguous()
    if ps.dim() != 4 or tuple(ps.shape[2:]) != (3, 4) or ps.shape[0] < 1:
        raise ValueError("clean_pvnet_amd.render: pose must be [B,M,3,4] or [B,3,4] with B >= 1, got %s" % (tuple(pose.shape),))
    B, M = int(ps.shape[0]), int(ps.shape[1])
    if not 1 <= M <= MAX_M or B * M > 65535:
        raise ValueError("clean_pvnet_amd.render: M must lie in [1, %d] and B*M must not exceed 65535, got B=%d M=%d" % (MAX_M, B, M))
    if md.dim() != 2 or md.shape[1] != 3 or md.shape[0] < 1 or tuple(cl.shape) != tuple(md.shape):
        raise ValueError("clean_pvnet_amd.render: pts must be [N >= 1, 3] and colors [N, 3], got %s and %s" % (tuple(md.shape), tuple(cl.shape)))
    if fc.dim() != 2 or fc.shape[1] != 3:
        raise ValueError("clean_pvnet_amd.render: faces must be [F,3], got %s" % (tuple(fc.shape),))
    N, F = int(md.shape[0]), int(fc.shape[0])
    rg, Nmax, Fmax = check_ranges(ranges, N, F)
    Km = K.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(Km.shape) not in ((3, 3), (B, 3, 3)):
        raise ValueError("clean_pvnet_amd.render: K must be [3,3] or [B,3,3], got %s" % (tuple(Km.shape),))
    ob = None
    if obj is not None:
        _native.need_cuda(obj, "obj", "render")
        if tuple(obj.shape) != (B, M) or obj.dtype not in (torch.int32, torch.int64):
            raise ValueError("clean_pvnet_amd.render: obj must be [B,M] = [%d,%d] int32, got %s %s" % (B, M, tuple(obj.shape), obj.dtype))
        ob = obj.to(device=dev, dtype=torch.int32).contiguous()
    bgt = None
    if bg is not None:
        _native.need_cuda(bg, "bg", "render")
        if bg.dtype != torch.uint8 or tuple(bg.shape) != (B, H, W, 3):
            raise TypeError("clean_pvnet_amd.render: bg must be [%d,%d,%d,3] uint8, got %s %s" % (B, H, W, tuple(bg.shape), bg.dtype))
        bgt = bg.contiguous()
    bgc = (ctypes.c_uint8 * 3)(*[int(v) for v in bg_color])
    out = {"img": torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), "label": torch.empty(B, H, W, dtype=torch.uint8, device=dev),
           "depth": torch.empty(B, H, W, dtype=torch.float32, device=dev), "area": torch.empty(B, M, dtype=torch.int32, device=dev)}
    if return_face:
        out["face"] = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    d_ranges = _native.upload(rg, dev)
    ws, _ = _lib.workspace("pvv_render_workspace_bytes", dev, B, M, Nmax, H, W)
    _lib.call("pvv_render_color", dev, md.data_ptr(), cl.data_ptr(), fc.data_ptr() if F else None, N, F, d_ranges.data_ptr(),
              int(rg.shape[0]), Nmax, Fmax, ps.data_ptr(), _native.ptr(ob), Km.data_ptr(), int(Km.dim() == 3), _native.ptr(bgt), bgc,
              B, M, H, W, float(near), float(far), float(ambient), ws.data_ptr(), ws.numel(), out["img"].data_ptr(),
              out["label"].data_ptr(), out["depth"].data_ptr(), out["area"].data_ptr(), _native.ptr(out.get("face")))
    return out


class SceneRenderer:
    """Several meshes on the device, rendered together: ``meshes`` is a list of (pts [n,3], colors [n,3] uint8, faces [f,3]) as
    arrays or tensors; they are concatenated once and ``ranges`` is built from their sizes.  ``__call__(pose, obj=None, K=None,
    bg=None)`` renders a batch with the stored size, camera and defaults (``near``, ``far``, ``ambient``, ``bg_color``,
    ``return_face``) and returns ``render_color``'s dict."""

    def __init__(self, meshes, size, K=None, device="cuda", **defaults):
        import torch
        if len(meshes) < 1:
            raise ValueError("clean_pvnet_amd.render: SceneRenderer needs at least one mesh")
        unknown = set(defaults) - {"near", "far", "ambient", "bg_color", "return_face"}
        if unknown:
            raise TypeError("clean_pvnet_amd.render: unknown defaults %s" % sorted(unknown))
        pts = [torch.as_tensor(m[0]).to(device=device, dtype=torch.float32).reshape(-1, 3) for m in meshes]
        col = [torch.as_tensor(m[1]).to(device=device).reshape(-1, 3) for m in meshes]
        fcs = [torch.as_tensor(m[2]).to(device=device, dtype=torch.int32).reshape(-1, 3) for m in meshes]
        if pts[0].device.type != "cuda":
            raise RuntimeError("clean_pvnet_amd.render: SceneRenderer needs a CUDA device; there is no CPU fallback")
        rows, v0, f0 = [], 0, 0
        for p, f in zip(pts, fcs):
            rows.append((v0, p.shape[0], f0, f.shape[0]))
            v0, f0 = v0 + p.shape[0], f0 + f.shape[0]
        self.pts, self.colors, self.faces = torch.cat(pts).contiguous(), torch.cat(col).contiguous(), torch.cat(fcs).contiguous()
        self.ranges = np.array(rows, np.int32)
        self.size = (int(size[0]), int(size[1]))
        self.K = None if K is None else torch.as_tensor(K).to(device=device, dtype=torch.float64)
        self.defaults = defaults

    def __call__(self, pose, obj=None, K=None, bg=None):
        K = self.K if K is None else K
        if K is None:
            raise ValueError("clean_pvnet_amd.render: SceneRenderer was built without K; pass it with the call")
        return render_color(self.pts, self.colors, self.faces, pose, K, self.size, ranges=self.ranges, obj=obj, bg=bg, **self.defaults)
