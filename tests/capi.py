"""ctypes view of the C ABI declared in include/pvnet_vote.h -- what a non-Python host would bind.
The GPU parity tests call the library through this (raw device pointers + the current HIP stream)
as well as through the pybind11 module."""
import ctypes
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
# PVV_LIBPATH: tools/variant_time.py points the same binding at an experimental build of the library
LIBPATH = os.environ.get("PVV_LIBPATH") or os.path.join(ROOT, "clean-pvnet_amd", "libpvnet_vote.so")

# clean-pvnet_amd/_native.py on its own (it needs neither torch nor the package): the reader of the headers
_spec = importlib.util.spec_from_file_location("_pvnet_native", os.path.join(ROOT, "clean-pvnet_amd", "_native.py"))
native = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(native)

c_i32, c_i64, c_u64, c_f32, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p


class Problem(ctypes.Structure):
    _fields_ = [("B", c_i32), ("H", c_i32), ("W", c_i32), ("K", c_i32), ("hn", c_i32),
                ("mask_elem_size", c_i32), ("min_num", c_i32), ("max_num", c_i32), ("cap", c_i32),
                ("singular_policy", c_i32), ("inlier_thresh", c_f32),
                ("mask_stride", c_i64 * 3), ("vertex_stride", c_i64 * 5), ("seed", c_u64),
                ("seg_classes", c_i32), ("first_image", c_i32), ("seg_stride", c_i64 * 4),
                ("count_kernel", c_i32), ("flags", c_i32), ("d_draws_out", vp), ("ev_count_begin", vp), ("ev_count_end", vp),
                ("d_status", vp), ("ev_marks", vp)]


def declared(name="vote"):
    """The functions include/pvnet_<name>.h declares, as the product's own reader finds them."""
    return set(native.declarations("pvnet_%s.h" % name))


def exported(name="vote"):
    """The functions libpvnet_<name>.so defines for others (``T`` in the dynamic symbol table)."""
    nm = subprocess.check_output(["nm", "-D", "--defined-only", libpath(name)]).decode()
    return {line.split()[-1] for line in nm.splitlines() if " T " in line}


def declared_symbols():
    """Every function the voting header declares."""
    return sorted(declared())


def libpath(name):
    return LIBPATH if name == "vote" else os.path.join(ROOT, "clean-pvnet_amd", "libpvnet_%s.so" % name)


_libs = {}


def load(name="vote"):
    """libpvnet_<name>.so with the signature of every function its header declares (a ``pvv_problem *`` is a void pointer:
    pass ``ctypes.byref(problem)``)."""
    if name not in _libs:
        _libs[name] = native.declare(ctypes.CDLL(libpath(name)), "pvnet_%s.h" % name)
    return _libs[name]


def problem(mask, vertex, hn, thresh, min_num=5, max_num=30000, policy=0, seed=0, count_kernel=0, draws_out=None,
            first_image=0, cap=None, status=None, flags=0):
    L = load()
    p = Problem()
    p.B, p.H, p.W, p.K, _ = vertex.shape
    p.hn = hn
    p.mask_elem_size = mask.element_size()
    p.min_num, p.max_num = min_num, max_num
    p.cap = L.pvv_default_cap(p.H, p.W, max_num) if cap is None else cap
    p.count_kernel = count_kernel
    p.flags = flags
    p.first_image = first_image
    p.d_draws_out = None if draws_out is None else draws_out.data_ptr()
    p.d_status = None if status is None else status.data_ptr()
    p.singular_policy = policy
    p.inlier_thresh = thresh
    p.mask_stride[:] = mask.stride()
    p.vertex_stride[:] = vertex.stride()
    p.seed = seed
    return p


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(code):
    assert code == 0, "pvv call failed (%d): %s" % (code, load().pvv_last_error().decode())


def v3(mask, vertex, hn, thresh, idxs=None, selection=None, **kw):
    """pvv_ransac_voting_v3 on torch CUDA tensors -> (out [B,K,2], win_counts [B,K], tn [B])."""
    import torch
    L = load()
    if selection is not None:      # injected draws may keep any number of pixels: reserve the whole image (as the pybind shim does)
        kw.setdefault("cap", vertex.shape[1] * vertex.shape[2])
    p = problem(mask, vertex, hn, thresh, **kw)
    n = L.pvv_workspace_bytes(ctypes.byref(p))
    assert n > 0, L.pvv_last_error()
    dev = vertex.device
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty(p.B, p.K, 2, device=dev)
    win = torch.empty(p.B, p.K, dtype=torch.int32, device=dev)
    tn = torch.empty(p.B, dtype=torch.int32, device=dev)
    check(L.pvv_ransac_voting_v3(ctypes.byref(p), ptr(mask), ptr(vertex), ptr(idxs), ptr(selection), ptr(ws), n,
                                 ptr(out), ptr(win), ptr(tn), stream()))
    return out, win, tn


def estimate(mask, vertex, mean, hn_total, thresh, idxs=None, selection=None, want_counts=True, **kw):
    """want_counts=False: no hypothesis / count outputs (NULL) -- only then may the pass count in stages."""
    import torch
    L = load()
    if selection is not None:
        kw.setdefault("cap", vertex.shape[1] * vertex.shape[2])
    p = problem(mask, vertex, hn_total, thresh, **kw)
    n = L.pvv_workspace_bytes(ctypes.byref(p))
    assert n > 0, L.pvv_last_error()
    dev = vertex.device
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    cov = torch.empty(p.B, p.K, 2, 2, device=dev)
    hyp = torch.empty(p.B, p.K, hn_total, 2, device=dev)
    counts = torch.empty(p.B, p.K, hn_total, dtype=torch.int32, device=dev)
    tn = torch.empty(p.B, dtype=torch.int32, device=dev)
    check(L.pvv_estimate_voting_distribution(ctypes.byref(p), ptr(mask), ptr(vertex), ptr(idxs), ptr(selection),
                                             ptr(mean), ptr(ws), n, ptr(cov), ptr(hyp) if want_counts else None,
                                             ptr(counts) if want_counts else None, ptr(tn), None, stream()))
    return cov, hyp, counts, tn
