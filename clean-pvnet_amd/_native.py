"""The one loader and the one calling convention of the ctypes-bound native libraries (``libpvnet_vote.so`` for ``crop`` and ``dcn``, ``libpvnet_nn.so``,
``libpvnet_pnp.so``, ``libpvnet_pose.so``, ``libpvnet_metrics.so``, ``libpvnet_vsd.so``, ``libpvnet_icp.so``; ``_build.py`` has the
table).

Every device entry point of these libraries takes the stream as its last argument and returns 0 on success: ``call`` is that
convention, ``load`` binds a library with its signatures, ``need_cuda`` / ``workspace`` / ``ptr`` are what the wrappers
share around a call, ``call_named`` / ``check_images`` / ``u8`` / ``upload`` what the image modules (``augment``, ``ct_augment``,
``tless_augment``, ``crop``) share in front of one.  torch is imported where it is used, so a host-pointer wrapper (``nn_utils``) loads without it.
There is no CPU fallback anywhere behind this module.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PTR, INT, LONGLONG, DOUBLE, SIZE = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_size_t


def load(module, libname, signatures):
    """``CDLL`` of ``libname`` next to this file for ``clean_pvnet_amd.<module>``, with ``restype`` / ``argtypes`` set from
    ``signatures``: {symbol: (restype, argtypes)}."""
    try:
        lib = ctypes.CDLL(os.path.join(HERE, libname))
    except OSError as e:
        raise ImportError("clean_pvnet_amd.%s: %s is not built (run `python __graft_entry__.py`); "
                          "there is no CPU fallback. Original error: %s" % (module, libname, e)) from e
    for symbol, (restype, argtypes) in signatures.items():
        fn = getattr(lib, symbol)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def need_cuda(t, what, module):
    import torch
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("clean_pvnet_amd.%s: %s must be a CUDA tensor; there is no CPU fallback" % (module, what))


def call(lib, symbol, dev, *args):
    """``lib.<symbol>(*args, stream)`` on the current stream of ``dev``; a non-zero return is a RuntimeError."""
    import torch
    with torch.cuda.device(dev):
        rc = getattr(lib, symbol)(*args, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (symbol, rc))


def call_named(module, lib, symbol, dev, *args):
    """``call`` for a library that keeps its last error (``pvv_last_error``): a failure names ``clean_pvnet_amd.<module>`` and
    says what the library recorded."""
    try:
        call(lib, symbol, dev, *args)
    except RuntimeError as e:
        raise RuntimeError("clean_pvnet_amd.%s: %s: %s" % (module, e, lib.pvv_last_error().decode())) from None


def u8(t):
    """``t`` contiguous, a bool tensor viewed as uint8."""
    import torch
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def upload(array, dev):
    """The bytes of the host array as a device tensor: one pinned block, one non-blocking copy."""
    import torch
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).pin_memory().to(dev, non_blocking=True)


def check_images(img, what, module, max_batch=None, max_side=None):
    """``img`` must be a [B,H,W,3] uint8 CUDA tensor, with limits: B in [1, max_batch] and the sides in [1, max_side]; returns
    (B, H, W).  Without limits the caller checks them."""
    import torch
    need_cuda(img, what, module)
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise TypeError("clean_pvnet_amd.%s: %s must be [B,H,W,3] uint8, got %s %s" % (module, what, tuple(img.shape), img.dtype))
    B, H, W = (int(v) for v in img.shape[:3])
    if max_batch is not None and not (1 <= B <= max_batch and 1 <= H <= max_side and 1 <= W <= max_side):
        raise ValueError("clean_pvnet_amd.%s: B must lie in [1, %d] and the sides in [1, %d], got %s" % (module, max_batch, max_side, tuple(img.shape)))
    return B, H, W


def workspace(nbytes, dev):
    """``nbytes`` (at least 16) of uninitialised device memory from the caching allocator.  A caller must not rely on its contents --
    a block comes back as the last call left it -- and every kernel clears what it assumes clear: tests/test_gpu_guarded.py enforces
    this by running each entry point on workspaces filled with 0x00, 0xFF and 0xA5."""
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)   # caching allocator: stream-ordered, no hipMalloc per call


def ptr(t):
    return None if t is None else t.data_ptr()
