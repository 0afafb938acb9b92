"""The one loader and the one calling convention of the ctypes-bound native libraries (``libpvnet_vote.so`` for everything but the
voting call itself, ``libpvnet_nn.so``, ``libpvnet_pnp.so``, ``libpvnet_pose.so``, ``libpvnet_metrics.so``, ``libpvnet_vsd.so``,
``libpvnet_icp.so``; ``_build.py`` has the table).

Every device entry point of these libraries takes the stream as its last argument and returns 0 on success.  A module states its
signatures once and keeps what ``bind`` returns as its ``_lib``: a ``Library``, whose attributes are the ctypes functions, whose
``call`` is that convention and whose ``workspace`` asks a size query and allocates.  The module's name, the prefix of its
messages and the library's error string (``pvv_last_error``, where the library keeps one) are fixed there, so no wrapper repeats
them around a launch.  ``Library`` is built on the functions below it, which stay importable: ``load`` opens a library, ``call`` /
``call_named`` are the convention without and with the error string, ``need_cuda`` / ``workspace`` / ``ptr`` what the wrappers share
around a call, and ``check_tensors`` / ``check_images`` / ``per_image`` / ``u8`` / ``upload`` / ``upload_parts`` what they share in
front of one.  ``need_cuda`` and ``workspace`` are looked up in this module when they are called, so a test that replaces either
is seen by everything above.  torch and numpy are imported where they are used, so a host-pointer wrapper (``nn_utils``) loads
without them; the autograd function of the two fused losses, which needs torch to be defined, is in ``_loss.py``.
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


def call_named(module, lib, symbol, dev, *args, last_error="pvv_last_error"):
    """``call`` for a library that keeps its last error (``last_error``): a failure names ``clean_pvnet_amd.<module>`` and
    says what the library recorded."""
    try:
        call(lib, symbol, dev, *args)
    except RuntimeError as e:
        raise RuntimeError("clean_pvnet_amd.%s: %s: %s" % (module, e, getattr(lib, last_error)().decode())) from None


def workspace(nbytes, dev):
    """``nbytes`` (at least 16) of uninitialised device memory from the caching allocator.  A caller must not rely on its contents --
    a block comes back as the last call left it -- and every kernel clears what it assumes clear: tests/test_gpu_guarded.py enforces
    this by running each entry point on workspaces filled with 0x00, 0xFF and 0xA5."""
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)   # caching allocator: stream-ordered, no hipMalloc per call


class Library:
    """``libname`` bound for ``clean_pvnet_amd.<module>`` (``load``'s ImportError when it is not built).  ``lib.<symbol>`` is the
    ctypes function, for the host-only entry points and the tests; every launch goes through ``call`` and every workspace
    through ``workspace``.
    :param signatures:   {symbol: (restype, argtypes)}
    :param last_error:   the symbol of the library's error string (``"pvv_last_error"``), whose signature is added here; None for
                         a library that keeps none: its calls fail with the plain message and its size queries refuse nothing
    :param prefix:       what a refused workspace's message starts with; ``clean_pvnet_amd.<module>`` by default
    :param plain_calls:  a failed call keeps the plain message although the library has an error string (``crop``, ``det_eval``)"""

    def __init__(self, module, libname, signatures, last_error=None, prefix=None, plain_calls=False):
        if last_error is not None:
            signatures = {last_error: (ctypes.c_char_p, []), **signatures}
        self._cdll = load(module, libname, signatures)
        self._module, self._last_error = module, last_error
        self._prefix = "clean_pvnet_amd.%s" % module if prefix is None else prefix
        self._named = last_error is not None and not plain_calls

    def __getattr__(self, symbol):
        return getattr(self._cdll, symbol)

    def call(self, symbol, dev, *args):
        """``<symbol>(*args, stream)`` on the current stream of ``dev``.  A non-zero return is a RuntimeError:
        ``clean_pvnet_amd.<module>: <symbol> failed (<rc>): <the library's last error>``, or the plain ``<symbol> failed (<rc>)``
        of a library without an error string (and of a module bound with ``plain_calls``)."""
        if self._named:
            call_named(self._module, self._cdll, symbol, dev, *args, last_error=self._last_error)
        else:
            call(self._cdll, symbol, dev, *args)

    def workspace(self, symbol, dev, *sizes, refused=lambda nbytes: nbytes == 0, error=ValueError):
        """(tensor, nbytes) for the size query ``<symbol>(*sizes)``: device memory from ``workspace`` above.  A size the
        library refuses -- ``refused(nbytes)``, 0 unless the query says otherwise -- allocates nothing and raises
        ``error("<prefix>: <the library's last error>")``."""
        nbytes = getattr(self._cdll, symbol)(*sizes)
        if self._last_error is not None and refused(nbytes):
            raise error("%s: %s" % (self._prefix, getattr(self._cdll, self._last_error)().decode()))
        return workspace(nbytes, dev), nbytes


bind = Library                       # ``_lib = _native.bind("module", "libpvnet_x.so", {...}, last_error="pvv_last_error")``


def ptr(t):
    return None if t is None else t.data_ptr()


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


def upload_parts(parts, dev):
    """``upload`` of the host arrays ``parts`` as one block, each a multiple of 4 bytes, those of 8-byte elements first: the
    device tensor and the device address of each part."""
    import numpy as np
    raw = [np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts]
    block = upload(np.concatenate(raw), dev)
    at, addresses = block.data_ptr(), []
    for r in raw:
        addresses.append(at)
        at += len(r)
    return block, addresses


def check_tensors(named, dtypes, module, phrases=()):
    """Device, then dtype, of every (name, tensor) of ``named``, in its order; shapes are the caller's and come after.
    ``dtypes`` is {name: the dtypes allowed} or one tuple of them for every name; a wrong one is a RuntimeError that lists
    them joined by "or", or says ``phrases[name]`` where a module words it otherwise."""
    for what, t in named:
        need_cuda(t, what, module)
    for what, t in named:
        allowed = dtypes[what] if isinstance(dtypes, dict) else dtypes
        if t.dtype not in allowed:
            phrase = phrases[what] if what in phrases else " or ".join(str(d).replace("torch.", "") for d in allowed)
            raise RuntimeError("clean_pvnet_amd.%s: %s must be %s, got %s" % (module, what, phrase, t.dtype))


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


def per_image(t, what, channels, H, W, module=None):
    """``t`` [B, channels, H, W] as (tensor, element stride between images): a view whose images are contiguous -- a channel
    slice of the network's output -- is taken as it is, by its stride.  With ``module`` the shape is checked first (a
    RuntimeError in that module's name); without, the caller has checked it."""
    if module is not None and (t.dim() != 4 or tuple(t.shape[1:]) != (channels, H, W)):
        raise RuntimeError("clean_pvnet_amd.%s: %s must be [B, %d, %d, %d], got %s" % (module, what, channels, H, W, tuple(t.shape)))
    image = channels * H * W
    if not t[:1].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < image):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else image)
