"""The one loader and the one calling convention of the ctypes-bound native libraries (``libpvnet_vote.so`` for everything but the
voting call itself, ``libpvnet_nn.so``, ``libpvnet_pnp.so``, ``libpvnet_pose.so``, ``libpvnet_metrics.so``, ``libpvnet_vsd.so``,
``libpvnet_icp.so``; ``_build.py`` has the table).

Every device entry point of these libraries takes the stream as its last argument and returns 0 on success.  The header states
the signatures: ``libpvnet_<name>.so`` is opened with the ``restype`` / ``argtypes`` of every function ``include/pvnet_<name>.h``
declares (``declarations``; a declaration its rules do not cover is an ImportError, never a default), so no module, test or tool
writes a type down.  A module keeps what ``bind`` returns as its ``_lib``: a ``Library``, whose attributes are the ctypes functions,
whose ``call`` is that convention and whose ``workspace`` asks a size query and allocates.  The module's name, the prefix of its
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
import re

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
PTR, INT, LONGLONG, DOUBLE, SIZE = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_size_t

# The scalar types of the C ABI.  A parameter with a ``*`` is PTR whatever it points to; ``const char *`` is the one pointer returned.
_SCALARS = {"int": INT, "int32_t": INT, "long long": LONGLONG, "int64_t": LONGLONG, "size_t": SIZE, "double": DOUBLE,
            "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint}
_TYPE_WORDS = {"int", "long", "short", "char", "signed", "unsigned", "float", "double", "void"}     # never a parameter's name
_declarations, _libraries = {}, {}


def parse(text, header="<text>"):
    """{symbol: (restype, argtypes)} of every function the header text declares.  Comments, preprocessor lines, ``typedef
    struct {...}`` bodies and the ``extern "C"`` braces are dropped; each statement left must be a function declaration in the
    types above, and one that is not is an ImportError that names ``header`` and the declaration."""
    def refuse(declaration):
        return ImportError("clean_pvnet_amd._native: %s: no ctypes rule covers `%s`" % (header, declaration))

    def scalar(words, declaration, named):
        m = re.fullmatch(r"(?:const )?(long long|\w+)(?: (\w+))?", words)
        if not m or m.group(1) not in _SCALARS or m.group(2) in _TYPE_WORDS or (m.group(2) and not named):
            raise refuse(declaration)
        return _SCALARS[m.group(1)]

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{};]*\{[^{}]*\}[^;]*;", " ", text)
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    found = {}
    for declaration in (" ".join(d.split()) for d in text.split(";")):
        if not declaration:
            continue
        m = re.fullmatch(r"(.*?) ?\b(\w+) ?\(([^()]*)\)", declaration)
        if not m or m.group(2) in found:
            raise refuse(declaration)
        returns, symbol, params = m.group(1), m.group(2), m.group(3).strip()
        if returns == "void":
            restype = None
        elif "*" in returns:
            if not re.fullmatch(r"const char ?\*", returns):
                raise refuse(declaration)
            restype = ctypes.c_char_p
        else:
            restype = scalar(returns, declaration, named=False)
        found[symbol] = (restype, [] if params in ("", "void") else
                         [PTR if "*" in p else scalar(p.strip(), declaration, named=True) for p in params.split(",")])
    return found


def declarations(header):
    """``parse`` of ``include/<header>``, read once per process."""
    if header not in _declarations:
        try:
            with open(os.path.join(INCLUDE, header)) as f:
                text = f.read()
        except OSError as e:
            raise ImportError("clean_pvnet_amd._native: include/%s, which states the signatures of its library, cannot be read; "
                              "there is no CPU fallback. Original error: %s" % (header, e)) from e
        _declarations[header] = parse(text, "include/" + header)
    return _declarations[header]


def declare(lib, header):
    """``lib``, an open ``CDLL``, with the ``restype`` / ``argtypes`` of every function ``include/<header>`` declares."""
    for symbol, (restype, argtypes) in declarations(header).items():
        fn = getattr(lib, symbol)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def load(module, libname):
    """``CDLL`` of ``lib<name>.so`` next to this file for ``clean_pvnet_amd.<module>``, declared by ``include/<name>.h``: opened
    and declared once per process, the modules bound to one library share it."""
    if libname not in _libraries:
        try:
            lib = ctypes.CDLL(os.path.join(HERE, libname))
        except OSError as e:
            raise ImportError("clean_pvnet_amd.%s: %s is not built (run `python __graft_entry__.py`); "
                              "there is no CPU fallback. Original error: %s" % (module, libname, e)) from e
        _libraries[libname] = declare(lib, libname[len("lib"):-len(".so")] + ".h")
    return _libraries[libname]


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
    :param last_error:   the symbol of the library's error string (``"pvv_last_error"``); None for a library that keeps none: its
                         calls fail with the plain message and its size queries refuse nothing
    :param prefix:       what a refused workspace's message starts with; ``clean_pvnet_amd.<module>`` by default
    :param plain_calls:  a failed call keeps the plain message although the library has an error string (``crop``, ``det_eval``)"""

    def __init__(self, module, libname, last_error=None, prefix=None, plain_calls=False):
        self._cdll = load(module, libname)
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


bind = Library                       # ``_lib = _native.bind("module", "libpvnet_x.so", last_error="pvv_last_error")``


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
