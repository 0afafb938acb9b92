"""Poisoned, guarded memory for the device entry points (test infrastructure only).

``Guarded`` is a ``TorchDispatchMode`` used as a context manager.  While it is active every factory call that creates a new
tensor on the target device (``torch.empty`` from Python, ``at::empty`` from the pybind shim, ``zeros`` / ``full`` / ``ones`` and
their ``*_like`` / ``new_*`` forms) is served from an arena of its own:

    [ head band: G bytes ][ body: n bytes ][ tail band: pad + G bytes ]          G = 512, pad rounds n up to a multiple of G

``G`` is the caching allocator's own granularity, so the body is aligned exactly as a plain allocation is.  The tensor handed out
is the body, viewed as the requested dtype / shape / strides; the tail band starts at the very next byte.  The bands hold one byte
value, the body holds ``fill`` (one of ``FILLS``) unless the op itself defines the contents.  Arenas live until the mode object
dies, so no arena reuses another's memory.

    check()           synchronise, return one ``Violation`` per arena whose bands changed (op, shape, first offending offset
                      relative to the body: negative = before it, >= n = past its end)
    owns(t)           whether ``t``'s storage is a recorded arena
    guarded_copy(t)   ``t`` in an arena whose bands are 0xFF (NaN in every float type, -1 in every integer type): an over-read
                      that reaches a result changes that result; ``inputs_changed()`` lists the copies whose body was written
    workspaces        [(nbytes asked, tensor)] of every ``_native.workspace`` call made while the mode was active (the wrapper
                      passes the size through as the product asked for it)

What three runs of one call under the three fills show: a store outside an output or workspace (``check()``), an output element
that is never written (the results differ between fills), a result that depends on what the workspace held before the call (same).
"""
import torch
from torch.utils._python_dispatch import TorchDispatchMode

G = 512
FILLS = (0x00, 0xFF, 0xA5)
BAND = 0x5A              # bands of factory arenas: differs from every fill, so a fill-valued store into a band shows
INPUT_BAND = 0xFF        # bands of guarded_copy arenas

_aten = torch.ops.aten
# ops whose result is a new tensor with contents the caller must not rely on / with defined contents (value or None = fill)
_FACTORIES = {
    _aten.empty.memory_format: None, _aten.empty_like.default: None, _aten.new_empty.default: None,
    _aten.empty_strided.default: None, _aten.new_empty_strided.default: None,
    _aten.zeros.default: 0, _aten.zeros_like.default: 0, _aten.new_zeros.default: 0,
    _aten.ones.default: 1, _aten.ones_like.default: 1, _aten.new_ones.default: 1,
    _aten.full.default: "arg", _aten.full_like.default: "arg", _aten.new_full.default: "arg",
}


class Violation:
    def __init__(self, arena, offset):
        self.arena, self.offset = arena, offset

    def __repr__(self):
        a = self.arena
        return "<band of arena #%d (%s, shape %s, %s, %d bytes, %s) changed at body offset %d>" % (
            a.index, a.op, tuple(a.shape), a.dtype, a.n, a.kind, self.offset)


class Arena:
    def __init__(self, index, op, kind, buf, n, tensor, band):
        self.index, self.op, self.kind, self.buf, self.n, self.tensor, self.band = index, op, kind, buf, n, tensor, band
        self.shape, self.dtype = tuple(tensor.shape), tensor.dtype
        self.snapshot = None

    @property
    def body(self):
        return self.buf[G:G + self.n]

    def first_changed(self):
        """Offset (relative to the body) of the first band byte that no longer holds the band value, or None."""
        head = (self.buf[:G] != self.band).nonzero()
        if head.numel():
            return int(head[0]) - G
        tail = (self.buf[G + self.n:] != self.band).nonzero()
        if tail.numel():
            return self.n + int(tail[0])
        return None


def _extent(shape, strides):
    """Elements of storage a dense-or-not strided tensor spans (0 for an empty one)."""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, strides))


class Guarded(TorchDispatchMode):
    def __init__(self, device, fill=0xA5):
        super().__init__()
        assert fill in FILLS, fill
        self.device, self.fill = torch.device(device), fill
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.arenas, self.workspaces = [], []
        self._native = self._saved_workspace = None

    # -- arenas ---------------------------------------------------------------------------------------------------------------
    def _arena(self, op, kind, meta, band, fill):
        """A new arena for a tensor of ``meta``'s dtype / shape / strides; body = ``fill`` bytes.  Runs with the mode off."""
        itemsize = meta.element_size()
        n = _extent(meta.shape, meta.stride()) * itemsize
        tail = (-n) % G + G
        buf = torch.empty(G + n + tail, dtype=torch.uint8, device=self.device)
        buf.fill_(band)
        buf[G:G + n].fill_(fill)
        t = buf[G:G + n].view(meta.dtype).as_strided(tuple(meta.shape), tuple(meta.stride()))
        a = Arena(len(self.arenas), op, kind, buf, n, t, band)
        self.arenas.append(a)
        return a

    def _same_device(self, d):
        d = torch.device(d)
        if d.type != self.device.type:
            return False
        if d.type == "cuda":
            return (torch.cuda.current_device() if d.index is None else d.index) == self.device.index
        return True

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func not in _FACTORIES:
            return func(*args, **kwargs)
        meta = func(*args, **{**kwargs, "device": "meta", "pin_memory": False})     # dtype, shape and strides as the op decides
        device = kwargs.get("device")
        if device is None:
            device = args[0].device if args and isinstance(args[0], torch.Tensor) else torch.empty(0).device
        if not self._same_device(device) or meta.layout != torch.strided or meta.is_quantized:
            return func(*args, **kwargs)
        a = self._arena(str(func), "factory", meta, BAND, self.fill)
        value = _FACTORIES[func]
        if value == "arg":                           # full(size, v), full_like(t, v), new_full(t, size, v)
            value = kwargs["fill_value"] if "fill_value" in kwargs else args[2 if func is _aten.new_full.default else 1]
        if value is not None:
            a.tensor.fill_(value)
        return a.tensor

    def guarded_copy(self, t):
        """``t`` (values, dtype, shape, strides) on the target device inside an arena with 0xFF bands."""
        with torch.utils._python_dispatch._disable_current_modes():
            src = t.detach()
            meta = torch.empty_strided(tuple(src.shape), tuple(src.stride()), dtype=src.dtype, device="meta")
            a = self._arena("guarded_copy", "input", meta, INPUT_BAND, INPUT_BAND)
            a.tensor.copy_(src)
            a.snapshot = a.body.clone()
            return a.tensor

    # -- questions ------------------------------------------------------------------------------------------------------------
    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self):
        self._sync()
        with torch.utils._python_dispatch._disable_current_modes():
            found = [(a, a.first_changed()) for a in self.arenas]
        return [Violation(a, off) for a, off in found if off is not None]

    def inputs_changed(self):
        """The guarded_copy arenas whose body no longer holds what was copied in."""
        self._sync()
        with torch.utils._python_dispatch._disable_current_modes():
            return [a for a in self.arenas if a.snapshot is not None and not torch.equal(a.body, a.snapshot)]

    def owns(self, t):
        if not isinstance(t, torch.Tensor) or t.device.type != self.device.type:
            return False
        p = t.untyped_storage().data_ptr()
        return any(a.buf.untyped_storage().data_ptr() == p for a in self.arenas)

    # -- the workspace hook ---------------------------------------------------------------------------------------------------
    def __enter__(self):
        import lib
        lib._register_clean_pvnet_amd()
        from clean_pvnet_amd import _native
        self._native, self._saved_workspace = _native, _native.workspace
        original = self._saved_workspace

        def workspace(nbytes, dev):
            ws = original(nbytes, dev)
            self.workspaces.append((int(nbytes), ws))
            return ws
        _native.workspace = workspace
        return super().__enter__()

    def __exit__(self, *exc):
        try:
            return super().__exit__(*exc)
        finally:
            self._native.workspace = self._saved_workspace
