"""CPU: the guarded-memory helper of tests/guarded.py holds -- each fault it exists to find, planted by hand inside an arena, is
reported; each factory op is carved; the workspace hook comes and goes with the mode."""
import pytest
import torch

from tests import guarded
from tests.guarded import G, Guarded

CPU = torch.device("cpu")


def _arena_of(mode, t):
    (a,) = [a for a in mode.arenas if a.buf.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()]
    return a


def test_a_byte_written_one_before_the_body_is_reported():
    with Guarded(CPU, fill=0xA5) as m:
        first = torch.empty(8, dtype=torch.float32)
        t = torch.empty(5, 3, dtype=torch.float32)
        assert m.check() == []
        a = _arena_of(m, t)
        assert a is m.arenas[1] and t.data_ptr() == a.buf.data_ptr() + G
        under = torch.as_strided(a.buf, (1,), (1,), G - 1)                   # the last byte of the head band: inside the arena
        under.fill_(0)
        (v,) = m.check()
    assert v.arena is a and v.offset == -1 and v.arena.shape == (5, 3) and "empty" in v.arena.op
    assert _arena_of(m, first) is m.arenas[0]


def test_a_byte_written_one_past_the_end_is_reported():
    with Guarded(CPU, fill=0x00) as m:
        t = torch.empty(7, 3, dtype=torch.uint8)                              # n = 21: no multiple of 16
        torch.empty(4)
        a = _arena_of(m, t)
        assert a.n == 21 and a.buf.numel() == G + 21 + (G - 21) + G
        t.fill_(9)                                                            # a full, in-bounds write changes no band
        assert m.check() == []
        over = torch.as_strided(a.buf, (1,), (1,), G + a.n)                   # the very next byte after the body
        over.fill_(9)
        (v,) = m.check()
    assert v.arena is a and v.offset == 21 and "21 bytes" in repr(v)


def test_a_store_of_the_fill_value_into_a_band_is_reported():
    """The band byte differs from every fill, so a kernel that copies stale body bytes past the end still shows."""
    assert guarded.BAND not in guarded.FILLS
    for fill in guarded.FILLS:
        with Guarded(CPU, fill=fill) as m:
            t = torch.empty(3, dtype=torch.int32)
            a = _arena_of(m, t)
            a.buf[G + a.n + 2] = fill
            (v,) = m.check()
        assert v.offset == a.n + 2


def test_an_unwritten_output_element_differs_between_fills():
    def kernel(x):
        out = torch.empty(x.shape[0], dtype=torch.float32)
        out[:-1] = x[:-1] * 2                                                  # forgets the last element
        return out
    x = torch.arange(6, dtype=torch.float32)
    got = []
    for fill in guarded.FILLS:
        with Guarded(CPU, fill=fill) as m:
            out = kernel(m.guarded_copy(x))
            assert m.check() == [] and m.owns(out)
            got.append(out.view(torch.uint8).clone())
    assert all(torch.equal(g[:-4], got[0][:-4]) for g in got)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2]) and not torch.equal(got[0], got[2])
    assert got[0][-4:].tolist() == [0x00] * 4 and got[1][-4:].tolist() == [0xFF] * 4 and got[2][-4:].tolist() == [0xA5] * 4


def test_the_ff_fill_is_nan_in_floats_and_minus_one_in_integers():
    with Guarded(CPU, fill=0xFF):
        for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            assert bool(torch.isnan(torch.empty(3, dtype=dt)).all())
        for dt in (torch.int8, torch.int16, torch.int32, torch.int64):
            assert torch.empty(3, dtype=dt).tolist() == [-1] * 3


LIKE = torch.arange(12, dtype=torch.float64).reshape(3, 4)
FACTORIES = {
    "empty": (lambda: torch.empty(3, 5, dtype=torch.int16), None),
    "empty_like": (lambda: torch.empty_like(LIKE), None),
    "new_empty": (lambda: LIKE.new_empty((2, 7)), None),
    "zeros": (lambda: torch.zeros(2, 3, dtype=torch.int64), 0),
    "zeros_like": (lambda: torch.zeros_like(LIKE), 0),
    "new_zeros": (lambda: LIKE.new_zeros((0, 9, 2), dtype=torch.float32), 0),
    "full": (lambda: torch.full((5,), -1.0), -1.0),
    "full_scalar": (lambda: torch.full((), 7, dtype=torch.int64), 7),
    "full_like": (lambda: torch.full_like(LIKE, float("nan")), float("nan")),
    "ones": (lambda: torch.ones(6, dtype=torch.uint8), 1),
    "ones_like": (lambda: torch.ones_like(LIKE), 1),
    "new_ones": (lambda: LIKE.new_ones(4), 1),
}


@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_each_factory_op_is_carved(name):
    make, value = FACTORIES[name]
    plain = make()
    for fill in guarded.FILLS:
        with Guarded(CPU, fill=fill) as m:
            t = make()
            assert m.owns(t) and len(m.arenas) == 1
            a = m.arenas[0]
            assert a.kind == "factory" and a.n == t.numel() * t.element_size() and (t.numel() == 0 or t.data_ptr() == a.buf.data_ptr() + G)
            assert (a.buf.numel() - a.n - 2 * G) in range(G) and a.buf.numel() % G == 0
            assert t.shape == plain.shape and t.dtype == plain.dtype and t.stride() == plain.stride()
            if value is None:
                assert a.body.tolist() == [fill] * a.n
            else:
                assert torch.equal(t, plain, ) or (value != value and bool(torch.isnan(t).all()))
            assert a.buf[:G].tolist() == [guarded.BAND] * G and set(a.buf[G + a.n:].tolist()) == {guarded.BAND}
            assert m.check() == []


def test_a_strided_layout_is_kept():
    src = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).permute(2, 0, 1)
    with Guarded(CPU) as m:
        like = torch.empty_like(src)                                           # preserve_format: the permuted strides
        copy = m.guarded_copy(src[:, :, ::2])                                  # a non-dense view: the arena spans its extent
        assert like.stride() == src.stride() and m.owns(like)
        assert copy.stride() == src[:, :, ::2].stride() and torch.equal(copy, src[:, :, ::2]) and m.owns(copy)
        assert m.check() == [] and m.inputs_changed() == []


def test_a_written_input_is_reported():
    x = torch.arange(10, dtype=torch.int32)
    with Guarded(CPU) as m:
        a, b = m.guarded_copy(x), m.guarded_copy(x)
        assert torch.equal(a, x) and m.arenas[0].buf[:G].tolist() == [0xFF] * G
        assert m.inputs_changed() == []
        b[3] = 99
        assert m.inputs_changed() == [m.arenas[1]] and m.check() == []


def test_tensors_of_other_devices_and_conversions_pass_through():
    with Guarded(CPU) as m:
        t = torch.empty(4, device="meta")
        c = torch.arange(4).to(torch.float32)                                  # aten._to_copy: an input conversion, not carved
        assert len(m.arenas) == 0 and not m.owns(t) and not m.owns(c)


def test_owns_is_false_for_a_tensor_made_outside_the_mode():
    outside = torch.empty(16)
    with Guarded(CPU) as m:
        inside = torch.empty(16)
        assert m.owns(inside) and m.owns(inside[3:9]) and m.owns(inside.view(4, 4)) and not m.owns(outside)
    after = torch.empty(16)
    assert not m.owns(after) and not m.owns(None)


def test_leaving_the_mode_restores_the_workspace_function(pkg):
    from clean_pvnet_amd import _native
    before = _native.workspace
    with Guarded(CPU) as m:
        assert _native.workspace is not before
        ws = _native.workspace(100, CPU)
        tiny = _native.workspace(0, CPU)
        assert m.workspaces[0][0] == 100 and m.workspaces[0][1] is ws and ws.numel() == 100 and m.owns(ws)     # not rounded
        assert m.workspaces[1][0] == 0 and tiny.numel() == 16 and m.owns(tiny)
    assert _native.workspace is before
    with pytest.raises(ZeroDivisionError):
        with Guarded(CPU):
            1 / 0
    assert _native.workspace is before

