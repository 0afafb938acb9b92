"""CPU tests of the 2-byte input fields' C ABI (PVV_FLAG_VERTEX_F16 / _BF16, PVV_FLAG_SEG_F16 / _BF16): the header declares
the bits, pvv_workspace_bytes accepts each of them with the same answer as without (nothing is copied or widened into the
workspace), and the two bits of one pair together are refused -- no compute call is made here."""
import ctypes
import re

from tests import capi

FLAGS = {"PVV_FLAG_VERTEX_F16": 2, "PVV_FLAG_VERTEX_BF16": 4, "PVV_FLAG_SEG_F16": 8, "PVV_FLAG_SEG_BF16": 16}


def _problem(flags, B=64, H=480, W=640, K=9, hn=512, max_num=30000, count_kernel=0):
    L = capi.load()
    p = capi.Problem()
    p.B, p.H, p.W, p.K, p.hn, p.mask_elem_size, p.min_num, p.max_num = B, H, W, K, hn, 8, 5, max_num
    p.cap = L.pvv_default_cap(H, W, max_num)
    p.inlier_thresh, p.flags, p.count_kernel = 0.99, flags, count_kernel
    return p


def test_header_declares_the_half_input_flags():
    txt = open(capi.HEADER).read()
    for name, value in FLAGS.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, txt)
        assert m and int(m.group(1)) == value, name


def test_workspace_bytes_are_the_same_for_every_field_dtype():
    L = capi.load()
    for base in (0, 1):                                                  # with and without PVV_FLAG_DEVICE_RNG
        for shape in (dict(), dict(B=1, H=128, W=128, K=4, hn=64), dict(B=16, H=540, W=720, K=17, hn=2048),
                      dict(hn=128, max_num=100), dict(hn=4096, count_kernel=4)):
            want = L.pvv_workspace_bytes(ctypes.byref(_problem(base, **shape)))
            assert want > 0, L.pvv_last_error()
            for bits in (2, 4, 8, 16, 2 | 8, 2 | 16, 4 | 8, 4 | 16):
                got = L.pvv_workspace_bytes(ctypes.byref(_problem(base | bits, **shape)))
                assert got == want, (shape, bits, got, want, L.pvv_last_error())


def test_fused_un_pnp_workspace_and_staging_queries_ignore_the_dtype():
    L = capi.load()
    for bits in (0, 2, 4, 8, 16, 4 | 16):
        p = _problem(1 | bits)
        assert L.pvv_workspace_bytes_un_pnp(ctypes.byref(p), 4096) == L.pvv_workspace_bytes_un_pnp(ctypes.byref(_problem(1)), 4096)
        for B in (1, 8, 64):
            q, r = _problem(bits, B=B, hn=4096), _problem(0, B=B, hn=4096)
            assert L.pvv_estimate_counts_in_stages(ctypes.byref(q)) == L.pvv_estimate_counts_in_stages(ctypes.byref(r))
        mean, thr = ctypes.c_float(), ctypes.c_float()
        mean0, thr0 = ctypes.c_float(), ctypes.c_float()
        L.pvv_stage_hint_query(ctypes.byref(mean), ctypes.byref(thr), ctypes.byref(_problem(bits)), None)
        L.pvv_stage_hint_query(ctypes.byref(mean0), ctypes.byref(thr0), ctypes.byref(_problem(0)), None)
        assert thr.value == thr0.value


def test_both_bits_of_a_pair_are_refused():
    L = capi.load()
    for bits, names in ((2 | 4, (b"VERTEX_F16", b"VERTEX_BF16")), (8 | 16, (b"SEG_F16", b"SEG_BF16"))):
        for base in (0, 1):
            assert L.pvv_workspace_bytes(ctypes.byref(_problem(base | bits))) == 0
            msg = L.pvv_last_error()
            assert b"flags" in msg and all(n in msg for n in names), msg
    # bits beyond the known ones stay unknown
    assert L.pvv_workspace_bytes(ctypes.byref(_problem(32))) == 0 and b"unknown bits in flags" in L.pvv_last_error()
