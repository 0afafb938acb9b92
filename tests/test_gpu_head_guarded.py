"""PVNet's output head on poisoned, guarded memory (tests/guarded.py; ``guarded_runs`` of tests/test_gpu_guarded.py): under the three
fills no band of any arena changes, no input is written, the output lies in an arena and is the twin's -- the same bytes every
time -- and no workspace is asked for.  ``odd_k`` is smaller than one tile, ``reference_channels`` has partial last tiles in both
axes and stores bfloat16, whose two-byte elements put the band right behind a half-written word."""
import numpy as np
import pytest
import torch

from tests import head_twin as twin
from tests.test_gpu_guarded import guarded_runs

pytestmark = pytest.mark.gpu
KEYS = ("fm", "x", "weight1", "scale", "shift", "weight2", "bias2")


def _canon16(bits):
    """bfloat16 bit patterns with -0 as +0 and every NaN as one pattern."""
    bits = np.asarray(bits).astype(np.uint16).copy()
    bits[bits == 0x8000] = 0
    bits[(bits & 0x7FFF) > 0x7F80] = 0x7FC0
    return bits


def test_forward_and_upsample_smaller_than_a_tile(pkg, gpu):
    from clean_pvnet_amd import head
    d = twin.reference("odd_k")

    def call(g, m):
        return {"out": head.pvnet_head(*(g[k] for k in KEYS)), "u": head.upsample2x(g["fm"])}
    got = guarded_runs(gpu, "head odd_k", {k: d[k] for k in KEYS}, call, workspace=False)
    assert twin.same_bits(got["out"], d["out"]) and twin.same_bits(got["u"], d["u"])


def test_forward_bfloat16_over_partial_tiles(pkg, gpu):
    from clean_pvnet_amd import head
    d = twin.reference("reference_channels")

    def call(g, m):
        out = head.pvnet_head(*(g[k] for k in KEYS), out_dtype=torch.bfloat16)
        assert out.dtype == torch.bfloat16
        return {"out": out.view(torch.int16)}                                       # (numpy has no bfloat16: the same storage, as bits)
    got = guarded_runs(gpu, "head reference_channels bf16", {k: d[k] for k in KEYS}, call, workspace=False)
    assert got["out"].shape == d["out"].shape
    assert np.array_equal(_canon16(got["out"].view(np.uint16)), _canon16(twin.to_bf16(d["out"])))
