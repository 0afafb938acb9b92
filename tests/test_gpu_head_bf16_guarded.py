"""The bfloat16 compute mode of the output head on poisoned, guarded memory (tests/guarded.py; ``guarded_runs`` of
tests/test_gpu_guarded.py): under the three fills no band of any arena changes, no input is written, the output lies in an arena,
is the same bytes every time and lies within the twin's ``bound_acc``, and no workspace is asked for.  ``odd_k`` is smaller than
one tile; ``reference_channels`` has partial last tiles in both axes and stores bfloat16, whose two-byte elements put the band right behind a half-written word."""
import numpy as np
import pytest
import torch

from tests import head_bf16_twin as twin
from tests import head_twin as ht
from tests.test_gpu_guarded import guarded_runs

pytestmark = pytest.mark.gpu
KEYS = twin.KEYS


def test_bfloat16_smaller_than_a_tile(pkg, gpu):
    from clean_pvnet_amd import head
    d = twin.reference("odd_k")

    def call(g, m):
        return {"out": head.pvnet_head(*(g[k] for k in KEYS), negative_slope=d["slope"], compute="bfloat16")}
    got = guarded_runs(gpu, "head odd_k bfloat16", {k: d[k] for k in KEYS}, call, workspace=False)
    assert twin.within(got["out"], d["bfloat16"], "bfloat16")


def test_bfloat16_store_over_partial_tiles(pkg, gpu):
    from clean_pvnet_amd import head
    d = twin.reference("reference_channels")
    ref = d["bfloat16"]

    def call(g, m):
        out = head.pvnet_head(*(g[k] for k in KEYS), negative_slope=d["slope"], out_dtype=torch.bfloat16, compute="bfloat16")
        assert out.dtype == torch.bfloat16
        return {"out": out.view(torch.int16)}                                       # (numpy has no bfloat16: the same storage, as bits)
    got = guarded_runs(gpu, "head reference_channels bfloat16, bf16 store", {k: d[k] for k in KEYS}, call, workspace=False)
    assert got["out"].shape == ref["out64"].shape
    stored = (got["out"].view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    f = np.isfinite(ref["out64"])
    bound = ref["bound_acc"][f] + ht.half_ulp(np.abs(ref["out64"][f]) + ref["bound_acc"][f], "bfloat16")    # the store's rounding
    assert (np.abs(stored[f] - ref["out64"][f]) <= bound).all()
    assert twin.nonfinite_sets_match(stored, ref["out64"], "bfloat16")
