"""The bfloat16 mode of PVNet's decoder stages on poisoned, guarded memory (tests/guarded.py; ``guarded_runs`` of
tests/test_gpu_guarded.py): under the three fills no band of any arena changes, no input is written, the output lies in an arena,
is the same bytes every time and lies within the twin's ``bound_acc``, and no workspace is asked for.  ``one_by_one`` is all
border; ``odd_chunks`` has several chunks of channels, a last one of one channel and a partial tile; ``no_skip_same_res`` has no
skip tensor (a NULL ``d_x``), a partial last row block and a partial tile along W; ``straddle`` has a group of eight channels
from both tensors and stores bfloat16, whose two-byte elements put the band right behind a half-written word; ``c33`` reads a
weight row's last channel alone."""
import pytest

from tests import decoder_bf16_twin as twin
from tests.test_gpu_guarded import guarded_runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["one_by_one", "odd_chunks", "no_skip_same_res", "c33"])
def test_stage_on_guarded_memory(pkg, gpu, name):
    from clean_pvnet_amd import head
    d = twin.reference(name)

    def call(g, m):
        return {"out": head.pvnet_stage(*(g[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"], compute="bfloat16")}
    got = guarded_runs(gpu, "bfloat16 stage " + name, {k: d[k] for k in twin.KEYS}, call, workspace=False)
    assert twin.within(got["out"], d)


def test_bfloat16_store_of_a_straddling_group_on_guarded_memory(pkg, gpu):
    import numpy as np
    import torch
    from clean_pvnet_amd import head
    d = twin.reference("straddle")

    def call(g, m):
        out = head.pvnet_stage(*(g[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"], compute="bfloat16",
                               out_dtype=torch.bfloat16)
        return {"out": out.view(torch.int16)}                                       # (numpy has no bfloat16: the same storage, as bits)
    got = guarded_runs(gpu, "bfloat16 stage straddle, bf16 store", {k: d[k] for k in twin.KEYS}, call, workspace=False)
    stored = (got["out"].view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert twin.within(stored, d, "bfloat16")
