"""PVNet's decoder stages on poisoned, guarded memory (tests/guarded.py; ``guarded_runs`` of tests/test_gpu_guarded.py): under the
three fills no band of any arena changes, no input is written, the output lies in an arena and is the twin's -- the same bytes
every time -- and no workspace is asked for.  ``one_by_one`` is all border, ``odd_chunks`` has several halo chunks with a partial
last one and a partial tile, ``no_skip_same_res`` has no skip tensor, four row blocks with a partial last and a partial tile
along W."""
import pytest

from tests import decoder_twin as twin
from tests.test_gpu_guarded import guarded_runs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["one_by_one", "odd_chunks", "no_skip_same_res"])
def test_stage_on_guarded_memory(pkg, gpu, name):
    from clean_pvnet_amd import head
    d = twin.reference(name)

    def call(g, m):
        return {"out": head.pvnet_stage(*(g[k] for k in twin.KEYS), upsample=d["up"], negative_slope=d["slope"])}
    got = guarded_runs(gpu, "stage " + name, {k: d[k] for k in twin.KEYS}, call, workspace=False)
    assert twin.same_bits(got["out"], d["out"])
