"""The batch of tests/test_gpu_deferred_rows.py on poisoned, guarded memory (tests/guarded.py; ``guarded_runs`` of
tests/test_gpu_guarded.py): a v3 call counted in stages, whose first count launch gathers the rows of the staged images' rest chunks
itself.  Under the three fills no band of any arena changes, no input is written, and keypoints, winner counts and tn are the same
bytes every time and those of the unguarded full pass -- a deferred row read before it was written would be a fill's value, another
one per run."""
import pytest
import torch

from tests.test_gpu_deferred_rows import DEFERRED, H, HN, K, MAX_NUM, ROWS, SEED, W, _batch, _rows
from tests.test_gpu_guarded import _bits_equal, _shutdown, guarded_runs

pytestmark = pytest.mark.gpu


def test_staged_call_with_deferred_rows(pkg, gpu):
    from clean_pvnet_amd import ransac_voting as ext
    mask, vertex, _idxs = _batch()
    B = len(ROWS)

    def call(g, m):
        out, win, tn, ws = ext.ransac_voting_v3(g["mask"], g["vertex"], HN, 0.99, 5, MAX_NUM, None, None, SEED, ext.SINGULAR_ZERO,
                                                count_kernel=ext.COUNT_STAGED)
        assert ws.numel() == ext.workspace_bytes(B, H, W, K, HN, MAX_NUM, 8, ext.COUNT_STAGED, True)
        m.workspaces.append((ws.numel(), ws))
        torch.cuda.synchronize()
        assert _rows(ext, ws, (B, H, W, K, HN), ext.COUNT_STAGED, True, tn.cpu().tolist())[2] == list(DEFERRED)
        return {"out": out, "win": win, "tn": tn}
    got = guarded_runs(gpu, "v3 deferred rows", {"mask": mask, "vertex": vertex}, call, workspace="ext", before=_shutdown)
    _shutdown()
    full = ext.ransac_voting_v3(mask.to(gpu), vertex.to(gpu), HN, 0.99, 5, MAX_NUM, None, None, SEED, ext.SINGULAR_ZERO, count_kernel=ext.COUNT_FULL)
    for k, t in zip(("out", "win", "tn"), full[:3]):
        assert _bits_equal(got[k], t.cpu().numpy()), k
    _shutdown()
