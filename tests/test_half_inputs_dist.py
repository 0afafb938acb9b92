"""CPU: a batch of 2-byte (float16 / bfloat16) vertex fields sharded with an uneven split.  The ranks that vote get float32
keypoints from the layer, so the ranks without an image must contribute float32 zero rows too: every rank enters the one
all_gather with the same dtype and byte count, and the gathered result is float32.  The GPU layer is stood in for by a
function that returns float32 keypoints, as the layer does for every field dtype."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K = 16, 16, 3


def _vote(mask, vertex, hn, **kw):
    """stand-in for ransac_voting_layer_v3: float32 [b,vn,2], whatever the vertex dtype"""
    assert vertex.shape[0] > 0, "sharded_vote must not call the layer on an empty shard"
    return vertex.float().mean((1, 2)) + 100.0 * torch.arange(vertex.shape[0]).view(-1, 1, 1)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_empty_half_shard_gives_float32_in_one_process(pkg, dt):
    from clean_pvnet_amd import dist as pdist
    out = pdist.sharded_vote(_vote, torch.zeros(0, H, W, dtype=torch.int64), torch.zeros(0, H, W, K, 2, dtype=dt), 0, 64)
    assert out.dtype == torch.float32 and tuple(out.shape) == (0, K, 2)
    out = pdist.sharded_vote(_vote, torch.zeros(0, H, W, dtype=torch.int64), torch.zeros(0, H, W, K, 2, dtype=dt), 0, 64, seed=3)
    assert out.dtype == torch.float32 and tuple(out.shape) == (0, K, 2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, batch, dt, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lib
        lib._register_clean_pvnet_amd()
        from clean_pvnet_amd import dist as pdist
        lo, hi = pdist.shard_bounds(batch, world, rank)
        g = torch.Generator().manual_seed(7)
        vertex = torch.randn(batch, H, W, K, 2, generator=g).to(dt)                  # the same batch on every rank
        mask = torch.ones(batch, H, W, dtype=torch.int64)
        out = pdist.sharded_vote(_vote, mask[lo:hi], vertex[lo:hi], batch, 64, seed=11)
        q.put((rank, str(out.dtype), out.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_gloo_uneven_split_of_a_half_batch(pkg, dt):
    """batch 3 on 4 ranks: rank 3 has no image (ceil(3/4) = 1 image per rank)"""
    batch, world = 3, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, batch, dt, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=120) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    g = torch.Generator().manual_seed(7)
    vertex = torch.randn(batch, H, W, K, 2, generator=g).to(dt)
    want = torch.cat([_vote(None, vertex[i:i + 1], 64) for i in range(batch)]).numpy()
    for rank, dtype, out in got:
        assert dtype == "torch.float32", (rank, dtype)
        assert (out == want).all(), rank
