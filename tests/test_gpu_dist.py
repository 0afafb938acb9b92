"""The N > 1 path on the GPU box, as far as one GPU can show it: a real RCCL ("nccl") process group of ONE rank --
``bench.py`` launched the way the driver launches it for N > 1 (torch.distributed.run), and the HIP layer under
``clean_pvnet_amd.dist.sharded_vote`` compared with the un-sharded call.  (Two and more ranks: tests/test_dist.py on gloo.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _env():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RANK", None)
    return env


def test_bench_under_torchrun_one_rank_executes_the_rccl_exchange(gpu):
    """python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1: init_process_group("nccl"), an
    all_gather_into_tensor in EVERY step, barrier + max-over-ranks timing -- the N > 1 code path, one rank."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--batch", "4", "--rotate", "2", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=_env(), timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["scaling"] == "strong"           # (BASELINE config 3 read literally: the default since round 5)
    assert line["value_strong"] == line["value"] == line["value_weak"]                          # one GPU: the two modes are the same run
    assert line["extra"]["rccl_ranks"] == 1 and "all_gather" in line["extra"]["exchange"]
    assert line["config"]["global_batch"] == 4 and line["config"]["batch_per_gpu"] == 4
    assert line["value"] > 0 and line["extra"]["known_answer_max_err_px"] < 20
    assert len(line["extra"]["per_rank_count_kernel_ms"]) == 1 and line["roofline_contract_count_pass"]["kernel_ms_avg"] > 0
    assert line["roofline"]["bound"] == "valu_issue" and 0 < line["roofline_dense_equivalent"]["frac"]
    assert "in-place" in line["extra"]["exchange"] and line["extra"]["exchange_impl"].startswith("rccl")


_SHARDED = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, %r)
import lib; lib._register_clean_pvnet_amd()
from clean_pvnet_amd import dist as pdist, synth
from lib.csrc.ransac_voting.ransac_voting_gpu import ransac_voting_layer_v3, estimate_voting_distribution_with_mean
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
c = {**synth.CONFIGS["cfg1"], "B": 5}
d = synth.make_batch(**c, device=dev)
lo, hi = pdist.shard_bounds(5, dist.get_world_size(), dist.get_rank())
assert (lo, hi) == (0, 5)
got = pdist.sharded_vote(ransac_voting_layer_v3, d["mask"][lo:hi], d["vertex"][lo:hi], 5, c["hn"], inlier_thresh=0.99, seed=4242)
want = ransac_voting_layer_v3(d["mask"], d["vertex"], c["hn"], inlier_thresh=0.99, seed=4242)
# the shard split in two calls, as two ranks would make them, through the same collective
a = ransac_voting_layer_v3(d["mask"][:3], d["vertex"][:3], c["hn"], inlier_thresh=0.99, seed=4242, first_image=0)
b = ransac_voting_layer_v3(d["mask"][3:], d["vertex"][3:], c["hn"], inlier_thresh=0.99, seed=4242, first_image=3)
both = pdist.gather_results(torch.cat([a, b]), 5)
# an empty shard enters the collective too (a trailing rank of an uneven split)
empty = pdist.sharded_vote(ransac_voting_layer_v3, d["mask"][:0], d["vertex"][:0], 0, c["hn"], inlier_thresh=0.99, seed=1)
mean, cov = estimate_voting_distribution_with_mean(d["mask"], d["vertex"], want, seed=7)
cov_g = pdist.gather_results(cov, 5)
# round 5: RCCL's all-gather issued directly on the launch stream (clean_pvnet_amd/rccl.py), through the persistent gather buffer
from clean_pvnet_amd import rccl
comm = rccl.Comm.create(dev)
direct = dict(created=comm is not None, error=rccl.Comm.last_error)
if comm is not None:
    buf = pdist.GatherBuffer(5, (4, 2), dev, comm=comm)
    for rep in range(3):                                  # the buffer is reused step after step
        ransac_voting_layer_v3(d["mask"], d["vertex"], c["hn"], inlier_thresh=0.99, seed=4242, out=buf.mine)
        g = buf.gather()
    send = torch.arange(12., device=dev)
    recv = torch.zeros(12, device=dev)
    comm.all_gather_f32(send, recv)                       # not in place: one rank -> a copy
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                         # and on another stream: the current one is taken
        recv2 = torch.zeros(12, device=dev)
        comm.all_gather_f32(send, recv2)
    side.synchronize()
    torch.cuda.synchronize()
    direct.update(equal=bool(torch.equal(g, want)), copy=bool(torch.equal(recv, send)), copy2=bool(torch.equal(recv2, send)),
                  in_place=g.data_ptr() == buf.full.data_ptr())
    # the whole step -- voting kernels + the exchange -- captured into ONE HIP graph and replayed (stream order is the only
    # synchronisation of the direct call, so there is nothing a capture could not record)
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cs):
            ransac_voting_layer_v3(d["mask"], d["vertex"], c["hn"], inlier_thresh=0.99, seed=4242, out=buf.mine)
            gg = buf.gather()
        buf.full.zero_()
        graph.replay()
    torch.cuda.synchronize()
    direct.update(graph_equal=bool(torch.equal(gg, want)))
    comm.destroy()
torch.cuda.synchronize()
print(json.dumps(dict(equal=bool(torch.equal(got, want)), split_equal=bool(torch.equal(both, want)), shape=list(got.shape),
                      empty=list(empty.shape), cov_equal=bool(torch.equal(cov_g, cov)), backend=dist.get_backend(),
                      err=float((got - d["kpt_2d"]).abs().max()), direct=direct)))
dist.destroy_process_group()
""" % ROOT


def test_hip_layer_under_a_one_rank_nccl_group_equals_the_unsharded_call(gpu):
    env = dict(_env(), MASTER_PORT="29534")
    r = subprocess.run([sys.executable, "-c", _SHARDED], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, "no result line:\n%s\n%s" % (r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert res["backend"] == "nccl"
    assert res["equal"] and res["split_equal"] and res["cov_equal"]
    assert res["shape"] == [5, 4, 2] and res["empty"] == [0, 4, 2] and res["err"] < 10
    dr = res["direct"]                                            # the ctypes RCCL communicator on a one-rank group
    assert dr["created"], dr
    assert dr["equal"] and dr["copy"] and dr["copy2"] and dr["in_place"] and dr["graph_equal"]


# ---------------------------------------------------------------------------------------------------------------------
# A world of TWO ranks on the ONE GPU the box has.  RCCL refuses two ranks on one device, so the ranks
# exchange over gloo (clean_pvnet_amd.dist stages the 72 B/image results through the host); everything else -- shard
# bounds, the common RNG key, uneven and empty shards, padding inside gather_results, the HIP layer itself -- is the code
# an 8-GPU run executes.
# ---------------------------------------------------------------------------------------------------------------------
_TWO_RANKS = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, %r)
import lib; lib._register_clean_pvnet_amd()
from clean_pvnet_amd import dist as pdist, synth
from lib.csrc.ransac_voting.ransac_voting_gpu import ransac_voting_layer_v3, estimate_voting_distribution_with_mean
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dev = torch.device("cuda", 0)                      # both ranks on the one GPU
torch.cuda.set_device(dev)
dist.init_process_group("gloo", rank=rank, world_size=world)
res = {}
for name, batch, cfgname in (("b5", 5, "cfg1"), ("b1", 1, "cfg1"), ("b3_480x640", 3, "cfg2")):
    c = {**synth.CONFIGS[cfgname], "B": batch}
    hn = c["hn"]
    d = synth.make_batch(**c, device=dev)          # every rank can make the whole batch: images depend on their index only
    lo, hi = pdist.shard_bounds(batch, world, rank)
    got = pdist.sharded_vote(ransac_voting_layer_v3, d["mask"][lo:hi], d["vertex"][lo:hi], batch, hn, inlier_thresh=0.99, seed=4242)
    want = ransac_voting_layer_v3(d["mask"], d["vertex"], hn, inlier_thresh=0.99, seed=4242)       # unsharded HIP call
    mean, cov = estimate_voting_distribution_with_mean(d["mask"][lo:hi], d["vertex"][lo:hi], want[lo:hi], seed=7, first_image=lo)
    cov_all = pdist.gather_results(cov, batch)
    _m, cov_want = estimate_voting_distribution_with_mean(d["mask"], d["vertex"], want, seed=7)
    res[name] = dict(shard=[lo, hi], equal=bool(torch.equal(got, want)), cov_equal=bool(torch.equal(cov_all, cov_want)),
                     shape=list(got.shape), err=float((got - d["kpt_2d"]).abs().max()))
torch.cuda.synchronize()
out = json.dumps(dict(rank=rank, world=dist.get_world_size(), backend=dist.get_backend(), res=res))
open(os.path.join(os.environ["PVV_TEST_OUT"], "rank%%d.json" %% rank), "w").write(out)      # (one pipe for two ranks garbles lines)
dist.barrier()
dist.destroy_process_group()
""" % ROOT


def test_hip_layer_in_a_world_of_two_ranks_on_one_gpu_uneven_shards(gpu, tmp_path):
    """5 images / 2 ranks (3 + 2), 1 image / 2 ranks (1 + 0: the second rank enters the collective with zero rows) and
    3 full-size images (2 + 1): sharded HIP calls + gather == the unsharded HIP call, bit for bit, on every rank -- means
    from ransac_voting_layer_v3 and covariances from the estimate (device RNG keyed by the global image index)."""
    script = tmp_path / "two_ranks.py"
    script.write_text(_TWO_RANKS)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29535", str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(_env(), PVV_TEST_OUT=str(tmp_path)), timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in (0, 1)]
    assert sorted(x["rank"] for x in lines) == [0, 1]
    for x in lines:
        assert x["world"] == 2 and x["backend"] == "gloo"
        assert x["res"]["b5"]["shard"] == ([0, 3] if x["rank"] == 0 else [3, 5])
        assert x["res"]["b1"]["shard"] == ([0, 1] if x["rank"] == 0 else [1, 1])
        for name, shape in (("b5", [5, 4, 2]), ("b1", [1, 4, 2]), ("b3_480x640", [3, 9, 2])):
            q = x["res"][name]
            assert q["equal"] and q["cov_equal"] and q["shape"] == shape and q["err"] < 10, (name, q)


def test_bare_bench_gpus_2_launches_its_own_ranks(gpu):
    """`python bench.py --gpus 2 --steps 3` with NO launcher and no WORLD_SIZE (it used to die on an
    assertion): bench.py starts its ranks under torch.distributed.run itself.  On this 1-GPU box the two ranks share the
    device and exchange over gloo; strong scaling (the default) cuts the 5 images into shards of 3 + 2; the weak-scaling (5 per rank)
    and overlapped-exchange legs are included."""
    env = _env()
    for k in ("WORLD_SIZE", "LOCAL_RANK", "TORCHELASTIC_RUN_ID", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--batch", "5",
           "--rotate", "2", "--prewarm-ms", "20", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 prints, nobody else
    line = json.loads(lines[0])
    ex = line["extra"]
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "strong" and line["value"] > 0
    assert ex["shard_sizes"] == [3, 2] and ex["collective_ranks"] == 2 and ex["backend"] == "gloo"
    assert ex["oversubscribed_ranks_per_gpu"] == 2 and ex["rccl_ranks"] is None
    assert len(ex["per_rank_count_kernel_ms"]) == 2 and all(x > 0 for x in ex["per_rank_count_kernel_ms"])
    assert ex["known_answer_max_err_px"] < 20 and ex["weak_scaling_images_per_s"] > 0
    assert line["value_strong"] == line["value"] and line["value_weak"] == ex["weak_scaling_images_per_s"]
    assert "scaling_vs_n1_profile" in ex and line["cpu_baseline"] is None


def test_bare_bench_gpus_8_the_drivers_literal_command_on_one_gpu(gpu):
    """`python bench.py --gpus 8 --steps 20 --warmup 5` -- the driver's literal N = 8 command (VERDICT r5 #2a), plus --full for the per-rank figures -- with eight ranks
    sharing this box's one GPU: BASELINE config 3 read literally (64 images in shards of 8), every rank in the collective, the
    strong- and weak-scaling values at the top level, the multi_gpu block filled in, rc 0.  (Ranks sharing a device exchange over
    gloo -- RCCL refuses two ranks on one device; on the 8-GPU node the same lines run over RCCL.)"""
    env = _env()
    for k in ("WORLD_SIZE", "LOCAL_RANK", "TORCHELASTIC_RUN_ID", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "5", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    ex, mg = line["extra"], line["multi_gpu"]
    assert line["n_gpus"] == 8 and line["steps"] == 20 and line["warmup"] == 5 and line["scaling"] == "strong"
    assert ex["shard_sizes"] == [8] * 8 and ex["collective_ranks"] == 8
    assert line["config"]["global_batch"] == 64 and line["config"]["batch_per_gpu"] == 8
    assert line["value"] > 0 and line["value_strong"] == line["value"] and line["value_weak"] > 0
    assert mg["ranks"] == 8 and mg["shard_sizes"] == [8] * 8 and mg["collective_ranks"] == 8 and mg["backend"] == "gloo"
    assert mg["exchange_impl"] == "torch_distributed" and mg["oversubscribed_ranks_per_gpu"] == 8 and mg["rccl_ranks"] is None
    assert len(mg["per_rank_count_pass_ms"]) == 8 and all(x > 0 for x in mg["per_rank_count_pass_ms"])
    assert ex["known_answer_max_err_px"] < 20 and line["cpu_baseline"] is None
    assert line["metric"].startswith("images/sec RANSAC-vote")


@pytest.mark.parametrize("stage", ["load", "before_init", "inside_init"])
def test_bench_one_rank_rccl_group_survives_an_injected_communicator_fault(gpu, stage):
    """PVV_RCCL_FAULT=0:<stage> under a REAL one-rank RCCL group (the rehearsal hook of clean_pvnet_amd/rccl.py): the direct
    communicator is given up, the step's exchange goes through torch.distributed's collective, the line says why, rc 0."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(29537 + ["load", "before_init", "inside_init"].index(stage)), os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4", "--rotate", "2", "--full", "--no-cpu-baseline", "--no-sustained",
           "--no-side-legs", "--no-two-stream"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(_env(), PVV_RCCL_FAULT="0:" + stage), timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    mg = line["multi_gpu"]
    assert mg["exchange_impl"] == "torch_distributed" and "injected" in mg["exchange_fallback_reason"], mg
    assert mg["rccl_ranks"] == 1 and line["value"] > 0 and line["extra"]["known_answer_max_err_px"] < 20
