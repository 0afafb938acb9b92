"""The fused optimizer step (include/pvnet_vote.h, "Optimizer step", clean_pvnet_amd.optim) without a GPU: the numpy twin of the
contract (tests/optim_twin.py) against the runs of the optimizers it replaces (tests/golden/optim_*.npz, made by
tests/golden/make_optim_golden.py from torch.optim.Adam, torch.optim.SGD and the reference's own RAdam), and the host side: the
table, the refusals, the ``state_dict`` interchange, the header and the symbols.  The GPU tests (tests/test_gpu_optim.py) then hold
the device to the twin byte for byte.

The bound is not a constant: per fixture D is the distance of the reference's own float32 run from its float64 run in the unit
U(i,t) of tests/optim_twin.py, and the twin has to lie within 2 D of both runs (RAdam has no float64 form: it is held to its
float32 run with the D of the Adam fixture of the same draws).  D itself has to be <= 8 U, or the fixture says nothing.
Measured (largest over the runs): Adam D 2.80, twin 3.58 from the float32 and 3.11 from the float64 run; SGD D 1.18, twin 1.82 and
1.38; RAdam twin 1.68 from its float32 run.  States at the last step in 2^-24 * 12 * max |state| per tensor: Adam m D 0.22, twin
0.27; v D 0.49, twin 0.40; SGD m D 0.49, twin 0.49; RAdam m 0.24, v 0.16."""
import os

import numpy as np
import pytest

from tests import capi
from tests import optim_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pvnet_vote.h")
SYMBOLS = {"pvv_optim_step", "pvv_optim_chunk"}
TITLE = "Optimizer step: the clipped Adam / RAdam / SGD step of every parameter tensor in one launch"
CASES = [(k, r) for k in twin.KINDS for r in twin.GOLDEN_RUNS]


@pytest.fixture(scope="module")
def optim(pkg):
    from clean_pvnet_amd import optim as o
    return o


@pytest.fixture(scope="module")
def runs():
    """{(kind, run): (fixture, twin p [T,N], twin m, twin v)}, computed once."""
    return {(k, r): (twin.load_golden(k, r), *twin.twin_run(k, r)) for k, r in CASES}


# ------------------------------------------------------------------------------------------------ 1. the twin against the fixtures
def test_fixtures_hold_what_the_issue_asks():
    p0, grads = twin.golden_draws()
    assert sum(a.size for a in p0) == 1503 and len(grads) == 12 and [a.shape for a in p0] == twin.GOLDEN_SHAPES
    over = [bool((np.abs(g[4]) > twin.GOLDEN_CLIP).any()) for g in grads]
    assert any(over) and (np.abs(twin.flat([g[4] for g in grads])) <= twin.GOLDEN_CLIP).any()       # clipped on some steps, in part
    sizes = [float(np.abs(twin.flat([g[i] for g in grads])).mean()) for i in range(len(p0))]
    assert min(sizes) < 2e-3 and max(sizes) > 50                                              # gradient scales 1e-3 ... 1e2
    for kind, run in CASES:
        g = twin.load_golden(kind, run)
        assert g["p0_sum"] == twin.flat(p0).astype(np.float64).sum()
        assert g["g_sum"] == sum(twin.flat(x).astype(np.float64).sum() for x in grads)
        assert g["lr"].tolist() == [twin.golden_lr(run, t) for t in range(1, 13)]
        assert g["p32"].dtype == np.float32 and g["p32"].shape == (12, 1503)
        assert os.path.getsize(os.path.join(twin.GOLDEN, "optim_%s_%s.npz" % (kind, run))) < 300 * 1024
    assert twin.load_golden("adam", "halved")["lr"][6:8].tolist() == [1e-3, 5e-4]


@pytest.mark.parametrize("run", list(twin.GOLDEN_RUNS))
def test_radam_scalars_equal_the_references_bit_for_bit(run, optim):
    g = twin.load_golden("radam", run)
    for own in (twin.radam_rectification, optim.radam_rectification):
        got = [own(t, 0.9, 0.999) for t in range(1, 13)]
        assert np.asarray([n for n, _ in got]).tobytes() == g["n_sma"].tobytes()
        assert np.asarray([s for _, s in got]).tobytes() == g["step_size"].tobytes()
    assert (g["n_sma"][:5] < 5).all() and (g["n_sma"][5:] >= 5).all()                         # both branches: the switch is at step 6


@pytest.mark.parametrize("kind,run", CASES)
def test_twin_lies_within_twice_the_references_own_distance(kind, run, runs):
    _, p, m, v = runs[(kind, run)]
    twin.assert_within_bound(kind, run, p, m, v)


def test_twin_edge_values():
    """What the device tests lean on: the clamp keeps a NaN and -0, +-Inf becomes +-c; subnormal second moments stay."""
    s, flags = twin.scalars("adam", 1, 1e-3)
    g = np.array([np.nan, np.inf, -np.inf, 40.0, -40.0, -0.0, 1e-20], np.float32)
    p, m, v = np.ones(7, np.float32), np.zeros(7, np.float32), np.zeros(7, np.float32)
    twin.step("adam", p, g, m, v, s, flags, clip=40.0)
    assert np.isnan(p[0]) and np.isfinite(p[1:]).all() and m[1] == m[3] and m[2] == m[4] and m[1] == -m[2]
    assert 0 < v[6] < np.finfo(np.float32).tiny and np.sqrt(v[6]) > 0                       # v is subnormal, not flushed
    assert np.signbit(m[5]) == False and g[1] == np.inf                                      # noqa: E712  (g keeps its values)
    twin.step("sgd", p, g, m, None, *twin.scalars("sgd", 1, 1e-3), clip=40.0, zero_grad=True)
    assert g.tobytes() == np.zeros(7, np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_table_chunk_counts_and_prefix(optim):
    C = optim.CHUNK
    assert C == twin.CHUNK and C % 1024 == 0
    numels = [1, 3, C - 1, C, C + 1, 2 * C + 3, 5]
    ptrs = [(16 * i + 1, 16 * i + 2, 16 * i + 3, 16 * i + 4) for i in range(len(numels))]
    sc = [optim.row_scalars("adam", i + 1, 1e-3 * (i + 1), 5e-4, (0.9, 0.999), 1e-8, 0.9) for i in range(len(numels))]
    rows, start = optim.build_table("adam", ptrs, numels, sc)
    assert start.dtype == np.int32 and start.tolist() == [0, 1, 2, 3, 4, 6, 9, 10] == twin.chunk_starts(numels).tolist()
    assert rows.dtype.itemsize == 80 and rows["numel"].tolist() == numels and rows["p"].tolist() == [p for p, _, _, _ in ptrs]
    assert rows["v"].tolist() == [v for _, _, _, v in ptrs] and not rows["reserved"].any()
    for i in range(len(numels)):
        s, flags = twin.scalars("adam", i + 1, 1e-3 * (i + 1), 5e-4)
        assert rows["s"][i].tobytes() == s.tobytes() and rows["flags"][i] == flags
    for kind in ("radam", "sgd"):
        for step in (1, 5, 6, 7):
            for wd in (0.0, 5e-4):
                s, flags = optim.row_scalars(kind, step, 2e-3, wd, (0.9, 0.999), 1e-8, 0.9)
                want, wflags = twin.scalars(kind, step, 2e-3, wd)
                assert np.asarray(s + (0,) * (8 - len(s)), np.float32).tobytes() == want.tobytes() and flags == wflags
    assert optim.row_scalars("radam", 1, 1e-3, 0.0, (0.9, 0.999), 1e-8, 0.9, degenerated_to_sgd=False)[1] == optim.ROW_NO_UPDATE
    rows, start = optim.build_table("sgd", [], [], [])
    assert len(rows) == 0 and start.tolist() == [0]
    with pytest.raises(ValueError, match="numel >= 1"):
        optim.build_table("sgd", [(1, 2, 3, 0)], [0], [((0, 0, 0), 0)])
    with pytest.raises(ValueError, match="2\\^31"):
        optim.build_table("sgd", [(1, 2, 3, 0)], [C * 2 ** 31], [((0, 0, 0), 0)])


def test_refusals_name_the_tensor(optim):
    import torch
    f = lambda *shape, **kw: torch.zeros(*shape, **kw)                                         # noqa: E731
    kw = dict(steps=1, lr=1e-3)
    ok = lambda: [f(3), f(2, 2)]                                                               # noqa: E731
    with pytest.raises(RuntimeError, match=r"CUDA tensor; there is no CPU fallback"):
        optim.optim_step("adam", ok(), ok(), ok(), ok(), **kw)
    with pytest.raises(RuntimeError, match=r"grads\[1\] must be float32, got torch.float64"):
        optim.optim_step("adam", ok(), [f(3), f(2, 2, dtype=torch.float64)], ok(), ok(), **kw)
    with pytest.raises(ValueError, match=r"exp_avg_sq\[0\] must have the shape of params\[0\], \(3,\), got \(4,\)"):
        optim.optim_step("adam", ok(), ok(), ok(), [f(4), f(2, 2)], **kw)
    with pytest.raises(ValueError, match=r"params\[1\] must be contiguous"):
        optim.optim_step("adam", [f(3), f(2, 2).t()], ok(), ok(), ok(), **kw)
    with pytest.raises(ValueError, match=r"exp_avg\[0\] must be contiguous"):
        optim.optim_step("sgd", [f(3)], [f(3)], [f(6)[::2]], **kw)
    with pytest.raises(RuntimeError, match=r"exp_avg\[1\] is on meta, params\[0\] on cpu"):
        optim.optim_step("adam", ok(), ok(), [f(3), f(2, 2, device="meta")], ok(), **kw)
    with pytest.raises(ValueError, match=r"grads has 1 tensors, params has 2"):
        optim.optim_step("adam", ok(), [f(3)], ok(), ok(), **kw)
    with pytest.raises(ValueError, match="kind must be one of"):
        optim.optim_step("adamw", ok(), ok(), ok(), ok(), **kw)
    with pytest.raises(ValueError, match="sgd takes no exp_avg_sq"):
        optim.optim_step("sgd", ok(), ok(), ok(), ok(), **kw)
    with pytest.raises(ValueError, match="adam needs exp_avg_sq"):
        optim.optim_step("adam", ok(), ok(), ok(), **kw)
    optim.optim_step("adam", [], [], [], [], **kw)                                             # nothing to do is not an error
    for cls in (optim.Adam, optim.RAdam, optim.SGD):
        with pytest.raises(ValueError, match="Invalid learning rate"):
            cls([f(3)], lr=-1.0)
        with pytest.raises(ValueError, match="Invalid clip_value"):
            cls([f(3)], lr=1e-3, clip_value=-1.0)
    with pytest.raises(ValueError, match="no dampening and no nesterov"):
        optim.SGD([f(3)], lr=1e-3, momentum=0.9, nesterov=True)


def _filled(opt, names, step):
    """Fill ``opt``'s state by hand (no step runs on the CPU): distinct values per parameter."""
    import torch
    for i, p in enumerate(p for g in opt.param_groups for p in g["params"]):
        for j, k in enumerate(names):
            opt.state[p][k] = torch.full_like(p, 10 * i + j + 1)
        if step is not None:
            opt.state[p]["step"] = step(i)


def test_state_dicts_go_both_ways(optim):
    import torch
    mk = lambda: [torch.zeros(3, requires_grad=True), torch.zeros(2, 2, requires_grad=True)]     # noqa: E731
    groups = lambda ps: [{"params": [p], "lr": 1e-3, "weight_decay": 5e-4} for p in ps]      # noqa: E731
    # Adam: ours -> torch -> ours
    ours = optim.Adam(groups(mk()), 1e-3, weight_decay=5e-4, clip_value=40.0)
    _filled(ours, ("exp_avg", "exp_avg_sq"), lambda i: 3 + i)
    step = ours.state_dict()["state"][1]["step"]
    assert isinstance(step, torch.Tensor) and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 4       # torch's form
    theirs = torch.optim.Adam(groups(mk()), 1e-3, weight_decay=5e-4, foreach=False)
    assert set(theirs.param_groups[0]) <= set(ours.param_groups[0])                          # every key torch's step reads
    theirs.load_state_dict(ours.state_dict())
    tp = [p for g in theirs.param_groups for p in g["params"]]
    assert float(theirs.state[tp[1]]["step"]) == 4 and theirs.state[tp[1]]["exp_avg_sq"].tolist() == [[12, 12], [12, 12]]
    for p in tp:
        p.grad = torch.ones_like(p)
    theirs.step()                                                                             # torch steps on what we saved
    assert float(theirs.state[tp[0]]["step"]) == 4 and float(theirs.state[tp[1]]["step"]) == 5
    back = optim.Adam(groups(mk()), 1e-3)
    back.load_state_dict(theirs.state_dict())
    bp = [p for g in back.param_groups for p in g["params"]]
    assert back.state[bp[1]]["step"] == 5 and type(back.state[bp[1]]["step"]) is int and back.param_groups[0]["weight_decay"] == 5e-4
    assert torch.equal(back.state[bp[0]]["exp_avg"], theirs.state[tp[0]]["exp_avg"])
    back.state[bp[0]]["step"] = torch.tensor(7.0)                                             # set by hand in torch's form: accepted
    assert back._state_of(bp[0], back.param_groups[0])[0] == 8 and back.state[bp[0]]["step"] == 8
    # SGD
    ours = optim.SGD(groups(mk()), 1e-3, momentum=0.9, clip_value=40.0)
    _filled(ours, ("momentum_buffer",), None)
    theirs = torch.optim.SGD(groups(mk()), 1e-3, momentum=0.9, foreach=False)
    assert set(theirs.param_groups[0]) <= set(ours.param_groups[0])
    theirs.load_state_dict(ours.state_dict())
    tp = [p for g in theirs.param_groups for p in g["params"]]
    assert theirs.state[tp[1]]["momentum_buffer"].tolist() == [[11, 11], [11, 11]] and theirs.param_groups[1]["weight_decay"] == 5e-4
    for p in tp:
        p.grad = torch.ones_like(p)
    theirs.step()
    back = optim.SGD(groups(mk()), 1e-3, momentum=0.9)
    back.load_state_dict(theirs.state_dict())
    bp = [p for g in back.param_groups for p in g["params"]]
    assert torch.equal(back.state[bp[1]]["momentum_buffer"], theirs.state[tp[1]]["momentum_buffer"])
    # RAdam: the layout of the reference's class -- lr, betas, eps, weight_decay, buffer in the groups; step an int
    ours = optim.RAdam(groups(mk()), 1e-3, weight_decay=5e-4, clip_value=40.0)
    _filled(ours, ("exp_avg", "exp_avg_sq"), lambda i: 3 + i)
    sd = ours.state_dict()
    assert set(sd["param_groups"][0]) == {"params", "lr", "betas", "eps", "weight_decay", "buffer"}
    assert len(sd["param_groups"][0]["buffer"]) == 10 and sd["param_groups"][0]["buffer"][0] == [None, None, None]
    assert sd["state"][1]["step"] == 4 and set(sd["state"][1]) == {"step", "exp_avg", "exp_avg_sq"}
    theirs_sd = {"state": {0: {"step": 9, "exp_avg": torch.ones(3), "exp_avg_sq": torch.ones(3)},
                           1: {"step": torch.tensor(9.0), "exp_avg": torch.ones(2, 2), "exp_avg_sq": torch.ones(2, 2)}},
                 "param_groups": [{"lr": 5e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "params": [i],
                                   "buffer": [[9, 100.0, 1.5]] + [[None, None, None] for _ in range(9)]} for i in range(2)]}
    back = optim.RAdam(groups(mk()), 1e-3)
    back.load_state_dict(theirs_sd)
    bp = [p for g in back.param_groups for p in g["params"]]
    assert [back.state[p]["step"] for p in bp] == [9, 9] and back.param_groups[0]["lr"] == 5e-4


def test_make_optimizer_groups_as_the_reference_does(optim):
    import types

    import torch
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 1))
    net[1].bias.requires_grad_(False)
    for name, cls in (("adam", optim.Adam), ("radam", optim.RAdam), ("sgd", optim.SGD)):
        cfg = types.SimpleNamespace(train=types.SimpleNamespace(optim=name, lr=1e-3, weight_decay=5e-4))
        opt = optim.make_optimizer(cfg, net)
        assert type(opt) is cls and isinstance(opt, torch.optim.Optimizer) and opt.clip_value == 40.0
        assert [len(g["params"]) for g in opt.param_groups] == [1, 1, 1]
        assert [g["params"][0] is p for g, p in zip(opt.param_groups, (net[0].weight, net[0].bias, net[1].weight))] == [True] * 3
        assert all(g["lr"] == 1e-3 and g["weight_decay"] == 5e-4 for g in opt.param_groups)
        if name == "sgd":
            assert all(g["momentum"] == 0.9 for g in opt.param_groups)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)       # a scheduler drives group['lr']
        assert opt.step() is None and not opt.state                                         # no gradient anywhere: nothing to do
        sched.step()
        assert all(g["lr"] == 5e-4 for g in opt.param_groups)


def test_header_declares_and_library_exports_the_entry_points(optim):
    raw = open(HEADER).read()
    assert SYMBOLS <= capi.declared()
    assert TITLE in raw and "#define PVV_ABI_VERSION 8" in raw                               # additive: the version did not move
    section = raw[raw.index(TITLE):raw.index("Model metadata (ABI v8")]
    for cite in ("lib/train/trainers/trainer.py:42-45", "lib/train/optimizer.py:12-27", "lib/utils/optimizer/radam.py:29-95"):
        assert cite in section
    assert "#define PVV_OPTIM_CHUNK %d" % optim.CHUNK in section
    for name, value in (("ADAM", 0), ("RADAM", 1), ("SGD", 2), ("CLIP", optim.CLIP), ("ZERO_GRAD", optim.ZERO_GRAD),
                        ("ROW_ADAPTIVE", optim.ROW_ADAPTIVE), ("ROW_DECAY", optim.ROW_DECAY), ("ROW_NO_UPDATE", optim.ROW_NO_UPDATE),
                        ("ROW_FIRST", optim.ROW_FIRST)):
        assert "#define PVV_OPTIM_%s %d\n" % (name, value) in section
    assert (optim.ROW_ADAPTIVE, optim.ROW_DECAY, optim.ROW_NO_UPDATE, optim.ROW_FIRST) == \
        (twin.ROW_ADAPTIVE, twin.ROW_DECAY, twin.ROW_NO_UPDATE, twin.ROW_FIRST)
    assert SYMBOLS <= capi.exported()
    assert optim._lib.pvv_optim_chunk() == optim.CHUNK
    import lib
    assert len(lib.load_build().HIP_LIBS) == 7                                              # part of libpvnet_vote.so: no new library


def test_entry_point_refuses_before_any_launch(optim):
    L = optim._lib
    err = lambda: L.pvv_last_error().decode()                                                  # noqa: E731
    assert L.pvv_optim_step(3, 256, 512, 1, 1, 0.0, 0, None) == -1 and "unknown kind" in err()
    assert L.pvv_optim_step(0, 256, 512, 1, 1, 0.0, 4, None) == -1 and "unknown bits" in err()
    assert L.pvv_optim_step(0, 256, 512, 2, 1, 0.0, 0, None) == -1 and "n_chunks" in err()
    assert L.pvv_optim_step(0, 256, 512, 1, 2 ** 31, 0.0, 0, None) == -1 and "2^31" in err()
    assert L.pvv_optim_step(0, 256, 512, 1, 1, -1.0, optim.CLIP, None) == -1 and "clip_value" in err()
    assert L.pvv_optim_step(0, 256, 512, 1, 1, float("nan"), optim.CLIP, None) == -1 and "clip_value" in err()
    assert L.pvv_optim_step(0, None, 512, 1, 1, 0.0, 0, None) == -1 and "NULL" in err()
    assert L.pvv_optim_step(0, 260, 512, 1, 1, 0.0, 0, None) == -1 and "aligned" in err()
    assert L.pvv_optim_step(0, None, None, 0, 0, 0.0, 0, None) == 0                            # nothing to do, nothing launched
