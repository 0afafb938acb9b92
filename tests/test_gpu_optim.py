"""The fused optimizer step on the MI355X (clean_pvnet_amd.optim) against the numpy twin (tests/optim_twin.py, itself held to the
optimizers it replaces in tests/test_optim.py): ``p``, ``m`` and ``v`` as bytes after each of 12 steps, for Adam, RAdam and SGD,
through ``optim_step`` and through the classes with a scheduler halving ``lr`` mid-run.

The shapes are the smallest that reach every path: numel 1, 3, 4, 5 (less than one 16-byte group, exactly one, one and a scalar
tail), CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 3 (a chunk's end, more than one block per tensor, a one-element last chunk), a
parameter that is ``base[1:]`` (4 bytes off: the scalar form), 300 tensors of 1-7 elements packed into one allocation (the table
lookup; a store past a tensor's end lands in its neighbour), an empty tensor and a parameter without a gradient in the middle."""
import numpy as np
import pytest

from tests import optim_twin as twin

pytestmark = pytest.mark.gpu
C = twin.CHUNK
KINDS = list(twin.KINDS)
SIZES = [1, 3, 4, 5, C - 1, C, 0, C + 1, 2 * C + 3, 1029]           # 0: an empty tensor in the middle; the last is base[1:]
VIEW = len(SIZES) - 1
CLIP = 40.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %d: %r != %r" % (
        what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _on(gpu, a, view=False):
    """``a`` on the device; with ``view`` as ``base[1:]`` of a one-longer allocation (its address is 4 bytes past a 16-byte line)."""
    import torch
    if not view:
        return torch.tensor(a, device=gpu)
    base = torch.zeros(a.size + 1, dtype=torch.float32, device=gpu)
    t = base[1:]
    t.copy_(torch.tensor(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _problem(seed=3):
    """Start values, states and 12 steps of gradients for SIZES, with the edge values the issue lists."""
    rng = np.random.default_rng(seed)
    n = len(SIZES)
    p = [(rng.standard_normal(s) * (1, 0.01)[i % 2]).astype(np.float32) for i, s in enumerate(SIZES)]
    first = [i % 3 for i in range(n)]                               # steps already taken: per-tensor step counts
    m = [(rng.standard_normal(s) * 0.1).astype(np.float32) if first[i] else np.zeros(s, np.float32) for i, s in enumerate(SIZES)]
    v = [(rng.standard_normal(s) ** 2 * 0.01).astype(np.float32) if first[i] else np.zeros(s, np.float32) for i, s in enumerate(SIZES)]
    scale = [1e-3, 1e-2, 1e2, 1e-1, 30, 1, 1, 1e-2, 10, 1]
    grads = []
    for t in range(12):
        g = [(rng.standard_normal(s) * scale[i]).astype(np.float32) for i, s in enumerate(SIZES)]
        g[3][:] = 1e-20                                             # v = 1e-43: lives in the subnormals for all 12 steps
        g[4][:8] = (40.0, -40.0, -0.0, 0.0, np.inf, -np.inf, 40.000004, -40.000004)
        if t >= 2:
            g[7][7] = np.nan                                        # that element only, from step 3 on
        g[8][C - 2:C + 2] = (np.inf, -np.inf, 41.0, -41.0)          # across a chunk boundary
        g[VIEW][-3:] = (np.inf, -0.0, -40.0)                        # in the scalar form
        grads.append(g)
    lr = [1e-3 * (1 + i % 4) for i in range(n)]
    wd = [(0.0, 5e-4, 1e-2)[i % 3] for i in range(n)]
    return p, m, v, grads, first, lr, wd


def _sgd_first(first, m):
    """sgd knows no step count: a tensor on its first step has no buffer yet; the kernel must not read what it is given."""
    return [np.full_like(a, np.nan) if f == 0 else a for a, f in zip(m, first)]


@pytest.mark.parametrize("kind", KINDS)
def test_optim_step_equals_the_twin_as_bytes(pkg, gpu, kind):
    from clean_pvnet_amd.optim import CHUNK, optim_step
    assert CHUNK == C
    p, m, v, grads, first, lr, wd = _problem()
    tp, tm, tv = [a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v]
    dm = _sgd_first(first, m) if kind == "sgd" else m
    dp, dm, dv = ([_on(gpu, a, i == VIEW) for i, a in enumerate(x)] for x in (p, dm, v))
    for t in range(12):
        steps = [f + t + 1 for f in first]
        lrs = [x * (0.5 if t >= 6 else 1.0) for x in lr]           # a scheduler halves every lr mid-run
        g = grads[t]
        dg = [_on(gpu, a, i == VIEW) for i, a in enumerate(g)]     # a new gradient tensor every step
        optim_step(kind, dp, dg, dm, None if kind == "sgd" else dv, steps=steps, lr=lrs, weight_decay=wd, clip_value=CLIP)
        twin.step_all(kind, tp, [a.copy() for a in g], tm, tv, steps, lrs, wd, clip=CLIP)
        for i in range(len(SIZES)):
            _same(dp[i], tp[i], "%s step %d p[%d]" % (kind, t + 1, i))
            _same(dm[i], tm[i], "%s step %d m[%d]" % (kind, t + 1, i))
            if kind != "sgd":
                _same(dv[i], tv[i], "%s step %d v[%d]" % (kind, t + 1, i))
            _same(dg[i], g[i], "%s step %d g[%d] (not written)" % (kind, t + 1, i))
    nan = np.isnan(tp[7])
    assert nan[7] and nan.sum() == 1 and not any(np.isnan(a).any() for i, a in enumerate(tp) if i != 7)      # the NaN stays in its element
    if kind != "sgd":
        assert 0 < tv[3].max() < np.finfo(np.float32).tiny         # the subnormal second moment was kept, on both sides


@pytest.mark.parametrize("kind", KINDS)
def test_three_hundred_small_tensors_in_one_allocation(pkg, gpu, kind):
    """The table lookup: 300 tensors of 1-7 elements, views of one packed buffer each for p, g, m, v, so every tensor's neighbour is
    another tensor and most start off a 16-byte line."""
    import torch
    from clean_pvnet_amd.optim import optim_step
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 8, 300)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    total = int(offs[-1])
    host = {k: rng.standard_normal(total).astype(np.float32) for k in "pgm"}
    host["v"] = (rng.standard_normal(total) ** 2).astype(np.float32)
    host["g"] *= 50                                                 # some beyond the clip value
    dev = {k: torch.tensor(a, device=gpu) for k, a in host.items()}
    cut = lambda x: [x[offs[i]:offs[i + 1]] for i in range(300)]    # noqa: E731
    steps = [2 + i % 9 for i in range(300)]                         # radam: both branches in one launch
    lr = [1e-3 * (1 + i % 5) for i in range(300)]
    wd = [(0.0, 5e-4)[i % 2] for i in range(300)]
    for _ in range(3):
        optim_step(kind, cut(dev["p"]), cut(dev["g"]), cut(dev["m"]), None if kind == "sgd" else cut(dev["v"]), steps=steps, lr=lr,
                   weight_decay=wd, clip_value=CLIP)
        twin.step_all(kind, cut(host["p"]), cut(host["g"]), cut(host["m"]), cut(host["v"]), steps, lr, wd, clip=CLIP)
        steps = [s + 1 for s in steps]
        for k in "pgmv":
            _same(dev[k], host[k], "%s packed %s" % (kind, k))


def _class_run(gpu, kind, zero_grad=False):
    """12 steps through the class with a MultiStepLR; returns the device's and the twin's (p, m, v) lists and the optimizer."""
    import torch
    from clean_pvnet_amd import optim
    p, _, _, grads, _, _, _ = _problem(seed=5)
    n = len(SIZES)
    params = [torch.nn.Parameter(_on(gpu, a, i == VIEW)) for i, a in enumerate(p)]
    frozen = torch.nn.Parameter(torch.ones(6, device=gpu))          # never gets a gradient: untouched, no state
    wd = [(0.0, 5e-4)[i % 2] for i in range(n)]
    groups = [{"params": [q], "lr": 1e-3, "weight_decay": w} for q, w in zip(params, wd)]
    groups.insert(4, {"params": [frozen], "lr": 1e-3, "weight_decay": 5e-4})
    cls = {"adam": optim.Adam, "radam": optim.RAdam, "sgd": optim.SGD}[kind]
    opt = cls(groups, 1e-3, momentum=0.9, clip_value=CLIP) if kind == "sgd" else cls(groups, 1e-3, clip_value=CLIP)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[6], gamma=0.5)
    tp = [a.copy() for a in p]
    tm, tv = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    count = [0] * n
    late = 2                                                        # this parameter gets its first gradient at step 4
    for t in range(12):
        lr = 1e-3 * (0.5 if t >= 6 else 1.0)
        assert all(g["lr"] == lr for g in opt.param_groups)
        tg = []
        for i, q in enumerate(params):
            if i == late and t < 3:
                q.grad = None
                tg.append(None)
                continue
            if t % 2 == 0 or q.grad is None:
                q.grad = _on(gpu, grads[t][i], i == VIEW)           # replaced by a new tensor, as after zero_grad(set_to_none=True)
            else:
                q.grad.copy_(torch.tensor(grads[t][i]))             # written in place, as after zero_grad(set_to_none=False)
            count[i] += 1
            tg.append(grads[t][i].copy())
        opt.step(zero_grad=zero_grad)
        sched.step()
        twin.step_all(kind, tp, tg, tm, tv, [max(c, 1) for c in count], lr, wd, clip=CLIP)
        for i, q in enumerate(params):
            _same(q, tp[i], "%s class step %d p[%d]" % (kind, t + 1, i))
            if zero_grad and q.grad is not None:
                assert not _bits(q.grad.cpu().numpy()).any(), "%s step %d: g[%d] is not all +0" % (kind, t + 1, i)
    return opt, params, frozen, tp, tm, tv, count


@pytest.mark.parametrize("kind", KINDS)
def test_classes_equal_the_twin_as_bytes(pkg, gpu, kind):
    import torch
    opt, params, frozen, tp, tm, tv, count = _class_run(gpu, kind)
    assert frozen not in opt.state and torch.equal(frozen, torch.ones_like(frozen))
    assert count[2] == 9 and count[0] == 12
    first, second = ("momentum_buffer", None) if kind == "sgd" else ("exp_avg", "exp_avg_sq")
    for i, q in enumerate(params):
        st = opt.state[q]
        assert set(st) == ({first} if kind == "sgd" else {"step", first, second})
        _same(st[first], tm[i], "%s %s[%d]" % (kind, first, i))
        if second:
            _same(st[second], tv[i], "%s %s[%d]" % (kind, second, i))
            assert int(st["step"]) == count[i]
            assert type(st["step"]) is int


@pytest.mark.parametrize("kind", KINDS)
def test_zero_grad_leaves_every_gradient_plus_zero(pkg, gpu, kind):
    _class_run(gpu, kind, zero_grad=True)                           # the same bytes for p, and g all +0 after every step


def test_reruns_from_equal_state_give_equal_bytes(pkg, gpu):
    from clean_pvnet_amd.optim import optim_step
    p, m, v, grads, first, lr, wd = _problem(seed=9)
    out = []
    for _ in range(3):
        dp, dg, dm, dv = ([_on(gpu, a, i == VIEW) for i, a in enumerate(x)] for x in (p, grads[0], m, v))
        for t in range(2):
            optim_step("adam", dp, dg, dm, dv, steps=[f + t + 1 for f in first], lr=lr, weight_decay=wd, clip_value=CLIP)
        out.append(b"".join(a.cpu().numpy().tobytes() for a in dp + dm + dv))
    assert out[0] == out[1] == out[2]


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_trajectories_hold_on_the_device(pkg, gpu, kind):
    """The reference's own runs (tests/golden/optim_*.npz): the device gives the twin's bytes, so the bound of tests/test_optim.py
    holds for it as well -- both are asserted."""
    import torch
    from clean_pvnet_amd.optim import optim_step

    def device_step(ps, gs, ms, vs, t, lr, wd):
        dp, dg, dm, dv = ([torch.tensor(a, device=gpu) for a in x] for x in (ps, gs, ms, vs))
        optim_step(kind, dp, dg, dm, None if kind == "sgd" else dv, steps=t, lr=lr, weight_decay=wd, clip_value=twin.GOLDEN_CLIP)
        return ([a.cpu().numpy() for a in x] for x in (dp, dm, dv))

    for run in twin.GOLDEN_RUNS:
        p, m, v = twin.twin_run(kind, run, device_step)
        tp, tm, tv = twin.twin_run(kind, run)
        _same(p, tp, "%s %s p" % (kind, run))
        _same(m, tm, "%s %s m" % (kind, run))
        _same(v, tv, "%s %s v" % (kind, run))
        twin.assert_within_bound(kind, run, p, m, v)


def test_refusals_on_the_device(pkg, gpu):
    import torch
    from clean_pvnet_amd.optim import optim_step
    a = lambda: [torch.zeros(4, device=gpu)]                        # noqa: E731
    with pytest.raises(RuntimeError, match=r"grads\[0\] is on cpu, params\[0\] on cuda:0"):
        optim_step("adam", a(), [torch.zeros(4)], a(), a(), steps=1, lr=1e-3)
    with pytest.raises(ValueError, match=r"steps\[0\] must be >= 1"):
        optim_step("adam", a(), a(), a(), a(), steps=0, lr=1e-3)
    with pytest.raises(ValueError, match="clip_value must be >= 0"):
        optim_step("adam", a(), a(), a(), a(), steps=1, lr=1e-3, clip_value=-1.0)
    with pytest.raises(ValueError, match="lr has 2 entries for 1 tensors"):
        optim_step("adam", a(), a(), a(), a(), steps=1, lr=[1e-3, 1e-3])
