"""The fused optimizer step on poisoned, guarded memory (tests/guarded.py).  ``guarded_runs`` asserts that no input is written, so
it cannot take an in-place call: ``Guarded`` is used directly, once per fill.  Every ``p``, ``g``, ``m``, ``v`` of a small mixed list
(numel 1, 5, CHUNK + 1, a ``base[1:]`` view, and a parameter without a gradient) lies in an arena of its own between two 512-byte
bands; after three steps no band may have changed (a 16-byte store past a tensor's end would), exactly the ``p``, ``m``, ``v`` arenas of
the stepped tensors were written (and ``g`` only under ``zero_grad``), and the results are the twin's bytes under every fill."""
import numpy as np
import pytest

from tests import optim_twin as twin
from tests.guarded import FILLS, Guarded

pytestmark = pytest.mark.gpu
SIZES = [1, 5, twin.CHUNK + 1, 1029, 6]          # [3] is base[1:] of a 1030-element arena, [4] never gets a gradient
VIEW, IDLE = 3, 4
STEPS0 = [0, 4, 5, 2, 3]                         # steps already taken: radam's two branches and sgd's first step are all there


def _host(kind):
    rng = np.random.default_rng(17)
    p = [rng.standard_normal(s).astype(np.float32) for s in SIZES]
    g = [(rng.standard_normal(s) * 30).astype(np.float32) for s in SIZES]
    m = [(rng.standard_normal(s) * 0.1).astype(np.float32) if c else np.zeros(s, np.float32) for s, c in zip(SIZES, STEPS0)]
    v = [(rng.standard_normal(s) ** 2).astype(np.float32) if c else np.zeros(s, np.float32) for s, c in zip(SIZES, STEPS0)]
    return p, g, m, v


def _run(gpu, kind, zero_grad, fill):
    """Three steps through the class under ``Guarded``: (bytes of every tensor afterwards, the mode, {arena index: name})."""
    import torch
    from clean_pvnet_amd import optim
    p, g, m, v = _host(kind)
    names = {}
    with Guarded(gpu, fill) as mode:
        def put(a, name, view):
            host = np.concatenate([np.float32([7]), a]) if view else a          # base[0] = 7 must stay
            t = mode.guarded_copy(torch.tensor(host))
            names[mode.arenas[-1].index] = name
            return t[1:] if view else t

        cols = {k: [put(a, "%s[%d]" % (k, i), i == VIEW) for i, a in enumerate(x)] for k, x in (("p", p), ("g", g), ("m", m), ("v", v))}
        assert cols["p"][VIEW].data_ptr() % 16 == 4
        groups = [{"params": [q], "lr": 1e-3 * (i + 1), "weight_decay": (0.0, 5e-4)[i % 2]} for i, q in enumerate(cols["p"])]
        if kind == "sgd":
            opt = optim.SGD(groups, 1e-3, momentum=0.9, clip_value=40.0)
        else:
            opt = {"adam": optim.Adam, "radam": optim.RAdam}[kind](groups, 1e-3, clip_value=40.0)
        for i, q in enumerate(cols["p"]):
            if kind == "sgd":
                if STEPS0[i]:
                    opt.state[q]["momentum_buffer"] = cols["m"][i]
            elif STEPS0[i]:
                step = torch.tensor(float(STEPS0[i])) if kind == "adam" else STEPS0[i]
                opt.state[q].update(step=step, exp_avg=cols["m"][i], exp_avg_sq=cols["v"][i])
            if i != IDLE:
                q.grad = cols["g"][i]
        for _ in range(3):
            opt.step(zero_grad=zero_grad)
        assert mode.check() == []                                                # no band around any tensor changed
        changed = sorted(names[a.index] for a in mode.inputs_changed())
        first = [q for i, q in enumerate(cols["p"]) if not STEPS0[i]][0]         # its state was made by the class: a factory arena
        made = opt.state[first]
        assert all(mode.owns(t) for t in made.values() if isinstance(t, torch.Tensor) and t.is_cuda)
        out = {k: [t.cpu().numpy() for t in ts] for k, ts in cols.items()}
        out["made"] = [made[k].cpu().numpy() for k in (("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq"))]
        base0 = [float(mode.arenas[i].tensor[0]) for i, nm in names.items() if nm.endswith("[%d]" % VIEW)]
    return out, changed, base0


@pytest.mark.parametrize("zero_grad", [False, True])
@pytest.mark.parametrize("kind", list(twin.KINDS))
def test_three_steps_on_guarded_memory(pkg, gpu, kind, zero_grad):
    p, g, m, v = _host(kind)
    wd = [(0.0, 5e-4)[i % 2] for i in range(len(SIZES))]
    lr = [1e-3 * (i + 1) for i in range(len(SIZES))]
    tg = [None if i == IDLE else a for i, a in enumerate(g)]
    for k in range(3):
        twin.step_all(kind, p, tg, m, v, [c + k + 1 for c in STEPS0], lr, wd, clip=40.0, zero_grad=zero_grad)
    stepped = [i for i in range(len(SIZES)) if i != IDLE]
    want_changed = ["p[%d]" % i for i in stepped]
    want_changed += ["m[%d]" % i for i in stepped if STEPS0[i]]                   # the others' states are the class's own tensors
    if kind != "sgd":
        want_changed += ["v[%d]" % i for i in stepped if STEPS0[i]]
    if zero_grad:
        want_changed += ["g[%d]" % i for i in stepped]
    results = []
    for fill in FILLS:
        out, changed, base0 = _run(gpu, kind, zero_grad, fill)
        assert changed == sorted(want_changed), (fill, changed)
        assert base0 == [7.0] * 4                                                # the element in front of the view
        for i in range(len(SIZES)):
            assert out["p"][i].tobytes() == p[i].tobytes(), (fill, "p", i)
            assert out["g"][i].tobytes() == g[i].tobytes(), (fill, "g", i)       # the twin zeroed its own when asked to
            if STEPS0[i]:
                assert out["m"][i].tobytes() == m[i].tobytes(), (fill, "m", i)
                if kind != "sgd":
                    assert out["v"][i].tobytes() == v[i].tobytes(), (fill, "v", i)
        assert out["made"][0].tobytes() == m[0].tobytes() and (kind == "sgd" or out["made"][1].tobytes() == v[0].tobytes())
        results.append(b"".join(a.tobytes() for k in ("p", "g", "m", "v", "made") for a in out[k]))
    assert results[0] == results[1] == results[2]
