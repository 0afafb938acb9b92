#!/usr/bin/env python
"""Generate tests/golden/optim_<kind>_<run>.npz by running the optimizers the fused step replaces, on the CPU: ``torch.optim.Adam``
and ``torch.optim.SGD(momentum=0.9)`` (``foreach=False``) and THE REFERENCE'S OWN ``RAdam``, loaded where it lies
(``lib/utils/optimizer/radam.py`` under the root given by ``--reference`` or the environment variable ``CLEAN_PVNET_REFERENCE``).
Nothing of the reference's program text enters the repository: the files hold data only.

Every parameter is a param group of its own with ``lr`` and ``weight_decay``, as the reference's ``make_optimizer`` groups them
(lib/train/optimizer.py:17-25), and ``clip_grad_value_(params, 40)`` runs before every step, as its trainer does
(lib/train/trainers/trainer.py:44).  Tensors, scales, seed and runs are tests/optim_twin.py's (``GOLDEN_*``): 12 steps; the runs
are weight decay 0, weight decay 5e-4, and weight decay 5e-4 with the learning rate halved by a ``MultiStepLR`` from step 8 on.

Stored per file: ``p0_sum`` / ``g_sum`` (binary64 sums of the regenerated draws, which the tests check instead of storing them),
``lr`` [12] as the scheduler set it, ``p32`` [12, N] the float32 trajectory of all parameters (flattened, in order) after every
step, ``m32`` / ``v32`` [N] the states at the last step (sgd: ``m32`` the momentum buffer, no ``v32``); for Adam and SGD the same
run with float64 parameters (the same float32 draws, widened): ``p64``, ``m64``, ``v64`` -- the reference's RAdam casts to float32 and
has no float64 form; for RAdam ``n_sma`` / ``step_size`` [12], what it buffered at every step.

Run from the repository root:  python tests/golden/make_optim_golden.py --reference <the reference's root>
"""
import argparse
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import optim_twin as twin  # noqa: E402


def _radam(ref):
    path = os.path.join(ref, "lib", "utils", "optimizer", "radam.py")
    spec = importlib.util.spec_from_file_location("_reference_radam", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RAdam


def run(kind, name, dtype, RAdam):
    import torch
    wd, halved = twin.GOLDEN_RUNS[name]
    p0, grads = twin.golden_draws()
    params = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in p0]
    groups = [{"params": [p], "lr": twin.GOLDEN_LR, "weight_decay": wd} for p in params]
    if kind == "adam":
        opt = torch.optim.Adam(groups, twin.GOLDEN_LR, weight_decay=wd, foreach=False)
    elif kind == "radam":
        opt = RAdam(groups, twin.GOLDEN_LR, weight_decay=wd)
    else:
        opt = torch.optim.SGD(groups, twin.GOLDEN_LR, momentum=0.9, foreach=False)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[twin.HALVED_AT - 1] if halved else [], gamma=0.5)
    traj, lrs, n_sma, step_size = [], [], [], []
    for t in range(1, twin.GOLDEN_STEPS + 1):
        for p, g in zip(params, grads[t - 1]):
            p.grad = torch.tensor(g, dtype=dtype)
        torch.nn.utils.clip_grad_value_(params, twin.GOLDEN_CLIP)
        lrs.append(opt.param_groups[0]["lr"])
        assert all(g["lr"] == lrs[-1] for g in opt.param_groups)
        opt.step()
        sched.step()
        traj.append(twin.flat([p.detach().numpy() for p in params]))
        if kind == "radam":
            buffered = opt.param_groups[0]["buffer"][t % 10]
            assert buffered[0] == t
            n_sma.append(buffered[1])
            step_size.append(buffered[2])
    names = ("momentum_buffer", None) if kind == "sgd" else ("exp_avg", "exp_avg_sq")
    m, v = (None if k is None else twin.flat([opt.state[p][k].numpy() for p in params]) for k in names)
    return {"p": np.stack(traj), "m": m, "v": v, "lr": np.asarray(lrs, np.float64), "n_sma": np.asarray(n_sma, np.float64),
            "step_size": np.asarray(step_size, np.float64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CLEAN_PVNET_REFERENCE"))
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit("make_optim_golden: give the reference's root with --reference or CLEAN_PVNET_REFERENCE")
    import torch
    warnings.simplefilter("ignore")
    RAdam = _radam(a.reference)
    p0, grads = twin.golden_draws()
    sums = {"p0_sum": np.float64(twin.flat(p0).astype(np.float64).sum()),
            "g_sum": np.float64(sum(twin.flat(g).astype(np.float64).sum() for g in grads))}
    assert any((np.abs(g[4]) > twin.GOLDEN_CLIP).any() for g in grads), "no gradient beyond the clip value"
    for kind in twin.KINDS:
        for name in twin.GOLDEN_RUNS:
            r32 = run(kind, name, torch.float32, RAdam)
            out = dict(sums, lr=r32["lr"], p32=r32["p"].astype(np.float32), m32=r32["m"].astype(np.float32))
            assert r32["p"].dtype == np.float32
            if kind != "sgd":
                out["v32"] = r32["v"].astype(np.float32)
            if kind == "radam":
                out["n_sma"], out["step_size"] = r32["n_sma"], r32["step_size"]
                first = int(np.argmax(out["n_sma"] >= 5)) + 1
                print("radam %s: N_sma >= 5 from step %d on" % (name, first))
            else:
                r64 = run(kind, name, torch.float64, RAdam)
                assert r64["p"].dtype == np.float64
                out["p64"], out["m64"] = r64["p"], r64["m"]
                if kind != "sgd":
                    out["v64"] = r64["v"]
            path = os.path.join(OUT, "optim_%s_%s.npz" % (kind, name))
            np.savez(path, **out)
            print("wrote %s (%d bytes)" % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
