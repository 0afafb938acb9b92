"""The timed loop and the summary of the ``*_time.py`` tools: forms alternated in one process on the same inputs, each call
bracketed by device events after a synchronisation."""
import inspect

import numpy as np
import torch


def alternate(forms, rounds, warmup, skip=None):
    """{name: [ms of each timed round]} for ``forms`` {name: callable}.  A form that takes an argument gets the round index;
    ``skip(name, i)`` leaves a form out of round ``i`` (warm-up rounds are ``i < warmup``)."""
    wants_round = {name: bool(inspect.signature(f).parameters) for name, f in forms.items()}
    ms = {name: [] for name in forms}
    for i in range(warmup + rounds):
        for name, f in forms.items():                                                      # alternated, same inputs
            if skip is not None and skip(name, i):
                continue
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            f(i) if wants_round[name] else f()
            e.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[name].append(s.elapsed_time(e))
    return ms


def summary(ms, digits):
    v = np.asarray(ms)
    return {"median": round(float(np.median(v)), digits), "min": round(float(v.min()), digits),
            "max": round(float(v.max()), digits)}
