#!/usr/bin/env python
"""Generate tests/golden/train_*.npz by running THE REFERENCE'S OWN ``compute_vertex`` and ``NetworkWrapper`` on the CPU.

``lib/utils/pvnet/pvnet_data_utils.py`` is loaded where it lies under /root/reference with ``pycocotools``, ``plyfile`` and
``PIL`` stubbed where they are absent (``compute_vertex`` uses none of them).  ``lib/train/trainers/pvnet.py`` is loaded where
it lies with ``lib.utils.net_utils`` stubbed for its import only and ``sys.modules`` restored afterwards; its
``NetworkWrapper`` wraps a net that returns given tensors, and runs forward and backward in float32 and again in float64.
Nothing of the reference's program text enters the repository: the files hold data only.

Stored per case (tests/train_twin.py::GOLDEN_CASES): the case's sizes and seed -- the tests regenerate the predictions with
``train_twin.make_inputs`` and check them against ``vertex_pred_sum`` / ``seg_pred_sum`` -- the mask, the keypoints, ``target``
(the reference's ``compute_vertex`` per image, transposed as its loader does), and from the reference's wrapper ``vote_loss``,
``seg_loss``, ``vote_grad``, ``seg_grad`` in float32 and ``vote_loss64``, ``seg_loss64``, ``seg_grad64`` from the float64 run.

Run from the repository root in the build container:  python tests/golden/make_train_golden.py
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import train_twin as twin  # noqa: E402


class _Stub(types.ModuleType):
    """An empty module whose every name is None: enough for ``from plyfile import PlyData`` at import time."""

    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return None


def _load(name, path, stubs):
    """The module at ``path`` with the modules of ``stubs`` that cannot be imported replaced by empty ones for the import only."""
    saved = {}
    for stub in stubs:
        try:
            importlib.import_module(stub)
        except ImportError:
            saved[stub] = sys.modules.get(stub)
            sys.modules[stub] = _Stub(stub)
            parent, _, leaf = stub.rpartition(".")
            if parent:
                setattr(sys.modules[parent], leaf, sys.modules[stub])
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for stub, old in saved.items():
            if old is None:
                del sys.modules[stub]
            else:
                sys.modules[stub] = old
            parent, _, leaf = stub.rpartition(".")
            if parent and parent in sys.modules and leaf in vars(sys.modules[parent]):
                delattr(sys.modules[parent], leaf)
    return mod


def load_reference():
    data_utils = _load("ref_pvnet_data_utils", "lib/utils/pvnet/pvnet_data_utils.py",
                       ["pycocotools", "pycocotools.mask", "plyfile", "PIL", "PIL.Image"])
    trainer = _load("ref_pvnet_trainer", "lib/train/trainers/pvnet.py", ["lib.utils", "lib.utils.net_utils"])
    return data_utils.compute_vertex, trainer.NetworkWrapper


def run_wrapper(NetworkWrapper, d, target, dtype):
    import torch
    from torch import nn

    vp = torch.from_numpy(d["vertex_pred"]).to(dtype).requires_grad_(True)
    sp = torch.from_numpy(d["seg_pred"]).to(dtype).requires_grad_(True)

    class Given(nn.Module):
        def forward(self, inp):
            return {"vertex": vp, "seg": sp}

    batch = {"inp": torch.zeros(1), "mask": torch.from_numpy(d["mask"]), "vertex": torch.from_numpy(target).to(dtype), "meta": {}}
    _, loss, stats, _ = NetworkWrapper(Given())(batch)
    loss.backward()
    return (stats["vote_loss"].detach().numpy(), stats["seg_loss"].detach().numpy(), vp.grad.numpy(), sp.grad.numpy())


def case(name, compute_vertex, NetworkWrapper):
    B, K, C, H, W, seed, empty = twin.GOLDEN_CASES[name]
    d = twin.golden_inputs(name)
    target = np.stack([compute_vertex(d["mask"][b], d["kpt_2d"][b]).transpose(2, 0, 1) for b in range(B)])
    assert target.dtype == np.float32 and target.shape == (B, 2 * K, H, W)
    v32, s32, gv32, gs32 = run_wrapper(NetworkWrapper, d, target, __import__("torch").float32)
    v64, s64, _, gs64 = run_wrapper(NetworkWrapper, d, target, __import__("torch").float64)
    return {"sizes": np.array([B, K, C, H, W, seed], np.int32), "mask": d["mask"], "kpt_2d": d["kpt_2d"], "target": target,
            "vertex_pred_sum": d["vertex_pred"].astype(np.float64).sum(), "seg_pred_sum": d["seg_pred"].astype(np.float64).sum(),
            "vote_loss": np.float32(v32), "seg_loss": np.float32(s32), "vote_grad": gv32.astype(np.float32), "seg_grad": gs32.astype(np.float32),
            "vote_loss64": np.float64(v64), "seg_loss64": np.float64(s64), "seg_grad64": gs64.astype(np.float64)}


def main():
    compute_vertex, NetworkWrapper = load_reference()
    assert "lib.utils.net_utils" not in sys.modules
    for name in twin.GOLDEN_CASES:
        c = case(name, compute_vertex, NetworkWrapper)
        path = os.path.join(OUT, "train_%s.npz" % name)
        if os.path.exists(path) and "--force" not in sys.argv:       # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v), equal_nan=True) for k, v in c.items())
            print(name, "exists,", "identical content" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, {k: (v.shape if getattr(v, "shape", ()) else v) for k, v in c.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
