#!/usr/bin/env python
"""Generate tests/golden/ct_train_*.npz by running THE REFERENCE'S OWN ``prepare_detection``, ``ct_collator`` and detector
``NetworkWrapper`` on the CPU.

The reference's files are loaded where they lie (its root is given by ``--reference`` or the environment variable
``CLEAN_PVNET_REFERENCE``), with the modules they import but do not use here stubbed for the import only and ``sys.modules``
restored afterwards: ``lib/utils/data_utils.py`` (``gaussian_radius``, ``draw_umich_gaussian``; ``cv2``, ``imgaug`` and
``lib.config`` stubbed), ``lib/datasets/tless_train/ct.py`` (``Dataset.prepare_detection``, which does not use ``self``;
``cv2``, ``pycocotools``, ``PIL`` and ``lib.utils.tless`` stubbed, ``lib.utils.data_utils`` the module above),
``lib/datasets/collate_batch.py`` (``ct_collator``), ``lib/utils/net_utils.py`` and ``lib/train/trainers/ct.py``
(``NetworkWrapper`` over a net that returns given tensors, forward and backward in float32 and again in float64).  If the
collator's uint8-mask indexing does not run on the installed torch, the padding is done here (zeros to the batch's largest
``ct_num``, the rows in order) and the script says so.  Nothing of the reference's program text enters the repository: the files
hold data only.

Stored per case (tests/ct_train_twin.py::GOLDEN_CASES): ``sizes`` and the seed -- the tests regenerate logits and wh predictions
with ``ct_train_twin.make_inputs`` and check them against ``ct_hm_pred_sum`` / ``wh_pred_sum`` -- the boxes, classes and counts;
the reference's ``ct_hm``, ``wh``, ``ct_cls``, ``ct_ind``, ``ct_01``, ``ct_num`` (padded to its own width ``width``) and the radii
its ``gaussian_radius`` gave; from its wrapper ``ct_loss``, ``wh_loss``, ``wh_grad`` in float32, ``ct_loss64``, ``wh_loss64`` and
``hm_grad64`` from the float64 run (the gradient rounded to float32 once where it has more than 2^14 elements, to keep the file
small).  The reference's own float32-float64 distances are measured here and stored: ``ct_loss_f32_dist``, ``wh_loss_f32_dist``
(absolute) and ``hm_grad_f32_ulps`` (the largest distance of its float32 gradient from its float64 one in float32 units).
Both gradients are those of the wrapper's ``loss = ct_loss + 0.1 * wh_loss``: the upstream gradient of ``wh_loss`` is float32(0.1).
``wh_grad_ulps`` is the largest distance between tests/ct_train_twin.py's wh gradient and torch's CPU autograd (0: bit for bit).

Only objects the contract keeps are handed to the reference (ct.py:91-92 drops the degenerate boxes itself; a class or a centre
outside the map is an indexing accident there), in their order.

Run from the repository root:  python tests/golden/make_ct_train_golden.py --reference <the reference's root>
"""
import argparse
import importlib
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

from tests import ct_train_twin as twin  # noqa: E402


class _Stub(types.ModuleType):
    """An empty module whose every name is None: enough for ``from cv2 import x`` or ``import cv2`` at import time."""

    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return None


def _load(ref, name, path, stubs, given=None):
    """The module at ``path`` with the modules of ``stubs`` that cannot be imported replaced by empty ones, and those of
    ``given`` by the modules handed in, for the import only."""
    saved, given = {}, dict(given or {})
    for stub in list(stubs) + list(given):
        if stub not in given:
            try:
                importlib.import_module(stub)
                continue
            except ImportError:
                pass
        saved[stub] = sys.modules.get(stub)
        sys.modules[stub] = given.get(stub) or _Stub(stub)
        parent, _, leaf = stub.rpartition(".")
        if parent:
            setattr(sys.modules[parent], leaf, sys.modules[stub])
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for stub, old in reversed(list(saved.items())):
            if old is None:
                del sys.modules[stub]
            else:
                sys.modules[stub] = old
            parent, _, leaf = stub.rpartition(".")
            if parent and parent in sys.modules and leaf in vars(sys.modules[parent]):
                delattr(sys.modules[parent], leaf)
    return mod


def load_reference(ref):
    data_utils = _load(ref, "ref_data_utils", "lib/utils/data_utils.py", ["cv2", "imgaug", "imgaug.augmenters", "lib.config"])
    dataset = _load(ref, "ref_tless_train_ct", "lib/datasets/tless_train/ct.py",
                    ["cv2", "pycocotools", "pycocotools.coco", "PIL", "PIL.Image", "lib.utils", "lib.utils.tless",
                     "lib.utils.tless.visualize_utils", "lib.utils.tless.tless_config", "lib.utils.tless.tless_train_utils"],
                    {"lib.utils.data_utils": data_utils})
    collate = _load(ref, "ref_collate_batch", "lib/datasets/collate_batch.py", [])
    net_utils = _load(ref, "ref_net_utils", "lib/utils/net_utils.py", [])
    trainer = _load(ref, "ref_ct_trainer", "lib/train/trainers/ct.py", ["lib.utils"], {"lib.utils.net_utils": net_utils})
    return data_utils, dataset.Dataset.prepare_detection, collate.ct_collator, trainer.NetworkWrapper


def run_targets(data_utils, prepare_detection, ct_collator, d, C, H, W):
    """The reference's targets of a batch, padded by its collator; (dict, the radii per image, how the padding was done)."""
    import math
    import torch
    B = d["cls"].shape[0]
    samples, radii = [], []
    for b in range(B):
        ct_hm = np.zeros([C, H, W], dtype=np.float32)
        wh, ct_cls, ct_ind, rad = [], [], [], []
        for n in range(int(d["num"][b])):
            if twin.one_object(d["boxes"][b, n], d["cls"][b, n], C, H, W) is None:
                continue
            box = [v.item() for v in np.asarray(d["boxes"][b, n]).astype(np.float64 if d["boxes"].dtype.kind == "f" else np.int64)]
            prepare_detection(None, box, ct_hm, int(d["cls"][b, n]), wh, ct_cls, ct_ind)
            rad.append(max(0, int(data_utils.gaussian_radius((math.ceil(box[3] - box[1]), math.ceil(box[2] - box[0]))))))
        samples.append({"inp": np.zeros(1, np.float32), "img": np.zeros(1, np.float32), "ct_hm": ct_hm, "wh": wh, "ct_cls": ct_cls,
                        "ct_ind": ct_ind, "meta": {"ct_num": len(ct_ind)}})
        radii.append(rad)
    how = "ct_collator"
    try:
        if max(len(s["ct_ind"]) for s in samples) == 0:
            raise RuntimeError("no object in the batch: the collator has nothing to index")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ret = ct_collator(samples)
        out = {k: ret[k].numpy() for k in ("ct_hm", "wh", "ct_cls", "ct_ind", "ct_01")}
        out["ct_num"] = ret["meta"]["ct_num"].numpy().astype(np.int64)
    except Exception as e:                                          # the padding of collate_batch.py:16-29, done here
        how = "padded in the script (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:80])
        width = max(1, max(len(s["ct_ind"]) for s in samples))
        out = {"ct_hm": np.stack([s["ct_hm"] for s in samples]), "wh": np.zeros((B, width, 2), np.float32),
               "ct_cls": np.zeros((B, width), np.int64), "ct_ind": np.zeros((B, width), np.int64), "ct_01": np.zeros((B, width), np.float32),
               "ct_num": np.array([len(s["ct_ind"]) for s in samples], np.int64)}
        for b, s in enumerate(samples):
            k = len(s["ct_ind"])
            if k:
                out["wh"][b, :k] = torch.Tensor(s["wh"]).numpy()
                out["ct_cls"][b, :k], out["ct_ind"][b, :k], out["ct_01"][b, :k] = s["ct_cls"], s["ct_ind"], 1
    return out, radii, how


def run_wrapper(NetworkWrapper, d, t, dtype):
    import torch
    from torch import nn

    hp = torch.from_numpy(d["ct_hm_pred"]).to(dtype).requires_grad_(True)
    wp = torch.from_numpy(d["wh_pred"]).to(dtype).requires_grad_(True)

    class Given(nn.Module):
        def forward(self, inp):
            return {"ct_hm": hp, "wh": wp}

    batch = {"inp": torch.zeros(1), "ct_hm": torch.from_numpy(t["ct_hm"]).to(dtype), "wh": torch.from_numpy(t["wh"]).to(dtype),
             "ct_ind": torch.from_numpy(t["ct_ind"]), "ct_01": torch.from_numpy(t["ct_01"]).to(dtype)}
    _, loss, stats, _ = NetworkWrapper(Given())(batch)
    assert list(stats) == ["ct_loss", "wh_loss", "loss"]
    loss.backward()
    return stats["ct_loss"].detach().numpy(), stats["wh_loss"].detach().numpy(), hp.grad.numpy(), wp.grad.numpy()


def case(name, ref):
    import torch
    data_utils, prepare_detection, ct_collator, NetworkWrapper = ref
    B, C, H, W, N, seed, kind, clamp, no_pos = twin.GOLDEN_CASES[name]
    d = twin.golden_inputs(name)
    t, radii, how = run_targets(data_utils, prepare_detection, ct_collator, d, C, H, W)
    width = t["ct_ind"].shape[1]
    radius = np.zeros((B, width), np.int64)
    for b, rad in enumerate(radii):
        radius[b, :len(rad)] = rad
    c32, w32, gh32, gw32 = run_wrapper(NetworkWrapper, d, t, torch.float32)
    c64, w64, gh64, gw64 = run_wrapper(NetworkWrapper, d, t, torch.float64)
    mine = twin.wh_grad(d["wh_pred"], t["wh"], t["ct_ind"], t["ct_01"], go=0.1)        # trainers/ct.py:26: loss += 0.1 * wh_loss
    out = {"sizes": np.array([B, C, H, W, N, seed], np.int32), "width": np.int64(width), "boxes": d["boxes"], "cls": d["cls"], "num": d["num"],
           "ct_hm_pred_sum": d["ct_hm_pred"].astype(np.float64).sum(), "wh_pred_sum": d["wh_pred"].astype(np.float64).sum(),
           "radius": radius, "ct_loss": np.float32(c32), "wh_loss": np.float32(w32), "wh_grad": gw32.astype(np.float32),
           "ct_loss64": np.float64(c64), "wh_loss64": np.float64(w64),
           "hm_grad64": gh64.astype(np.float64) if gh64.size <= 1 << 14 else gh64.astype(np.float32),
           "ct_loss_f32_dist": np.float64(abs(float(c32) - float(c64))), "wh_loss_f32_dist": np.float64(abs(float(w32) - float(w64))),
           "hm_grad_f32_ulps": np.int64(twin.ulp_apart(gh32, gh64.astype(np.float32)).max()),
           "wh_grad_ulps": np.int64(twin.ulp_apart(mine, gw32).max())}
    out.update(t)
    return out, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CLEAN_PVNET_REFERENCE"))
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit("make_ct_train_golden: give the reference's root with --reference or CLEAN_PVNET_REFERENCE")
    ref = load_reference(a.reference)
    assert "lib.utils.net_utils" not in sys.modules and "lib.utils" not in sys.modules
    for name in twin.GOLDEN_CASES:
        c, how = case(name, ref)
        print(name, "targets:", how, "| reference float32-float64: ct_loss %.3g, wh_loss %.3g, logit gradient %d ulps | twin wh gradient %d ulps from autograd"
              % (c["ct_loss_f32_dist"], c["wh_loss_f32_dist"], c["hm_grad_f32_ulps"], c["wh_grad_ulps"]))
        path = os.path.join(OUT, "ct_train_%s.npz" % name)
        if os.path.exists(path) and not a.force:                     # committed fixtures are not rewritten (zip metadata churn)
            old = dict(np.load(path))
            same = set(old) == set(c) and all(np.array_equal(np.asarray(old[k]), np.asarray(v), equal_nan=True) for k, v in c.items())
            print(name, "exists,", "identical content" if same else "CONTENT DIFFERS (run with --force to rewrite)")
            continue
        np.savez_compressed(path, **c)
        print(name, {k: (v.shape if getattr(v, "shape", ()) else v) for k, v in c.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
