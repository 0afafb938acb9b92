#!/usr/bin/env python
"""``clean_pvnet_amd.optim`` timed with device events after warm-up (ms per optimizer step, median and range over the timed rounds;
each round is ``--reps`` steps back to back), legs alternated in one process on the same gradients -> profiles/optim_time.json.

The tensors are the trainable parameters of PVNet's ResNet-18 for ``ver_dim = 18``, ``seg_dim = 2``, written out by hand from
lib/networks/pvnet/resnet.py and resnet18.py (``pvnet_shapes``): the reference is not needed.  Every parameter is a param group
of its own, as lib/train/optimizer.py:17-20 groups them, with lr 1e-3 and weight decay 5e-4; gradients are normal draws of scale
1 (a few beyond the clip value 40 are put in), the same for every leg, and no leg zeroes them unless it says so.

  (1) torch_adam            ``clip_grad_value_(params, 40)`` + ``torch.optim.Adam`` grouped per parameter, default implementation
  (2) torch_adam_fused      the same with ``fused=True``
  (3) torch_adam_one_group  one group, ``fused=True``: torch's best, not what the reference does
  (4) torch_radam_ops       ``clip_grad_value_`` + the reference's RAdam restated in torch ops (``TorchRAdam`` below), per parameter
  (5) ours_<kind>[_zero]    ``Adam`` / ``RAdam`` / ``SGD`` of this package with ``clip_value=40``, without and with ``zero_grad``

Before anything is timed the device's bytes are compared with the twin's (tests/optim_twin.py) on the same tensors for two steps
of every kind.  ``*_gbps`` is bytes moved per second -- p, g, m, v read and p, m, v written: 28 bytes per element (sgd: 20), 4 more
with ``zero_grad`` -- against the 6.3 TB/s measured-copy ceiling (``*_of_ceiling``).  The baseline is (1) and (2), never the code
under test.  No time is a pass criterion anywhere; this is for whoever has the card.

    python tools/optim_time.py [--rounds 20] [--warmup 3] [--reps 3] [--out profiles/optim_time.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import optim  # noqa: E402
from tests import optim_twin as twin  # noqa: E402

CEILING_GBPS = 6300.0
CLIP = 40.0


def pvnet_shapes(ver_dim=18, seg_dim=2):
    """The shapes of ``Resnet18(ver_dim, seg_dim).parameters()`` in order: a convolution without bias is one tensor, a batch norm
    two (weight, bias)."""
    out = []

    def conv_bn(cout, cin, k):
        out.extend([(cout, cin, k, k), (cout,), (cout,)])

    conv_bn(64, 3, 7)                                               # conv1, bn1
    inplanes = 64
    for planes in (64, 128, 256, 512):                              # layer1..layer4, two BasicBlocks each
        for block in range(2):
            conv_bn(planes, inplanes, 3)
            conv_bn(planes, planes, 3)
            if block == 0 and planes != inplanes:
                conv_bn(planes, inplanes, 1)                        # downsample
            inplanes = planes
    conv_bn(256, 512, 3)                                            # fc, replaced by a 3x3 convolution (fcdim = 256)
    conv_bn(128, 128 + 256, 3)                                      # conv8s
    conv_bn(64, 64 + 128, 3)                                        # conv4s
    conv_bn(32, 64 + 64, 3)                                         # conv2s
    conv_bn(32, 3 + 32, 3)                                          # convraw
    out.extend([(seg_dim + ver_dim, 32, 1, 1), (seg_dim + ver_dim,)])
    return out


class TorchRAdam(torch.optim.Optimizer):
    """The reference's RAdam (lib/utils/optimizer/radam.py:29-95, degenerated_to_sgd=True) restated in torch ops for float32
    parameters: what leg (4) times."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad, value = p.grad.float(), p.float()              # its two full-size float copies
                state = self.state[p]
                if not state:
                    state.update(step=0, exp_avg=torch.zeros_like(value), exp_avg_sq=torch.zeros_like(value))
                state["step"] += 1
                m, v = state["exp_avg"], state["exp_avg_sq"]
                v.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                m.mul_(beta1).add_(grad, alpha=1 - beta1)
                n_sma, size = optim.radam_rectification(state["step"], beta1, beta2)
                if group["weight_decay"] != 0:
                    value.add_(value, alpha=-group["weight_decay"] * group["lr"])
                if n_sma >= 5:
                    value.addcdiv_(m, v.sqrt().add_(group["eps"]), value=-size * group["lr"])
                else:
                    value.add_(m, alpha=-size * group["lr"])
                p.copy_(value)


def check_against_twin(shapes, dev):
    """Two steps of every kind on the real shapes: the device's bytes are the twin's."""
    rng = np.random.default_rng(1)
    for kind in twin.KINDS:
        hp = [rng.standard_normal(s).astype(np.float32) * 0.05 for s in shapes]
        hm, hv = [np.zeros_like(a) for a in hp], [np.zeros_like(a) for a in hp]
        dp, dm, dv = ([torch.tensor(a, device=dev) for a in x] for x in (hp, hm, hv))
        for step in (1, 2):
            hg = [rng.standard_normal(s).astype(np.float32) * 30 for s in shapes]
            dg = [torch.tensor(a, device=dev) for a in hg]
            optim.optim_step(kind, dp, dg, dm, None if kind == "sgd" else dv, steps=step, lr=1e-3, weight_decay=5e-4, clip_value=CLIP)
            twin.step_all(kind, hp, hg, hm, hv, step, 1e-3, 5e-4, clip=CLIP)
        for name, d, h in (("p", dp, hp), ("m", dm, hm), ("v", dv, hv)):
            for i, (a, b) in enumerate(zip(d, h)):
                assert a.cpu().numpy().tobytes() == b.tobytes(), "%s: %s[%d] differs from the twin" % (kind, name, i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="steps back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    shapes = pvnet_shapes()
    elements = sum(math.prod(s) for s in shapes)
    check_against_twin(shapes, dev)

    g = torch.Generator(device="cpu").manual_seed(7)
    start = [(torch.randn(s, generator=g) * 0.05).to(dev) for s in shapes]
    grads = [torch.randn(s, generator=g).to(dev) for s in shapes]
    grads[0].view(-1)[:8] = 100.0                                   # beyond the clip value

    def leg(make, **step_kw):
        params = [torch.nn.Parameter(t.clone()) for t in start]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt = make(params)
        clip = not isinstance(opt, optim._Fused)

        def run():
            for _ in range(a.reps):
                if clip:
                    torch.nn.utils.clip_grad_value_(params, CLIP)
                opt.step(**step_kw)
        return run

    per = lambda ps: [{"params": [p], "lr": 1e-3, "weight_decay": 5e-4} for p in ps]           # noqa: E731
    baselines = {
        "torch_adam": leg(lambda ps: torch.optim.Adam(per(ps), 1e-3, weight_decay=5e-4)),
        "torch_adam_fused": leg(lambda ps: torch.optim.Adam(per(ps), 1e-3, weight_decay=5e-4, fused=True)),
        "torch_adam_one_group": leg(lambda ps: torch.optim.Adam(ps, 1e-3, weight_decay=5e-4, fused=True)),
        "torch_radam_ops": leg(lambda ps: TorchRAdam(per(ps), 1e-3, weight_decay=5e-4)),
    }
    ours = {"adam": lambda ps: optim.Adam(per(ps), 1e-3, weight_decay=5e-4, clip_value=CLIP),
            "radam": lambda ps: optim.RAdam(per(ps), 1e-3, weight_decay=5e-4, clip_value=CLIP),
            "sgd": lambda ps: optim.SGD(per(ps), 1e-3, momentum=0.9, clip_value=CLIP)}
    forms = {}
    for kind, make in ours.items():
        forms["ours_" + kind] = leg(make)
        forms["ours_%s_zero" % kind] = leg(make, zero_grad=True)
    forms.update(baselines)         # the leg after torch_radam_ops has measured slower and wider (ours_adam follows it across rounds)
    ms = alternate(forms, a.rounds, a.warmup)
    res = {"tensors": len(shapes), "elements": elements, "largest": max(math.prod(s) for s in shapes), "chunk": optim.CHUNK,
           "chunks": int(sum(-(-math.prod(s) // optim.CHUNK) for s in shapes)), "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "twin_bytes_equal": True}
    for name in forms:
        res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
    for kind in ours:
        for tail, extra in (("", 0), ("_zero", 4)):
            moved = elements * ((20 if kind == "sgd" else 28) + extra)
            gbps = moved / (res["ours_%s%s_ms" % (kind, tail)]["median"] * 1e-3) / 1e9
            res["ours_%s%s_gbps" % (kind, tail)] = round(gbps, 1)
            res["ours_%s%s_of_ceiling" % (kind, tail)] = round(gbps / CEILING_GBPS, 3)
    res["adam_speedup_over_torch"] = round(res["torch_adam_ms"]["median"] / res["ours_adam_ms"]["median"], 2)
    res["adam_speedup_over_torch_fused"] = round(res["torch_adam_fused_ms"]["median"] / res["ours_adam_ms"]["median"], 2)
    res["adam_speedup_over_torch_one_group"] = round(res["torch_adam_one_group_ms"]["median"] / res["ours_adam_ms"]["median"], 2)
    res["radam_speedup_over_torch_ops"] = round(res["torch_radam_ops_ms"]["median"] / res["ours_radam_ms"]["median"], 2)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([res], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
