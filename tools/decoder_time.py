#!/usr/bin/env python
"""``clean_pvnet_amd.head.pvnet_stage`` and ``PVNetDecoder`` at PVNet's own shapes -- a 480 x 640 image, the backbone's outputs at
1/8 (256 + 128 channels), 1/4 (64) and 1/2 (64) -- timed by tools/head_time.py's method: device events after warm-up (ms per
call, median, quartiles and range over the timed rounds; each round is ``--reps`` calls back to back), the legs alternated in
one process on the same inputs.  For each of ``conv8s``, ``conv4s``, ``conv2s`` and for the whole decoder (the three stages and
the head):

  fused     the float32 launch(es) of this package: one per stage, four for the decoder
  bf16      the stage with ``compute="bfloat16"``; the decoder with ``stage_compute="bfloat16", compute="bfloat16"``
  head_bf16 the decoder only: ``stage_compute="float32", compute="bfloat16"``, the fastest the float32 stages offer
  torch     the same function as the reference network runs it (lib/networks/pvnet/resnet18.py:31-59, 81-92): torch's own
            ``UpsamplingBilinear2d``, ``cat``, ``Conv2d``, ``BatchNorm2d`` in eval mode and ``LeakyReLU`` with their defaults
  autocast  ``torch`` under ``torch.autocast("cuda", torch.bfloat16)``: information

Before anything is timed the device's bytes are checked against the numpy twins: tests/decoder_twin.py bit for bit on three
stage cases and on the whole decoder at 16 x 24, tests/decoder_bf16_twin.py's bound on five; the run fails otherwise.  At the
first batch size max |fused - torch| of the decoder's output is printed: information, not a check, because MIOpen's order of
summation is not ours.  Three floors go with every stage:

  matrix        2 * 9 * C * M * H * W flop per image on ``v_mfma_f32_32x32x2_f32`` at the 155 TFLOP/s measured for that instruction
  matrix_bf16   the same flop on ``v_mfma_f32_32x32x16_bf16`` at 16 times that rate, 2.48 PFLOP/s: the instruction issues in 32
                cycles per SIMD against the float32 one's 64 and carries eight times the k
  bytes         the two inputs and the output once at the 6.29 TB/s measured for a copy

The bfloat16 stages are kept if at B = 32 the ``bf16`` decoder is faster than the ``head_bf16`` decoder by more than the
spread of the two: their inter-quartile ranges over the rounds do not overlap (``bf16_stages_kept`` in the decoder's record).

    python tools/decoder_time.py [--batches 1,32] [--rounds 20] [--warmup 3] [--reps 5] [--out profiles/decoder_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch import nn  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import head  # noqa: E402

MATRIX_F32 = 155e12                # measured rate of the f32-input MFMA
MATRIX_BF16 = 16 * MATRIX_F32      # v_mfma_f32_32x32x16_bf16: 32 cycles per SIMD for 8 times the k of the float32 one's 64
COPY_BYTES = 6.29e12               # measured HBM copy bandwidth
STAGES = ("conv8s", "conv4s", "conv2s")
FEATURES = ("x", "x2s", "x4s", "x8s", "xfc")
STAGE_LEGS = ("fused", "bf16", "torch", "autocast")
DECODER_LEGS = ("fused", "head_bf16", "bf16", "torch", "autocast")


def stage_shapes(H, W):
    """name -> (C2, C0, M, output height, output width, upsample)."""
    return {"conv8s": (256, 128, 128, H // 8, W // 8, False), "conv4s": (128, 64, 64, H // 4, W // 4, True),
            "conv2s": (64, 64, 32, H // 2, W // 2, True)}


def floors(B, C2, C0, M, Ho, Wo, up):
    flop = 2.0 * 9 * (C2 + C0) * M * Ho * Wo * B
    nbytes = 4.0 * B * (C2 * Ho * Wo / (4 if up else 1) + C0 * Ho * Wo + M * Ho * Wo)
    return flop, nbytes, flop / MATRIX_F32 * 1e3, nbytes / COPY_BYTES * 1e3


def make(B, H, W, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = head.PVNetDecoder(ver_dim=18, seg_dim=2).eval().requires_grad_(False)
    with torch.no_grad():
        for name in STAGES + ("convraw",):
            bn = getattr(m, name)[1]
            bn.weight.uniform_(0.5, 1.5, generator=g)
            bn.bias.normal_(generator=g)
            bn.running_mean.normal_(generator=g)
            bn.running_var.uniform_(0.5, 1.5, generator=g)
    shapes = {"x": (3, H, W), "x2s": (64, H // 2, W // 2), "x4s": (64, H // 4, W // 4), "x8s": (128, H // 8, W // 8),
              "xfc": (256, H // 8, W // 8)}
    return m.to(dev), {k: torch.randn(B, *s, generator=g).to(dev) for k, s in shapes.items()}


def torch_stage(m, up, name, a, skip):
    return getattr(m, name)(torch.cat([up(a) if name != "conv8s" else a, skip], 1))


def torch_decoder(m, up, f):
    fm = m.conv8s(torch.cat([f["xfc"], f["x8s"]], 1))
    fm = m.conv4s(torch.cat([up(fm), f["x4s"]], 1))
    fm = m.conv2s(torch.cat([up(fm), f["x2s"]], 1))
    return m.convraw(torch.cat([up(fm), f["x"]], 1))


def autocast(f, *args):
    with torch.autocast("cuda", torch.bfloat16):
        return f(*args)


def fused_stage(m, name, a, skip, compute="float32"):
    seq = getattr(m, name)
    scale, shift = m.folded(name)
    return head.pvnet_stage(a, skip, seq[0].weight, scale, shift, upsample=name != "conv8s", negative_slope=seq[2].negative_slope,
                            compute=compute)


def fused_decoder(m, f):
    out = m(*(f[k] for k in FEATURES))
    return out["seg"]._base


def check_against_the_twin(dev):
    """The device's bytes against the numpy twins: several halo chunks with a partial last one, one full tile of conv2s's
    channels, four row blocks without the upsample, and the whole decoder; the bfloat16 stage within its bound on those
    three, on a straddling group of channels and on the workgroups of four row blocks."""
    from tests import decoder_bf16_twin as bf16_twin
    from tests import decoder_twin as twin
    for name in ("odd_chunks", "stage_2s", "no_skip_same_res"):
        d = twin.reference(name)
        t = [torch.tensor(np.asarray(d[k]), device=dev) for k in twin.KEYS]
        got = head.pvnet_stage(*t, upsample=d["up"], negative_slope=d["slope"]).cpu().numpy()
        assert twin.same_bits(got, d["out"]), "the device differs from the twin on %s" % name
    d = twin.decoder_reference()
    m = head.PVNetDecoder.from_state_dict({k: torch.tensor(np.asarray(v)) for k, v in d["state"].items()}).to(dev).requires_grad_(False)
    out = m(*(torch.tensor(np.asarray(d[k]), device=dev) for k in FEATURES))
    assert twin.same_bits(torch.cat([out["seg"], out["vertex"]], 1).cpu().numpy(), d["out"]), "the decoder differs from its twin"
    print("device == twin, bit for bit (-0 as +0), on odd_chunks, stage_2s, no_skip_same_res and decoder_16x24", flush=True)
    shares = {}
    for name in ("odd_chunks", "stage_2s", "no_skip_same_res", "straddle", "wide_c16_up"):
        d = bf16_twin.reference(name)
        t = [torch.tensor(np.asarray(d[k]), device=dev) for k in bf16_twin.KEYS]
        got = head.pvnet_stage(*t, upsample=d["up"], negative_slope=d["slope"], compute="bfloat16").cpu().numpy()
        assert bf16_twin.within(got, d), "the bfloat16 stage leaves the twin's bound on %s" % name
        shares[name] = round(bf16_twin.worst(got, d), 3)
    print("bfloat16 stage within bound_acc; worst share per case: %s" % shares, flush=True)


def spread(ms, digits=4):
    """``summary`` with the quartiles: the acceptance compares inter-quartile ranges."""
    q1, q3 = np.percentile(np.asarray(ms), [25, 75])
    return dict(summary(ms, digits), q1=round(float(q1), digits), q3=round(float(q3), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls back to back inside one timed window")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    batches = [int(b) for b in a.batches.split(",")]
    for B in batches:
        for name, shape in stage_shapes(H, W).items():
            flop, nbytes, t_mat, t_mem = floors(B, *shape)
            print("B = %d, %s: %.2f GFLOP -> %.4f ms at the float32 matrix rate, %.4f ms at the bfloat16 one (%.2f PFLOP/s); "
                  "%.1f MB -> %.4f ms at the copy rate"
                  % (B, name, flop / 1e9, t_mat, flop / MATRIX_BF16 * 1e3, MATRIX_BF16 / 1e15, nbytes / 1e6, t_mem), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("decoder_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    up = nn.UpsamplingBilinear2d(scale_factor=2)
    lines = []
    with torch.no_grad():
        check_against_the_twin(dev)
        for B in batches:
            m, f = make(B, H, W, dev)
            decoders = {"fused": m, "head_bf16": head.PVNetDecoder.from_module(m, compute="bfloat16"),
                        "bf16": head.PVNetDecoder.from_module(m, compute="bfloat16", stage_compute="bfloat16")}
            ins = {"conv8s": (f["xfc"], f["x8s"])}                                  # every stage on its predecessor's fused output
            ins["conv4s"] = (fused_stage(m, "conv8s", *ins["conv8s"]), f["x4s"])
            ins["conv2s"] = (fused_stage(m, "conv4s", *ins["conv4s"]), f["x2s"])
            forms = {}

            def leg(f, *args):                                                      # (a form without parameters: not given the round)
                return lambda: [f(*args) for _ in range(a.reps)]
            for name in STAGES:
                forms["fused_" + name] = leg(fused_stage, m, name, *ins[name])
                forms["bf16_" + name] = leg(fused_stage, m, name, *ins[name], "bfloat16")
                forms["torch_" + name] = leg(torch_stage, m, up, name, *ins[name])
                forms["autocast_" + name] = leg(autocast, torch_stage, m, up, name, *ins[name])
            for which, dec in decoders.items():
                forms[which + "_decoder"] = leg(fused_decoder, dec, f)
            forms["torch_decoder"] = leg(torch_decoder, m, up, f)
            forms["autocast_decoder"] = leg(autocast, torch_decoder, m, up, f)
            diff = float((fused_decoder(m, f) - torch_decoder(m, up, f)).abs().max())
            diff_bf16 = float((fused_decoder(decoders["bf16"], f) - torch_decoder(m, up, f)).abs().max())
            print("B = %d: max |fused decoder - torch decoder| = %.3g, with bfloat16 stages and head %.3g (informational)"
                  % (B, diff, diff_bf16), flush=True)
            ms = alternate(forms, a.rounds, a.warmup)
            for name in STAGES + ("decoder",):
                res = {"B": B, "H": H, "W": W, "what": name, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps}
                for leg_name in (STAGE_LEGS if name in STAGES else DECODER_LEGS):
                    res[leg_name + "_ms"] = spread([v / a.reps for v in ms[leg_name + "_" + name]])
                med, med_bf16 = res["fused_ms"]["median"], res["bf16_ms"]["median"]
                res["torch_over_fused"] = round(res["torch_ms"]["median"] / med, 2)
                res["fused_over_bf16"] = round(med / med_bf16, 2)
                res["fused_round_spread"] = round(res["fused_ms"]["max"] / res["fused_ms"]["min"], 3)
                if name in STAGES:
                    C2, C0, M, Ho, Wo, ups = stage_shapes(H, W)[name]
                    flop, nbytes, t_mat, t_mem = floors(B, C2, C0, M, Ho, Wo, ups)
                    t_bf16 = flop / MATRIX_BF16 * 1e3
                    res.update({"C2": C2, "C0": C0, "M": M, "out_h": Ho, "out_w": Wo, "upsample": ups, "flop": flop, "bytes": nbytes,
                                "floor_matrix_ms": round(t_mat, 4), "floor_matrix_bf16_ms": round(t_bf16, 4),
                                "matrix_bf16_flops": MATRIX_BF16, "floor_bytes_ms": round(t_mem, 4),
                                "fused_tflops": round(flop / (med * 1e-3) / 1e12, 2), "fused_over_floor_matrix": round(med / t_mat, 2),
                                "fused_over_floor_bytes": round(med / t_mem, 2),
                                "bf16_tflops": round(flop / (med_bf16 * 1e-3) / 1e12, 2),
                                "bf16_over_floor_matrix_bf16": round(med_bf16 / t_bf16, 2),
                                "bf16_over_floor_bytes": round(med_bf16 / t_mem, 2)})
                else:
                    flop = sum(floors(B, *s)[0] for s in stage_shapes(H, W).values())
                    res["launches"] = 4
                    res["fused_vs_torch_max_abs"] = diff
                    res["bf16_vs_torch_max_abs"] = diff_bf16
                    res["stages_floor_matrix_ms"] = round(flop / MATRIX_F32 * 1e3, 4)
                    res["stages_floor_matrix_bf16_ms"] = round(flop / MATRIX_BF16 * 1e3, 4)
                    res["head_bf16_over_bf16"] = round(res["head_bf16_ms"]["median"] / med_bf16, 2)
                    res["bf16_stages_kept"] = bool(res["bf16_ms"]["q3"] < res["head_bf16_ms"]["q1"])   # faster, by more than the spread
                print(json.dumps(res), flush=True)
                lines.append(res)
            del m, f, ins, decoders, forms
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
