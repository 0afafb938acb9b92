#!/usr/bin/env python
"""``clean_pvnet_amd.head.pvnet_head`` at PVNet's own shapes -- 480 x 640, C2 = 32 feature and C0 = 3 image channels, M1 = 32,
M2 = 20 (18 vertex + 2 segmentation channels) -- timed with device events after warm-up (ms per call, median and range over the
timed rounds; each round is ``--reps`` calls back to back), alternated in one process on the same inputs with

  torch    the same function as the reference network runs it (lib/networks/pvnet/resnet18.py:53-59, 90-92), six map-sized ops:
           ``UpsamplingBilinear2d``, ``cat``, ``Conv2d`` 3 x 3, ``BatchNorm2d`` in eval mode, ``LeakyReLU``, ``Conv2d`` 1 x 1 --
           torch's own modules with their defaults, nothing tuned down; followed by a cast for a half-precision output.
  bfloat16         the same fused call with ``compute="bfloat16"``, the matrix-core mode (``PVV_HEAD_COMPUTE_BF16``)
  torch_autocast   the torch chain under ``torch.autocast("cuda", torch.bfloat16)``: information only

The acceptance of the mode is read off the float32 output at B = 32, medians of one run: ``bfloat16`` at least 1.5 x faster than the
``fused`` (float32) leg of that run.  At the first batch size the keypoints ``decode_keypoint`` finds from the mode's output are
compared with those from the float32 head's: the largest and median distance in pixels, information only.

Before anything is timed the device's bytes are checked against the numpy twin (tests/head_twin.py) at a small shape, and the
bfloat16 mode against its twin's bound (tests/head_bf16_twin.py); the run fails otherwise.  At the first batch size max |fused - torch chain| is printed: information, not a check, because MIOpen's choice
of algorithm -- and so its order of summation -- is not ours.  Two floors are reported with every time:

  matrix   (316 * 32 + 32 * 32) * 2 * H * W flop per image on ``v_mfma_f32_32x32x2_f32`` (K = 315 padded to even, M2 to one 32-row
           block) at the 155 TFLOP/s measured for that instruction
  bytes    fm + image + output at the 6.29 TB/s measured for a copy

    python tools/head_time.py [--batches 1,32] [--rounds 20] [--warmup 3] [--reps 10] [--out profiles/head_time.json]
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
MODES = ("bfloat16",)
COPY_BYTES = 6.29e12               # measured HBM copy bandwidth
C2, C0, M1, M2 = 32, 3, 32, 20


def floors(B, H, W, out_dtype):
    flop = (316 * 32 + 32 * 32) * 2.0 * H * W * B
    item = 4 if out_dtype == torch.float32 else 2
    nbytes = B * (4 * C2 * (H // 2) * (W // 2) + 4 * C0 * H * W + item * M2 * H * W)
    return flop, nbytes, flop / MATRIX_F32 * 1e3, nbytes / COPY_BYTES * 1e3


def make(B, H, W, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = head.PVNetHead(ver_dim=M2 - 2, seg_dim=2, s2dim=C2, raw_dim=M1, image_dim=C0).eval().requires_grad_(False)
    with torch.no_grad():
        bn = m.convraw[1]
        bn.weight.uniform_(0.5, 1.5, generator=g)
        bn.bias.normal_(generator=g)
        bn.running_mean.normal_(generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    m = m.to(dev)
    fm = torch.randn(B, C2, H // 2, W // 2, generator=g).to(dev)
    x = torch.randn(B, C0, H, W, generator=g).to(dev)
    return m, fm, x, nn.UpsamplingBilinear2d(scale_factor=2)


def torch_chain(m, up, fm, x, out_dtype):
    out = m.convraw(torch.cat([up(fm), x], 1))
    return out if out_dtype == torch.float32 else out.to(out_dtype)


def torch_autocast(m, up, fm, x, out_dtype):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m.convraw(torch.cat([up(fm), x], 1))
    return out.to(out_dtype)


def fused(m, fm, x, out_dtype, compute="float32"):
    c = m.convraw
    scale, shift = m.folded()
    return head.pvnet_head(fm, x, c[0].weight, scale, shift, c[3].weight, c[3].bias, negative_slope=c[2].negative_slope,
                           out_dtype=out_dtype, compute=compute)


def keypoint_shift(m, fm, x):
    """{mode: (largest, median)} |keypoint(mode's head) - keypoint(float32 head)| in pixels through ``decode_keypoint``, same seed."""
    from clean_pvnet_amd.decode import decode_keypoint

    def keypoints(compute):
        out = fused(m, fm, x, torch.float32, compute)
        return decode_keypoint({"seg": out[:, :2], "vertex": out[:, 2:]}, seed=5)["kpt_2d"].double()
    base = keypoints("float32")
    shifts = {}
    for mode in MODES:
        dist = (keypoints(mode) - base).norm(dim=-1).flatten()
        dist = dist[torch.isfinite(dist)]
        shifts[mode] = (float(dist.max()), float(dist.median())) if dist.numel() else (float("nan"), float("nan"))
    return shifts


def check_against_the_twin(dev):
    """The device's bytes against the numpy twin on its two cases with PVNet's channel counts and with two row blocks."""
    from tests import head_twin as twin
    for name in ("reference_channels", "two_blocks"):
        d = twin.reference(name)
        t = [torch.tensor(np.asarray(d[k]), device=dev) for k in ("fm", "x", "weight1", "scale", "shift", "weight2", "bias2")]
        got = head.pvnet_head(*t).cpu().numpy()
        assert twin.same_bits(got, d["out"]), "the device differs from the twin on %s" % name
        half = head.pvnet_head(*t, out_dtype=torch.bfloat16).view(torch.int16).cpu().numpy()
        assert half.tobytes() == twin.to_bf16(got).tobytes(), "the bfloat16 store differs from the twin on %s" % name
    print("device == twin, bit for bit (-0 as +0), on reference_channels and two_blocks", flush=True)
    from tests import head_bf16_twin as btwin
    for name in ("reference_channels", "two_blocks", "exact_reference_channels"):
        d = btwin.reference(name)
        t = [torch.tensor(np.asarray(d[k]), device=dev) for k in btwin.KEYS]
        for mode in MODES:
            got = head.pvnet_head(*t, negative_slope=d["slope"], compute=mode).cpu().numpy()
            assert btwin.within(got, d[mode], mode), "compute=%s leaves the twin's bound_acc on %s" % (mode, name)
            if mode == "bfloat16" and name in btwin.EXACT_CASES:
                assert btwin.same_bits(got, d[mode]["out64"].astype(np.float32)), "compute=bfloat16 differs on the exact-sum case"
            print("compute=%s within bound_acc of its twin on %s: worst share %.3g" % (mode, name, btwin.worst(got, d[mode])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="calls back to back inside one timed window")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H, W = a.height, a.width
    for B in (1, 32):
        for dt in (torch.float32, torch.bfloat16):
            flop, nbytes, t_mat, t_mem = floors(B, H, W, dt)
            print("B = %d, %s: %.2f GFLOP -> %.4f ms at the matrix rate; %.1f MB -> %.4f ms at the copy rate"
                  % (B, str(dt).replace("torch.", ""), flop / 1e9, t_mat, nbytes / 1e6, t_mem), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("head_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    batches = [int(b) for b in a.batches.split(",")]
    lines = []
    with torch.no_grad():
        check_against_the_twin(dev)
        for B in batches:
            m, fm, x, up = make(B, H, W, dev)
            for dt in (torch.float32, torch.bfloat16):
                name = str(dt).replace("torch.", "")
                flop, nbytes, t_mat, t_mem = floors(B, H, W, dt)
                res = {"B": B, "H": H, "W": W, "C2": C2, "C0": C0, "M1": M1, "M2": M2, "out_dtype": name, "rounds": a.rounds,
                       "warmup": a.warmup, "reps": a.reps, "flop": flop, "bytes": nbytes, "floor_matrix_ms": round(t_mat, 4),
                       "floor_bytes_ms": round(t_mem, 4)}
                if B == batches[0]:
                    diff = (fused(m, fm, x, dt).float() - torch_chain(m, up, fm, x, dt).float()).abs().max()
                    res["fused_vs_torch_max_abs"] = float(diff)
                    print("B = %d, %s: max |fused - torch chain| = %.3g (informational)" % (B, name, float(diff)), flush=True)
                    try:
                        for mode, (worst, median) in keypoint_shift(m, fm, x).items():
                            res["keypoint_shift_px_" + mode] = {"max": worst, "median": median}
                            print("B = %d: |keypoint(%s head) - keypoint(float32 head)| max %.3g px, median %.3g px (informational)"
                                  % (B, mode, worst, median), flush=True)
                    except Exception as e:                                       # random weights need not give a usable mask
                        print("keypoint comparison skipped: %s" % e, flush=True)
                forms = {"fused": lambda: [fused(m, fm, x, dt) for _ in range(a.reps)],
                         "bfloat16": lambda: [fused(m, fm, x, dt, "bfloat16") for _ in range(a.reps)],
                         "torch": lambda: [torch_chain(m, up, fm, x, dt) for _ in range(a.reps)],
                         "torch_autocast": lambda: [torch_autocast(m, up, fm, x, dt) for _ in range(a.reps)]}
                ms = alternate(forms, a.rounds, a.warmup)
                for form in forms:
                    res[form + "_ms"] = summary([v / a.reps for v in ms[form]], 4)
                med = res["fused_ms"]["median"]
                res["fused_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
                res["fused_over_floor_matrix"] = round(med / t_mat, 2)
                res["fused_over_floor_bytes"] = round(med / t_mem, 2)
                res["torch_over_fused"] = round(res["torch_ms"]["median"] / med, 2)
                res["fused_round_spread"] = round(res["fused_ms"]["max"] / res["fused_ms"]["min"], 3)
                for mode in MODES:
                    res["fused_over_" + mode] = round(med / res[mode + "_ms"]["median"], 2)
                    res[mode + "_over_floor_bytes"] = round(res[mode + "_ms"]["median"] / t_mem, 2)
                if B == 32 and dt == torch.float32:
                    res["accept_bfloat16"] = bool(res["fused_over_bfloat16"] >= 1.5)
                print(json.dumps(res), flush=True)
                lines.append(res)
            del m, fm, x
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
