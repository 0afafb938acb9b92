#!/usr/bin/env python
"""``clean_pvnet_amd.tless_augment`` timed with device events after warm-up (ms per batch, median and range over the timed rounds;
each round is ``--reps`` calls back to back), legs alternated in one process on the same inputs -> profiles/tless_augment_time.json.

Per batch size (32 and 1) at the reference's sizes: 400x400 cut-outs with one disc each (the target and N = 6 distractors), a
540x720 canvas, ``input_size`` (256, 256), K = 9:

  (a) device        ``TlessPVNetAugment()(bg, img, mask, kpt_2d, other_img, other_mask, draws)``: the host's records and their copy,
                    the launches of the composition and of the crop
      compose       ``tless_compose`` alone;  augment  ``tless_pvnet_augment`` alone (on (a)'s canvas, mask, keypoints and box)
  (b) torch_ops     the same chain in torch ops on the same GPU in its cheapest form, in float32: ONE ``grid_sample`` turns the
                    target (image and mask as four channels) straight onto the canvas and one the N distractors, at places fixed
                    by the draws (no box of a rotated mask, no ``randint`` on it); N ``torch.where`` build the fused canvas; the
                    branch is a ``torch.where`` on two sums; the crop is one ``grid_sample`` through a transform handed in from (a)
                    (no box of the final mask, no ``magnify_box`` on the device: the kept rectangle is handed in too); the colour
                    steps pointwise in a fixed order with ``mean`` for the grey level; the mask by a nearest ``grid_sample``; the
                    keypoints by two ``baddbmm``.  It leaves out every box reduction and the placement they feed, the exclusive
                    extents, the fixed-point sampling and the rounding to uint8 between the stages.  Different arithmetic: it is
                    a cost comparison and is not compared for equality.

The device is compared with the numpy twin (tests/tless_augment_twin.py) on the first sample before anything is timed.  No time is
a pass criterion anywhere; this is for whoever has the card.

    python tools/tless_augment_time.py [--batches 32,1] [--rounds 20] [--warmup 3] [--reps 3] [--out profiles/tless_augment_time.json]
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
import torch.nn.functional as F  # noqa: E402

import lib  # noqa: E402

lib._register_clean_pvnet_amd()
from _timing import alternate, summary  # noqa: E402
from clean_pvnet_amd import tless_augment as ta  # noqa: E402
from tests import tless_augment_twin as twin  # noqa: E402

H, W, CH, CW, N, K = 540, 720, 400, 400, 6, 9
IH, IW = 256, 256


def inputs(B, rng):
    y, x = np.meshgrid(np.arange(CH), np.arange(CW), indexing="ij")

    def discs(shape):
        m = np.zeros(shape + (CH, CW), np.uint8)
        for i in np.ndindex(shape):
            cy, cx, r = rng.uniform(0.35, 0.65) * CH, rng.uniform(0.35, 0.65) * CW, rng.uniform(60, 110)
            m[i] = (y - cy) ** 2 + (x - cx) ** 2 < r * r
        return m
    bg = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    img, other_img = rng.integers(0, 256, (B, CH, CW, 3), dtype=np.uint8), rng.integers(0, 256, (B, N, CH, CW, 3), dtype=np.uint8)
    return bg, img, discs((B,)), rng.random((B, K, 2)) * [CW, CH], other_img, discs((B, N))


def thetas(deg, uy, ux):
    """affine_grid maps that turn a CH x CW cut-out by ``deg`` onto the H x W canvas around a centre fixed by (uy, ux)."""
    t = np.zeros(deg.shape + (2, 3), np.float32)
    for i in np.ndindex(deg.shape):
        c, s = math.cos(math.radians(deg[i])), math.sin(math.radians(deg[i]))
        ox, oy = (ux[i] - 0.5) * (W - CW) / CW * 2, (uy[i] - 0.5) * (H - CH) / CH * 2
        A = np.array([[c * W / CW, -s * H / CW], [s * W / CH, c * H / CH]])
        t[i] = np.concatenate([A, -(A @ [ox * CW / W, oy * CH / H])[:, None]], axis=1)
    return t


def torch_chain(bg, cut, others, th_t, th_o, top, black, ratio, th_crop, rect, alpha, light, mean, std, kpt, M_rot, M_crop):
    B = bg.shape[0]
    t = F.grid_sample(cut, F.affine_grid(th_t, (B, 4, H, W), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    o = F.grid_sample(others, F.affine_grid(th_o, (B * N, 4, H, W), align_corners=False), mode="bilinear", padding_mode="zeros",
                      align_corners=False).view(B, N, 4, H, W)
    canvas = bg.permute(0, 3, 1, 2).float()
    fused, covered = torch.where(black.view(B, 1, 1, 1), torch.zeros_like(canvas), canvas), torch.zeros(B, 1, H, W, dtype=torch.bool, device=bg.device)
    for n in range(N):
        m = o[:, n, 3:] != 0
        fused, covered = torch.where(m, o[:, n, :3], fused), covered | m
    tm = t[:, 3:] != 0
    visible, pixel_num = (tm & ~covered).sum((1, 2, 3)).double(), t[:, 3:].sum((1, 2, 3)).double()
    on_top = (top | (visible / pixel_num < ratio)).view(B, 1, 1, 1)
    over = torch.where(tm, t[:, :3], fused)
    under = torch.where(covered, fused, torch.where(tm, t[:, :3], canvas))
    img, mask = torch.where(on_top, over, under), torch.where(on_top, tm, tm & ~covered)
    grid = F.affine_grid(th_crop, (B, 3, IH, IW), align_corners=False)
    x = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    ys, xs = torch.arange(IH, device=bg.device).view(1, 1, IH, 1), torch.arange(IW, device=bg.device).view(1, 1, 1, IW)
    r = rect.view(B, 4, 1, 1, 1)
    x = torch.where((xs >= r[:, 0]) & (xs <= r[:, 2]) & (ys >= r[:, 1]) & (ys <= r[:, 3]), x, torch.zeros_like(x)).round().clamp(0, 255) / 255
    gs = (x[:, 0] * 0.114 + x[:, 1] * 0.587 + x[:, 2] * 0.299)[:, None]
    gm = gs.mean((1, 2, 3), keepdim=True)
    a = alpha.view(B, 3, 1, 1, 1)
    x = x * a[:, 0]
    x = x * a[:, 1] + gm * (1 - a[:, 1])
    x = x * a[:, 2] + gs * (1 - a[:, 2])
    inp = (x + light.view(B, 3, 1, 1) - mean) / std
    out_mask = F.grid_sample(mask.float(), grid, mode="nearest", padding_mode="zeros", align_corners=False).to(torch.uint8)
    k = torch.baddbmm(M_rot[:, :, 2:].transpose(1, 2), kpt, M_rot[:, :, :2].transpose(1, 2))
    k = torch.baddbmm(M_crop[:, :, 2:].transpose(1, 2), k, M_crop[:, :, :2].transpose(1, 2))
    return inp, out_mask, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls back to back inside one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tless_augment_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tless_augment_time: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    lines = []
    for B in (int(v) for v in a.batches.split(",")):
        host = inputs(B, np.random.default_rng(B))
        d = twin.draws_for(B, N, 7)
        d[0, twin.TOP] = 0.75                                                                  # the compared sample takes the occlusion test
        c_h = twin.compose(*[v[:1] for v in host], d[:1])
        a_h = twin.augment(c_h["img"], c_h["mask"], c_h["kpt_2d"], c_h["bbox"], d[:1], input_size=(IH, IW))
        g = [torch.tensor(v, device=dev) for v in host]
        aug = ta.TlessPVNetAugment(input_size=(IH, IW))
        comp = ta.tless_compose(*g, d)
        out = ta.tless_pvnet_augment(comp["img"], comp["mask"], comp["kpt_2d"], comp["bbox"], d, input_size=(IH, IW))
        same = all(comp[k][:1].cpu().numpy().tobytes() == c_h[k].tobytes() for k in twin.COMPOSE_KEYS) and \
            all(out[k][:1].cpu().numpy().tobytes() == a_h[k].tobytes() for k in twin.AUGMENT_KEYS)
        assert same, "the device differs from the twin"
        f32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=dev)           # noqa: E731
        cut = torch.cat([g[1], g[2][..., None]], -1).permute(0, 3, 1, 2).float()
        others = torch.cat([g[4], g[5][..., None]], -1).view(B * N, CH, CW, 4).permute(0, 3, 1, 2).float()
        cols = twin.N_SAMPLE + twin.PER * np.arange(N)
        th_t = f32(thetas(d[:, twin.ROT] * 360., d[:, twin.DST_Y], d[:, twin.DST_X]))
        th_o = f32(thetas(d[:, cols] * 360., d[:, cols + 1], d[:, cols + 2]).reshape(B * N, 2, 3))
        T = out["trans_input"].cpu().numpy()
        th_crop = f32(np.stack([np.array([[W / IW / t[0, 0] * IW / W, 0, ((IW - 1) / 2 - t[0, 2]) / t[0, 0] * 2 / W - 1 + 1 / W],
                                          [0, H / IH / t[1, 1] * IH / H, ((IH - 1) / 2 - t[1, 2]) / t[1, 1] * 2 / H - 1 + 1 / H]]) for t in T]))
        alpha, light = (f32(np.stack([ta.colour_params(u, ta.EIG_VAL, ta.EIG_VEC)[i] for u in d])) for i in (1, 3))
        mean, std = f32(twin.MEAN).view(1, 3, 1, 1), f32(twin.STD).view(1, 3, 1, 1)
        top, black = torch.tensor(d[:, twin.TOP] < 0.5, device=dev), torch.tensor(d[:, twin.BLACK] >= 0.9, device=dev)
        M_rot = f32(np.stack([np.reshape(twin.rotation(CH, CW, u * 360.)[0], (2, 3)) for u in d[:, twin.ROT]]))
        args = (g[0], cut, others, th_t, th_o, top, black, 0.8, th_crop, out["box"], alpha, light, mean, std, g[3].float(), M_rot, out["trans_input"].float())
        forms = {"device": lambda: [aug(*g, draws=d) for _ in range(a.reps)],
                 "compose": lambda: [ta.tless_compose(*g, d) for _ in range(a.reps)],
                 "augment": lambda: [ta.tless_pvnet_augment(comp["img"], comp["mask"], comp["kpt_2d"], comp["bbox"], d, input_size=(IH, IW)) for _ in range(a.reps)],
                 "torch_ops": lambda: [torch_chain(*args) for _ in range(a.reps)]}
        ms = alternate(forms, a.rounds, a.warmup)
        res = {"B": B, "canvas": [H, W], "cutouts": [1 + N, CH, CW], "input_size": [IH, IW], "K": K, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
               "paths": np.bincount(comp["path"].cpu().numpy(), minlength=4).tolist(),
               "torch_ops_leaves_out": "the boxes of the rotated masks and of the final mask with the placements and the crop they feed (handed in), "
                                       "magnify_box (handed in), fixed-point sampling, uint8 rounding between the stages; float32 throughout"}
        for name in forms:
            res[name + "_ms"] = summary([v / a.reps for v in ms[name]], 4)
        res["device_us_per_image"] = round(res["device_ms"]["median"] * 1e3 / B, 1)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
