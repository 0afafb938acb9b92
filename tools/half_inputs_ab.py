"""A/B of 2-byte input fields (PVV_FLAG_VERTEX_* / PVV_FLAG_SEG_*) against float32 ones, in ONE process -> profiles/half_inputs.json.

Legs, alternated within every repetition after a warm-up, timed with device events on the current stream:
  f32         float32 seg / vertex fields
  bf16        the same numbers in bfloat16, read as they are
  f16         the same numbers in float16, read as they are
  bf16_cast   bfloat16 fields, `.float()` and then the float32 call (what a caller had to do before)
Calls: ransac_voting_layer_v3(mask, vertex, 512, 0.99) on cfg3 (B = 64, contiguous [B,H,W,K,2] vertex); decode_keypoint default
and un_pnp on cfg3 (B = 64) and decode_keypoint default on cfg2 (B = 1), both on the real caller's layout (seg and vertex as channel
slices of one [B, 2 + 2K, H, W] tensor).  Also the scan and compaction stage times inside the pipeline (stage_ms_in_pipeline) and
the bytes of the input fields those two stages must read, computed from shapes.

    python tools/half_inputs_ab.py [--reps 40] [--warmup 5] [--out profiles/half_inputs.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ["f32", "bf16", "f16", "bf16_cast"]
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def network_output(synth, B, H, W, K, seed):
    """[B, 2 + 2K, H, W] float32: two-class logits whose argmax is the synthetic mask, then the planar vertex field"""
    d = synth.make_batch(B=B, H=H, W=W, K=K, fg=0.02, sigma=0.05, seed=seed, planar=True, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty(B, 2 + 2 * K, H, W, device="cuda")
    x[:, :2] = torch.randn(B, 2, H, W, generator=g, device="cuda") * 0.1
    x[:, 0] += 1.0
    x[:, 1] += 4.0 * (d["mask"] != 0)
    x[:, 2:] = d["vertex"].permute(0, 3, 4, 1, 2).reshape(B, 2 * K, H, W)
    return x, d


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def ab(fns, reps, warmup):
    """fns: {leg: callable}; the legs alternate inside every repetition -> {leg: stats}"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for r in range(reps):
        order = list(fns) if r % 2 == 0 else list(fns)[::-1]          # alternate the order too: no leg always runs first
        for k in order:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fns[k]()
            e.record()
            ev[k].append((s, e))
    torch.cuda.synchronize()
    return {k: stats([s.elapsed_time(e) for s, e in v]) for k, v in ev.items()}


def summarize(res):
    """per call: each native leg's median relative to the float32 fields and to bf16 + `.float()`; per stage: bf16 vs f32"""
    out = {}
    for c, legs in res["calls"].items():
        f32, cast = legs["f32"]["median_ms"], legs["bf16_cast"]["median_ms"]
        out[c] = {k: {"vs_f32": round(legs[k]["median_ms"] / f32, 3), "vs_bf16_cast": round(legs[k]["median_ms"] / cast, 3),
                      "f32_p10_p90_ms": [legs["f32"]["p10_ms"], legs["f32"]["p90_ms"]]} for k in ("bf16", "f16")}
    for c, st in res["stages_ms"].items():
        if c.endswith(" bf16"):
            ref = res["stages_ms"][c[:-5] + " f32"]
            out["stage " + c] = {k: round(st[k]["median_ms"] / ref[k]["median_ms"], 3) for k in st}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_inputs.json"))
    a = ap.parse_args()
    import lib
    lib._register_clean_pvnet_amd()
    from clean_pvnet_amd import ransac_voting as ext
    from clean_pvnet_amd import synth
    from clean_pvnet_amd.decode import decode_keypoint
    from clean_pvnet_amd.ransac_voting_gpu import ransac_voting_layer_v3

    res = {"tool": "tools/half_inputs_ab.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "legs": LEGS, "calls": {}, "stages_ms": {}, "stage_input_bytes": {}}
    c3, c2 = synth.CONFIGS["cfg3"], synth.CONFIGS["cfg2"]
    B, H, W, K = c3["B"], c3["H"], c3["W"], c3["K"]

    # ---- ransac_voting_layer_v3 on a contiguous vertex field, cfg3
    d = synth.make_batch(**c3, device="cuda")
    mask = d["mask"]
    v = {k: d["vertex"].to(t) for k, t in DT.items()}
    del d
    fns = {k: (lambda k=k: ransac_voting_layer_v3(mask, v[k], 512, 0.99, seed=7)) for k in DT}
    fns["bf16_cast"] = lambda: ransac_voting_layer_v3(mask, v["bf16"].float(), 512, 0.99, seed=7)
    res["calls"]["ransac_voting_layer_v3 cfg3 B=64"] = ab(fns, a.reps, a.warmup)
    tn = [int(t) for t in (mask != 0).sum((1, 2))]
    # scan + compaction inside the pipeline (device RNG, AUTO): per dtype, over reps calls
    for k in DT:
        ms = ext.stage_ms_in_pipeline([mask], [v[k]], 512, 0.99, 5, 30000, 11, a.reps + 5)[5:]
        res["stages_ms"]["v3 cfg3 B=64 " + k] = {"scan": stats([m[0] for m in ms]), "compact_hyp": stats([m[1] for m in ms])}
    for k in DT:
        es = torch.tensor([], dtype=DT[k]).element_size()
        res["stage_input_bytes"]["v3 cfg3 B=64 " + k] = {
            "scan_mask": B * H * W * mask.element_size(),
            "compact_vertex_rows": sum(tn) * K * 2 * es, "hypothesis_pairs": B * K * 512 * 2 * 2 * es}
    del v, mask
    torch.cuda.empty_cache()

    # ---- decode_keypoint on the network's layout
    for name, cfg in (("cfg3 B=64", c3), ("cfg2 B=1", c2)):
        x32, d = network_output(synth, cfg["B"], cfg["H"], cfg["W"], cfg["K"], seed=5)
        xs = {k: x32.to(t) for k, t in DT.items()}
        del x32
        out = {k: {"seg": xs[k][:, :2], "vertex": xs[k][:, 2:]} for k in DT}
        for un_pnp in ((False, True) if name.startswith("cfg3") else (False,)):
            fns = {k: (lambda k=k: decode_keypoint(dict(out[k]), un_pnp=un_pnp, weights=un_pnp, seed=3)) for k in DT}
            fns["bf16_cast"] = lambda: decode_keypoint({"seg": out["bf16"]["seg"].float(), "vertex": out["bf16"]["vertex"].float()},
                                                       un_pnp=un_pnp, weights=un_pnp, seed=3)
            res["calls"]["decode_keypoint%s %s" % (" un_pnp" if un_pnp else "", name)] = ab(fns, a.reps, a.warmup)
        if name.startswith("cfg3"):
            # the fused decode's scan (k_tile_scan_seg2) and compaction, v3 parameters (hn 512, max_num 30000)
            Bc, Hc, Wc, Kc = cfg["B"], cfg["H"], cfg["W"], cfg["K"]
            tn = [int(t) for t in (d["mask"] != 0).sum((1, 2))]
            for k in DT:
                seg, ver = out[k]["seg"], out[k]["vertex"].permute(0, 2, 3, 1).view(Bc, Hc, Wc, Kc, 2)
                ms = ext.stage_ms_in_pipeline([], [ver], 512, 0.99, 5, 30000, 11, a.reps + 5, segs=[seg])[5:]
                res["stages_ms"]["decode (fused scan) cfg3 B=64 " + k] = {"scan": stats([m[0] for m in ms]),
                                                                           "compact_hyp": stats([m[1] for m in ms])}
                es = xs[k].element_size()
                res["stage_input_bytes"]["decode (fused scan) cfg3 B=64 " + k] = {
                    "scan_seg": Bc * 2 * Hc * Wc * es, "compact_vertex_rows": sum(tn) * Kc * 2 * es,
                    "hypothesis_pairs": Bc * Kc * 512 * 2 * 2 * es}
        del xs, out, d
        torch.cuda.empty_cache()
    res["note"] = ("median / p10 / p90 / min of device-event times per call, legs alternated; stage_input_bytes: bytes of the input "
                   "fields the stage must read at least (seg logits of the scan, vertex rows and hypothesis pairs of the compaction), "
                   "from shapes and the foreground counts")
    res["seg2_load_width"] = ("2-byte logits are read with 8-byte loads of 4 pixels, which keeps k_tile_scan_seg2's pixel -> thread "
                              "mapping (a thread owns two runs of 4 pixels, 1024 apart) and its rank code.  16-byte loads of 8 "
                              "pixels would need a thread to own 8 consecutive pixels, i.e. another mapping and rank code: not "
                              "built and not measured")
    res["summary"] = summarize(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for c, legs in res["calls"].items():
        print(c, {k: s["median_ms"] for k, s in legs.items()})
    for c, s in res["stages_ms"].items():
        print(c, {k: v["median_ms"] for k, v in s.items()})


if __name__ == "__main__":
    main()
