#!/usr/bin/env python
"""Copy the judged summaries of one gpurun profiling session into profiles/ (round tag: third argument, default r02):
    python tools/refresh_profiles.py gpurun_out/prof_<tag> gpurun_out/<dir with bench_default.json, bench_extras.json, configs.json> [r02]
The session is produced on the GPU box by tools/profile_bench.sh <tag> plus `python bench.py --full [--extras]`."""
import csv, glob, json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
prof, fin = sys.argv[1], sys.argv[2]
TAG = sys.argv[3] if len(sys.argv) > 3 else "r02"


def copy_bench_lines():
    for a, b in (("bench_default", TAG + "_bench_default"), ("bench_extras", TAG + "_bench_extras"),
                 ("bench_torchrun1", TAG + "_bench_torchrun_1rank"), ("bench_under_rocprof", TAG + "_bench_under_rocprof"),
                 ("bench_driver_command", TAG + "_bench_driver_command")):
        if not os.path.exists(os.path.join(fin, a + ".json")):
            continue
        lines = [l for l in open(os.path.join(fin, a + ".json")) if l.startswith("{")]
        if lines:
            json.dump(json.loads(lines[-1]), open(os.path.join(ROOT, "profiles", b + ".json"), "w"), indent=1)


if "--bench-only" in sys.argv:      # tools/evidence_bench.sh: the lines printed with the committed profiles/call_pmc.json in place
    copy_bench_lines()
    if os.path.exists(os.path.join(fin, "kernel_stats_raw.csv")):
        rows = list(csv.DictReader(open(os.path.join(fin, "kernel_stats_raw.csv"))))
        with open(os.path.join(ROOT, "profiles", TAG + "_kernel_stats_bench_rerun.csv"), "w") as o:
            w = csv.writer(o)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
            for r in rows:
                m = re.search(r"(k_[a-z_0-9]+)(<\s*(\d+)[^>]*>)?", r["Name"])
                if m:
                    n = "%s<%s>" % (m.group(1), m.group(3)) if m.group(1) == "k_count_bf16" and m.group(3) else m.group(1)
                    w.writerow([n, r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["MinNs"], r["MaxNs"], r["StdDev"]])
    sys.exit(0)
tmp = os.path.join(ROOT, "profiles", TAG + "_summary.json")
if os.path.isdir(os.path.join(prof, "trace")):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "summarize_prof.py"), prof, "--json", tmp],
                          stdout=subprocess.DEVNULL)
    stats_csv = glob.glob(os.path.join(prof, "trace", "*kernel_stats.csv"))[0]
else:      # tools/evidence.sh summarised on the GPU box (the raw output does not fit gpurun's 64 MiB merge limit)
    json.dump(json.load(open(os.path.join(fin, "prof_summary.json"))), open(tmp, "w"), indent=1)
    stats_csv = os.path.join(fin, "kernel_stats_raw.csv")


def short(n):
    """this repository's kernel name without its template arguments -- except the count kernel's MODE (k_count_bf16<1>)"""
    m = re.search(r"(k_[a-z_0-9]+)(<\s*(\d+)[^>]*>)?", n)
    if not m:
        return None
    return "%s<%s>" % (m.group(1), m.group(3)) if m.group(1) == "k_count_bf16" and m.group(3) else m.group(1)


rows = list(csv.DictReader(open(stats_csv)))
with open(os.path.join(ROOT, "profiles", TAG + "_kernel_stats.csv"), "w") as o:
    w = csv.writer(o)
    w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
    for r in rows:
        if short(r["Name"]):
            w.writerow([short(r["Name"]), r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["MinNs"], r["MaxNs"], r["StdDev"]])
summ = json.load(open(tmp))
# the count pass of the profiled workload: one k_count_bf16<0> launch, or -- staged -- <1> + k_lead + the second launch
# (round 4: k_count_filter_runs; round 3: k_count_bf16<2>)
pass_kernels = [k for k in ("k_count_bf16<1>", "k_lead", "k_count_filter_runs", "k_count_bf16<2>") if k in summ["pmc"]] or ["k_count_bf16<0>"]
def kb(kern, name):
    return summ["pmc"].get(kern, {}).get(name, {}).get("main_mean", 0.0)
fetch = sum(kb(k, "FETCH_SIZE") for k in pass_kernels)
write = sum(kb(k, "WRITE_SIZE") for k in pass_kernels)
pmc_path = os.path.join(ROOT, "profiles", "count_kernel_pmc.json")
old = json.load(open(pmc_path))
old.update({"kernel": " + ".join(pass_kernels), "FETCH_SIZE_KB": fetch, "WRITE_SIZE_KB": write, "hbm_bytes_per_launch": int((fetch + write) * 1024),
            "images_per_launch": 64, "kernels": pass_kernels,
            "per_kernel_KB": {k: {"FETCH_SIZE": kb(k, "FETCH_SIZE"), "WRITE_SIZE": kb(k, "WRITE_SIZE")} for k in pass_kernels},
            "source": "%s (tools/profile_bench.sh: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes, python "
                      "bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-two-stream), round tag %s; 'launch' = one count "
                      "pass (the sum over the kernels listed)" % (prof, TAG)})
json.dump(old, open(pmc_path, "w"), indent=1)
# the two HBM-facing kernels of the front end (bench.py's roofline_scan / roofline_compact read this)
front = {"workload": old.get("workload"), "source": old["source"],
         "calibration": "MI355X_MICROARCH.md (HBM): on gfx950 FETCH_SIZE reports exactly half of the bytes of a wide coalesced streaming "
                        "read -- k_tile_scan is one (8 B per lane, unit stride, read once): 2 x FETCH_SIZE is taken and checks against the "
                        "known byte count, B*H*W*8 = 157.3 MB of int64 mask at B = 64 (k_stream_read, the probe, shows the same factor: "
                        "half of its 1.42 GB).  k_compact_hyp gathers 8 B per lane out of 72-byte pixel records: uncalibrated, taken x1.0; "
                        "WRITE_SIZE x1.0 (its known count: coords + planar dirs of the foreground = 64 x 6144 x 80 B = 31.5 MB + "
                        "hypotheses and zeroed counters 3.5 MB)"}
for kern, fmul in (("k_tile_scan", 2.0), ("k_compact_hyp", 1.0)):
    front[kern] = {"FETCH_SIZE_KB": kb(kern, "FETCH_SIZE"), "WRITE_SIZE_KB": kb(kern, "WRITE_SIZE"), "fetch_correction": fmul,
                   "hbm_bytes_per_launch": int((fmul * kb(kern, "FETCH_SIZE") + kb(kern, "WRITE_SIZE")) * 1024)}
json.dump(front, open(os.path.join(ROOT, "profiles", "front_kernels_pmc.json"), "w"), indent=1)

# ---- profiles/call_pmc.json (round 4): every kernel of ONE ransac_voting_layer_v3 call of the bench workload, per launch --
# HBM bytes (FETCH_SIZE corrected as MI355X_MICROARCH.md prescribes, see `fetch_correction`), issued VALU instructions, VALU
# busy -- and the same for the side paths (tools/prof_side.py: the estimate's 4096-hypothesis count kernel, the fused decode).
# bench.py reads this file for roofline.traffic, roofline_valu and the estimate's block; it says the figures are static.
WIDE_STREAMS = {"k_tile_scan": "8 B per lane, unit stride, read once: calibrated on the known byte count (B*H*W*8 of int64 mask) = 2.0 x FETCH_SIZE",
                "k_stream_read": "16 B per lane streaming read: x2 (MI355X_MICROARCH.md, HBM)",
                "k_tile_scan_seg2": "16 B per lane streaming read of two f32 planes: x2 (MI355X_MICROARCH.md, HBM); known byte count B*2*H*W*4"}


# round 6: the clock the chip ran at INSIDE the count kernels -- shader cycles (s_memtime) / real time (s_memrealtime, 100 MHz) of the blocks'
# matrix-core loops, instrumented build (tools/census_count.py, tools/census_filter.py; profiles/<TAG>_count_census.json)
EFFECTIVE_CLOCK = {}
_cc = os.path.join(fin, "count_census.json")
if not os.path.exists(_cc):
    _cc = os.path.join(ROOT, "profiles", TAG + "_count_census.json")
if os.path.exists(_cc):
    _c = json.load(open(_cc))["cases"]
    for kern, case in (("k_count_bf16<1>", "cfg3_B64_staged_first_launch"), ("side:k_count_bf16<0>", "estimate_4096_full_B64"),
                       ("side:k_count_bf16<1>", "cfg3_B64_staged_first_launch")):
        if case in _c and "effective_clock_GHz_mfma_loop" in _c[case]:
            EFFECTIVE_CLOCK[kern] = {"GHz": round(_c[case]["effective_clock_GHz_mfma_loop"], 3),
                                     "source": "profiles/%s_count_census.json case %s: s_memtime / s_memrealtime over the matrix-core loops (median call of %d; all calls: %s)"
                                               % (TAG, case, _c[case].get("calls", 0), _c[case].get("effective_clock_GHz_mfma_loop_all_calls"))}
_fc = os.path.join(fin, "filter_census.json")
if not os.path.exists(_fc):
    _fc = os.path.join(ROOT, "profiles", TAG + "_filter_census.json")
if os.path.exists(_fc):
    try:
        _f = json.load(open(_fc))
        _g = [c["shader_clock_ghz"] for c in _f.get("cases", []) if isinstance(c, dict) and "shader_clock_ghz" in c]     # (the first case is cfg3 at B = 64)
        if _g:
            for k in ("k_count_filter_runs", "side:k_count_filter_runs"):
                EFFECTIVE_CLOCK[k] = {"GHz": round(_g[0], 3), "source": "profiles/%s_filter_census.json: a block's shader cycles / its lifetime on the 100 MHz counter" % TAG}
    except Exception as e:                                               # noqa: BLE001
        print("filter census not usable for the clock:", e)


def kernel_block(summary, kern):
    def v(name):
        return summary["pmc"].get(kern, {}).get(name, {}).get("main_mean", 0.0)
    fmul = 2.0 if kern in WIDE_STREAMS else 1.0
    gui, act = v("GRBM_GUI_ACTIVE"), v("SQ_ACTIVE_INST_VALU")
    mfma, mfma_cyc = v("SQ_INSTS_MFMA"), v("SQ_VALU_MFMA_BUSY_CYCLES")
    blk = {"FETCH_SIZE_KB": v("FETCH_SIZE"), "WRITE_SIZE_KB": v("WRITE_SIZE"), "fetch_correction": fmul,
           "hbm_bytes": int((fmul * v("FETCH_SIZE") + v("WRITE_SIZE")) * 1024),
           "SQ_INSTS_VALU": int(v("SQ_INSTS_VALU")), "SQ_ACTIVE_INST_VALU": int(act), "GRBM_GUI_ACTIVE": int(gui),
           # (two counter passes: a saturated kernel can read a few % above 1; the raw ratio is kept beside the capped one)
           "valu_busy": round(min(1.0, act * 4 / 1024 / (gui / 8)), 4) if gui else None,
           "valu_busy_raw": round(act * 4 / 1024 / (gui / 8), 4) if gui else None,
           "avg_us": summary.get("kernel_stats", {}).get(kern, {}).get("avg_us")}
    # round 6 (VERDICT r5 #1b): figures that CAN be below 1 and are not instruction counts in another unit -- the share of the resident
    # waves' cycles (SQ_WAVE_CYCLES, quad-cycles summed over waves) spent waiting for an instruction to issue / complete, and the share
    # in which the wave had any instruction executing.  valu_busy above is SQ_ACTIVE_INST_VALU x 4 / SIMD cycles: that counter ticks one
    # quad-cycle per issued VALU instruction (it equals SQ_INSTS_VALU to 1 %), so "busy" = instructions x 4 cycles / time BY CONSTRUCTION --
    # an issue rate with an assumed 4-cycle cost, not an observation of a busy pipe.  Kept under its old name for continuity.
    wc = v("SQ_WAVE_CYCLES")
    if wc:
        blk.update({"SQ_WAVE_CYCLES": int(wc), "wave_wait_inst_frac": round(v("SQ_WAIT_INST_ANY") / wc, 4) if v("SQ_WAIT_INST_ANY") else None,
                    "wave_active_inst_frac": round(v("SQ_ACTIVE_INST_ANY") / wc, 4) if v("SQ_ACTIVE_INST_ANY") else None,
                    "mean_resident_waves_per_simd": round(wc * 4 / 1024 / (gui / 8), 2) if gui else None})
    clk = EFFECTIVE_CLOCK.get(kern if summary is summ else "side:" + kern)
    if clk:
        blk["effective_clock_GHz"] = clk["GHz"]
        blk["effective_clock_source"] = clk["source"]
        if blk["avg_us"] and v("SQ_INSTS_VALU"):
            blk["simd_cycles_per_valu_instruction_at_effective_clock"] = round(blk["avg_us"] * 1e-6 * clk["GHz"] * 1e9 * 1024 / v("SQ_INSTS_VALU"), 3)
    if mfma:      # round 5: the matrix pipe (SQ_VALU_MFMA_BUSY_CYCLES = 32 cycles per v_mfma_f32_32x32x16_bf16, summed over the SIMDs)
        blk.update({"SQ_INSTS_MFMA": int(mfma), "SQ_VALU_MFMA_BUSY_CYCLES": int(mfma_cyc),
                    "mfma_busy": round(mfma_cyc / 1024 / (gui / 8), 4) if gui else None,
                    "valu_per_mfma": round(v("SQ_INSTS_VALU") / mfma, 2), "SQ_INSTS_LDS": int(v("SQ_INSTS_LDS")),
                    "SQ_LDS_BANK_CONFLICT": int(v("SQ_LDS_BANK_CONFLICT"))})
    if kern in WIDE_STREAMS:
        blk["fetch_correction_why"] = WIDE_STREAMS[kern]
    return blk


call = {"workload": old.get("workload"), "round": TAG,
        "command": "python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-two-stream --no-side-legs",
        "how": "separate rocprofv3 --pmc passes of that command (tools/profile_bench.sh), per launch: the mean over the launches of the "
               "bench batch; hbm_bytes = (fetch_correction x FETCH_SIZE + WRITE_SIZE) x 1024; valu_busy = SQ_ACTIVE_INST_VALU x 4 / 1024 "
               "SIMDs / (GRBM_GUI_ACTIVE / 8 XCDs); mfma_busy = SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs / (GRBM_GUI_ACTIVE / 8); gathers and "
               "atomics are taken x1.0, uncalibrated",
        "kernels": {k: kernel_block(summ, k) for k in summ["pmc"]}}
# round 6: what the loop's own instruction mix can issue -- tools/microbench/count_pipe3.hip (per SIMD, shader cycles per matrix-core tile)
_p3 = os.path.join(fin, "count_pipe3.txt")
if not os.path.exists(_p3):
    _p3 = os.path.join(ROOT, "profiles", TAG + "_count_pipe3.txt")
if os.path.exists(_p3):
    rows3 = {}
    for line in open(_p3):
        m = re.match(r"(\d) (.*?)\s+W=(\d)\s+([\d.]+) ms \| per wave:\s+([\d.]+) cyc/tile\s+([\d.]+) ns/tile -> ([\d.]+) GHz \| per SIMD:\s+([\d.]+) ns/tile =\s+([\d.]+) cyc/tile", line)
        if m and (m.group(1), m.group(3)) not in rows3:
            rows3[(m.group(1), m.group(3))] = {"label": m.group(2).strip(), "waves_per_simd": int(m.group(3)), "ms": float(m.group(4)), "GHz": float(m.group(7)),
                                               "ns_per_tile_and_simd": float(m.group(8)), "cycles_per_tile_and_simd": float(m.group(9))}
    if ("0", "5") in rows3 and ("8", "5") in rows3 and ("5", "5") in rows3:
        VPT = 21.75                                                      # VALU instructions per tile in the loop's listing (174 per 8 tiles)
        call["count_loop_microbench"] = {
            "source": "profiles/%s_count_pipe3.txt (tools/microbench/count_pipe3.hip): the kernel's per-tile loop alone, 5 waves per SIMD, 60 ms pre-warm; "
                      "per SIMD = kernel time by HIP events / tiles per SIMD, converted with the clock measured inside the loop (s_memtime / s_memrealtime)" % TAG,
            "valu_instructions_per_tile": VPT,
            "shipped_loop": rows3[("0", "5")], "valu_alone": rows3[("8", "5")], "mfma_alone": rows3[("5", "5")],
            "calibration_one_wave_per_simd_mfma_alone": rows3.get(("5", "1")),
            "knock_outs": {k: rows3[(k, "5")] for k in ("6", "7", "1") if (k, "5") in rows3},
            "occupancy": {w: rows3[("0", w)] for w in ("4", "6", "8") if ("0", w) in rows3},
            "simd_cycles_per_valu_instruction_valu_alone": round(rows3[("8", "5")]["cycles_per_tile_and_simd"] / VPT, 3),
            "simd_cycles_per_valu_instruction_with_mfma": round(rows3[("0", "5")]["cycles_per_tile_and_simd"] / VPT, 3)}
side_path = os.path.join(fin, "prof_side_summary.json")
if os.path.exists(side_path):
    side = json.load(open(side_path))
    json.dump(side, open(os.path.join(ROOT, "profiles", TAG + "_side_summary.json"), "w"), indent=1)
    if "k_count_bf16<0>" in side.get("pmc", {}):
        call["estimate_4096"] = dict(kernel_block(side, "k_count_bf16<0>"), kernel="k_count_bf16<0> at 4096 hypotheses (estimate_voting_distribution_with_mean, B = 64)",
                                     command="python tools/prof_side.py")
    call["decode_fused"] = {k: kernel_block(side, k) for k in ("k_tile_scan_seg2", "k_mask_from_lists") if k in side.get("pmc", {})}
json.dump(call, open(os.path.join(ROOT, "profiles", "call_pmc.json"), "w"), indent=1)
for extra_name in ("staged_ab.json", "staged_ab_outliers.json", "ab_filter_runs.txt", "auto_regret.json", "filter_census.json", "count_pipe2.txt",
                   "count_census.json", "count_pipe3.txt"):
    if os.path.exists(os.path.join(fin, extra_name)):
        import shutil
        shutil.copy(os.path.join(fin, extra_name), os.path.join(ROOT, "profiles", TAG + "_" + extra_name))
copy_bench_lines()
if os.path.exists(os.path.join(fin, "configs.json")):
    json.dump(json.load(open(os.path.join(fin, "configs.json"))), open(os.path.join(ROOT, "profiles", TAG + "_configs.json"), "w"), indent=1)
for extra in glob.glob(os.path.join(fin, "gaps_*.json")):
    json.dump(json.load(open(extra)), open(os.path.join(ROOT, "profiles", TAG + "_" + os.path.basename(extra)), "w"), indent=1)
k = summ["kernel_stats"]
for kern in pass_kernels:
    g = kb(kern, "GRBM_GUI_ACTIVE") / 8
    if g and kern in k:
        print("%s avg_us %.2f  VALU insts %.3g  VALU busy (of GUI/8 cycles) %.3f" % (
            kern, k[kern]["avg_us"], kb(kern, "SQ_INSTS_VALU"), kb(kern, "SQ_ACTIVE_INST_VALU") * 4 / 1024 / g))
for n, v in k.items():
    print("  %-20s %8.2f us" % (n, v["avg_us"]))
