"""Counters of the int8 dump launches per MFMA form (profiles/r08s16/pmc_shapes.txt).

    python tools/pmc_shapes.py <dir>

<dir> holds, per form F in {16, 32} (32: the run had VS_X1_DUMP_MFMA=32):
  c3_kernel_stats_F.csv     rocprofv3 --kernel-trace --stats of tools/step_timeline.py
  pmc_F/g<i>/               rocprofv3 --pmc passes of bench.py --steps 1 --warmup 0
                            (tools/pmc_passes.sh's command), one group per run
  prof_F/pmc_{fetch,write}/ the FETCH_SIZE and WRITE_SIZE passes (tools/pmc_summary.py)
Every counter pass is a run of its own with nothing traced beside --pmc.  Prints
the mean per dump dispatch, the held clock (GRBM_GUI_ACTIVE / 8 / wall), MFMA
busy and the HBM bytes (gfx950 correction: 2 x FETCH_SIZE + WRITE_SIZE)."""
import collections
import csv
import glob
import os
import sys

root = sys.argv[1]
for form in ("16", "32"):
    # wall per dump dispatch from the traced search's kernel stats (a run of its own)
    wall_ns = None
    p = os.path.join(root, f"c3_kernel_stats_{form}.csv")
    if os.path.exists(p):
        for r in csv.DictReader(open(p)):
            if "gemm_topk_x1<8, 0, true, 1" in r["Name"]:
                wall_ns = float(r["AverageNs"])
                print(form, "trace:", r["Name"][:60], "calls", r["Calls"], "mean us %.1f" % (wall_ns / 1e3))
    vals = collections.defaultdict(list)
    ts = []
    for path in glob.glob(os.path.join(root, f"pmc_{form}", "g*", "**", "*counter_collection.csv"), recursive=True) + \
            glob.glob(os.path.join(root, f"prof_{form}", "pmc_*", "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "gemm_topk_x1<8, 0, true, 1" not in r["Kernel_Name"]:
                continue
            vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
            if r["Counter_Name"] == "GRBM_GUI_ACTIVE" and "Start_Timestamp" in r and "g0" in path:
                ts.append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    m = {k: sum(v) / len(v) for k, v in vals.items()}
    n = {k: len(v) for k, v in vals.items()}
    print(form, "counters (mean per dispatch):", {k: "%.6g (n=%d)" % (m[k], n[k]) for k in sorted(m)})
    if "GRBM_GUI_ACTIVE" in m:
        g = m["GRBM_GUI_ACTIVE"] / 8
        if ts:
            w = sum(ts) / len(ts)
            print(form, "profiled wall per dispatch us %.1f, held clock GHz %.3f (same pass)" % (w / 1e3, g / w))
        if wall_ns:
            print(form, "held clock GHz %.3f (cycles of the counter pass / wall of the traced search)" % (g / wall_ns))
        if "SQ_VALU_MFMA_BUSY_CYCLES" in m:
            print(form, "mfma_busy %.3f" % (m["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * g)))
        for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
            if k in m:
                print(form, k + "/wave %.3f" % (m[k] / m["SQ_WAVE_CYCLES"]))
    if "FETCH_SIZE" in m:
        print(form, "HBM bytes per dispatch %.4g" % (2 * m["FETCH_SIZE"] * 1024 + m.get("WRITE_SIZE", 0) * 1024))
