"""Fold one rocprofv3 --pmc pass over the bench (k_vote_mfma only) into the
issue-slot figures of DESIGN section 7b:
    vote_issue_pmc.py COUNTER_DIR OUT.json [CLOCK_GHZ (2.4)]
Per launch: the counters' means, VALU instructions per wave, and the share of
the SIMDs' cycles in which a VALU instruction (MFMA included) was issuing.
SQ_ACTIVE_INST_VALU, SQ_BUSY_CYCLES and SQ_WAVE_CYCLES count quad-cycles (x 4 =
shader cycles); SQ_VALU_MFMA_BUSY_CYCLES counts shader cycles (32 per 32x32 MFMA of
8 passes), so it is not multiplied.  (profiles/vote_issue/pmc_*.json were written
when this tool multiplied it too: their mfma_busy_share_of_simd_cycles is four
times too high.)"""
import collections
import csv
import glob
import json
import sys

src, out = sys.argv[1], sys.argv[2]
ghz = float(sys.argv[3]) if len(sys.argv) > 3 else 2.4
SIMDS = 256 * 4
vals, durs = collections.defaultdict(list), []
for f in glob.glob(src + "/**/*counter_collection.csv", recursive=True):
    seen = set()
    for r in csv.DictReader(open(f)):
        if "k_vote_mfma" not in r["Kernel_Name"]:
            continue
        vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
        if r["Dispatch_Id"] not in seen:
            seen.add(r["Dispatch_Id"])
            durs.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
m = {k: sum(v) / len(v) for k, v in vals.items()}
d = {"launches": len(durs), "counters_mean_per_launch": m}
if durs:
    d["duration_us_under_pmc"] = sum(durs) / len(durs) / 1e3
    cyc = d["duration_us_under_pmc"] * 1e3 * ghz * SIMDS     # SIMD cycles of a launch at the nominal clock
    if "SQ_ACTIVE_INST_VALU" in m:
        d["valu_issue_share_of_simd_cycles"] = 4 * m["SQ_ACTIVE_INST_VALU"] / cyc
    if "SQ_VALU_MFMA_BUSY_CYCLES" in m:
        d["mfma_busy_share_of_simd_cycles"] = m["SQ_VALU_MFMA_BUSY_CYCLES"] / cyc
        d["mfma_busy_cycles_per_simd"] = m["SQ_VALU_MFMA_BUSY_CYCLES"] / SIMDS
if m.get("SQ_WAVES"):
    d["valu_insts_per_wave"] = m.get("SQ_INSTS_VALU", 0.0) / m["SQ_WAVES"]
    if "SQ_ACTIVE_INST_VALU" in m and "SQ_WAVE_CYCLES" in m:
        d["valu_active_share_of_wave_cycles"] = m["SQ_ACTIVE_INST_VALU"] / m["SQ_WAVE_CYCLES"]
json.dump(d, open(out, "w"), indent=1)
print(json.dumps(d, indent=1))
