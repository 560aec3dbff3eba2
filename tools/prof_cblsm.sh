# kernel-trace stats of tools/cblsm_time.py at 1920x1080 D=192 (4 pairs; composed flow and batch entry side by side):
# the summed-area first pass (k_sat_cols, k_sat_rows, k_sat_box) against what it replaces (k_cblsm_ad + one order-1
# aggregation per view), and the bytes each kernel must move per hypothesis over its time against 8 TB/s.
#     sh tools/prof_cblsm.sh [out dir relative to the repository root, default prof_out/cblsm]
set -x
cd "$(dirname "$0")/.."
O=${1:-prof_out/cblsm}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/s -o s -- \
    python3 tools/cblsm_time.py --sizes 1080p --rounds 1 --reps 2 > $O/s.out 2> $O/s.err || exit 1
python3 - "$O" <<'PY'
import csv, glob, re, sys
O = sys.argv[1]
f = glob.glob(O + "/s/**/s_kernel_stats.csv", recursive=True) or glob.glob(O + "/s/s_kernel_stats.csv")
rows = list(csv.DictReader(open(f[0])))
V = 1080 * 1920 * 192
# bytes a kernel has to move per hypothesis at the least (corner and tap re-reads served by the caches)
need = {"k_sat_cols": 4, "k_sat_rows": 8, "k_sat_box": 8, "k_cblsm_ad": 4, "k_aggregate": 8}
print("kernel calls avg_ms min_ms max_ms B_per_hyp achieved_TBps of_8TBps")
for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
    name = r["Name"]
    m = re.search(r"\b(k_sat_cols|k_sat_rows|k_sat_box|k_cblsm_ad|k_aggregate)\w*", name)
    short = m.group(1) if m else None
    avg = float(r["AverageNs"]) / 1e6
    if short:
        b = need[short]
        tb = b * V / (avg * 1e-3) / 1e12
        print(short, r["Calls"], round(avg, 3), round(float(r["MinNs"]) / 1e6, 3), round(float(r["MaxNs"]) / 1e6, 3), b,
              round(tb, 2), round(tb / 8.0, 3))
    else:
        print(name[:60], r["Calls"], round(avg, 3))
PY
cp $(ls $O/s/*kernel_stats.csv $O/s/*/*kernel_stats.csv 2>/dev/null | head -1) $O/cblsm_kernel_stats.csv
