#!/usr/bin/env python3
"""Summary of a rocprofv3 kernel trace of tools/scan_views_time.py --trace (tools/prof_scan_views.sh): per kernel name the
number of launches and the median duration, and for the scanline launches of the last pipeline call the share of their run
time during which a cross-arm aggregation kernel was running on the device.
usage: python tools/scan_views_overlap.py kernel_trace.csv out.json"""
import csv
import json
import re
import statistics
import sys


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"\(.*$", "", name).replace("void ", "")


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows))
    by = {}
    for s, e, n in ev:
        by.setdefault(n, []).append((e - s) / 1e6)
    kernels = {n: dict(launches=len(v), median_ms=round(statistics.median(v), 4), total_ms=round(sum(v), 3))
               for n, v in sorted(by.items()) if n.startswith(("k_scan", "k_aggregate"))}
    # the last pipeline call: everything behind the last but one u8 -> f32 burst is simpler to take as the second half of
    # the aggregation launches
    agg = [(s, e) for s, e, n in ev if n.startswith("k_aggregate")]
    half = agg[len(agg) // 2][0] if agg else 0
    agg = [(s, e) for s, e in agg if s >= half]
    scans = [(s, e, n) for s, e, n in ev if n.startswith("k_scan") and s >= half]

    def beside(s, e):
        return sum(max(0, min(e, b) - max(s, a)) for a, b in agg)
    per = {}
    for s, e, n in scans:
        d = per.setdefault(n, [0, 0, 0])
        d[0] += 1; d[1] += e - s; d[2] += min(e - s, beside(s, e))
    overlap = {n: dict(launches=c, total_ms=round(t / 1e6, 3), beside_an_aggregation=round(b / t, 3) if t else None) for n, (c, t, b) in sorted(per.items())}
    span = (max(e for _, e, _ in scans) - half) / 1e6 if scans else None
    out = dict(kernels=kernels, last_pipeline_call=dict(span_ms=span, aggregation_launches=len(agg), scanline_launches=overlap))
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["last_pipeline_call"]))


if __name__ == "__main__":
    main()
