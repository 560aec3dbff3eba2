#!/usr/bin/env python3
"""Reads the kernel trace of a bench.py run (rocprofv3 --kernel-trace --output-format csv) and reports how the maps-only
launches of a step lie on the device: their durations, how long consecutive launches overlap, the offset between their
starts, the wall time of a step from its first launch's start to its last launch's end, and how much of every
stand-alone k_prep and k_shared_convert lies beside a cost launch.
usage: chain_trace.py KERNEL_TRACE.csv [pairs per step, default 8] [steps to report, default 20: the last ones]"""
import csv
import json
import statistics
import sys

COST = ("k_cost_maps_shared", "k_cost_maps2p")
AUX = ("k_prep", "k_shared_convert")


def main():
    path = sys.argv[1]
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        kind = next((k for k in COST + AUX if k in name), None)
        if kind:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, r.get("Queue_Id", "")))
    rows.sort()
    every = [r for r in rows if r[2] in COST]
    cost = every[-per * steps:]
    if len(cost) < per * steps:
        raise SystemExit(f"{len(cost)} cost launches in the trace, {per * steps} wanted")
    # the table kernel in front of a step's first launch and the conversion behind its last belong to the step
    t0, t1 = cost[0][0], cost[-1][1]
    aux = [r for r in rows if r[2] in AUX and r[1] > t0 - 200_000 and r[0] < t1 + 200_000]
    us = lambda ns: round(ns / 1e3, 2)
    med = lambda v: us(statistics.median(v)) if v else None
    dur = [e - s for s, e, _, _ in cost]
    overlap, offset, gap, wall = [], [], [], []
    for k in range(0, len(cost), per):
        step = cost[k:k + per]
        wall.append(max(e for _, e, _, _ in step) - step[0][0])
        for a, b in zip(step, step[1:]):
            overlap.append(max(0, min(a[1], b[1]) - b[0]))
            offset.append(b[0] - a[0])
            gap.append(max(0, b[0] - a[1]))
    beside = {k: [] for k in AUX}
    for s, e, kind, _ in aux:
        covered = sum(max(0, min(e, ce) - max(s, cs)) for cs, ce, _, _ in every if ce > s and cs < e)
        beside[kind].append(min(1.0, covered / max(1, e - s)))
    out = {
        "cost_launches": len(cost), "queues": sorted({q for _, _, _, q in cost}),
        "launch_us": {"min": us(min(dur)), "median": med(dur), "mean": us(statistics.mean(dur)), "max": us(max(dur))},
        "overlap_of_consecutive_launches_us": {"median": med(overlap), "min": us(min(overlap)), "max": us(max(overlap))},
        "start_offset_of_consecutive_launches_us": {"median": med(offset), "min": us(min(offset)), "max": us(max(offset))},
        "idle_gap_between_consecutive_launches_us": {"median": med(gap), "max": us(max(gap))},
        "step_wall_first_start_to_last_end_us": {"median": med(wall), "min": us(min(wall)), "max": us(max(wall))},
        "one_step_starts_ends_us": [(us(s - cost[-per][0]), us(e - cost[-per][0]), q) for s, e, _, q in cost[-per:]],
    }
    for kind in AUX:
        v = beside[kind]
        d = [e - s for s, e, k, _ in aux if k == kind]
        out[kind] = {"launches": len(v), "median_us": med(d),
                     "fraction_beside_a_cost_launch": sorted(round(x, 2) for x in v) if v else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
