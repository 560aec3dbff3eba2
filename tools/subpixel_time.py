#!/usr/bin/env python3
"""The four measurements of the sub-pixel switch, written to profiles/subpixel_time.json as
median [min-max] of 21 samples, device events around every sample.

  1. Switch off against another build (--parent-lib, the parent commit's libsmt_hip.so): smt_pipeline_run_batch of 8
     pairs at 1920x1080 D=192, smt_scanline_run and smt_crossarm_aggregate (variant 13, with its map) on their own, in
     worker processes that alternate between the two libraries (SMT_HIP_LIB), --rounds of each, 21 / rounds samples per
     process.  The condition: this build's median inside the parent's own [min-max].
  2. smt_wta_subpixel against smt_wta on the same volume at 450x375 D=60, 1280x720 D=128 and 1920x1080 D=192,
     interleaved in one process, with the rate of a device copy of the volume (which moves the bytes twice).
  3. The pipeline with the switch on against off against the composed alternative (off plus smt_wta_subpixel on the
     scanline sum and on the aggregated right volume of every pair), interleaved in one process.

usage: python tools/subpixel_time.py [--parent-lib PATH] [--rounds 3] [--this-first] [--out profiles/subpixel_time.json]
       python tools/subpixel_time.py --worker N [--full]      (one process, one library, N samples: one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, PAIRS = 1080, 1920, 192, 8
WTA_SIZES = [(375, 450, 60), (720, 1280, 128), (1080, 1920, 192)]
SAMPLES = 21


def worker(n, full):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    dev = torch.device("cuda:0")

    def timed(fn, reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / reps, 4)

    def interleaved(fns, reps, count):
        for f in fns.values():
            f(); f()
        out = {k: [] for k in fns}
        for _ in range(count):
            for k, f in fns.items():
                out[k].append(timed(f, reps))
        return out

    res = {"lib": os.environ.get("SMT_HIP_LIB", "default")}
    # the stages on their own, switch off: the inputs of one 1080p pair
    L, R = synth.synth_pair(H, W, D, 3)
    Lu = torch.from_numpy(L).to(dev)
    Lf = Lu.float()
    adc = smt.AD_Census().Initialize(Lf, torch.from_numpy(R).to(dev).float(), D, H, W, 10.0, 30.0, placement_search=False,
                                     store_calibration=False)
    adc.ComputeBoth()
    ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, dev)
    ca.ComputeArmLengths(Lu)
    agg, out = torch.empty((H, W, D), device=dev), torch.empty((H, W, D), device=dev)
    dmap = torch.empty((H, W), device=dev)
    cost = adc.GetPtrLeft()
    so = smt.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)
    ca.AggregationVertical(cost, agg, dmap)
    stage = {"aggregate_v13_ms": lambda: ca.AggregationVertical(cost, agg, dmap), "scanline_ms": lambda: so.ScanLine(agg, Lf, out, dmap)}
    if full:                                                         # the fused kernels beside them
        def agg_on():
            ca.set_subpixel(1.0); ca.AggregationVertical(cost, agg, dmap); ca.set_subpixel(None)

        def scan_on():
            so.set_subpixel(1.0); so.ScanLine(agg, Lf, out, dmap); so.set_subpixel(None)
        stage.update({"aggregate_v13_on_ms": agg_on, "scanline_on_ms": scan_on})
    res.update(interleaved(stage, 3, n))
    adc.close(); ca.close(); so.close()
    del agg, out, cost

    if full:                                                         # measurement 2
        res["wta"] = []
        for (h, w, d) in WTA_SIZES:
            vol = torch.rand((h, w, d), device=dev) * 2
            dst, m = torch.empty_like(vol), torch.empty((h, w), device=dev)
            r = interleaved({"wta_ms": lambda: smt.wta(vol, m), "wta_subpixel_ms": lambda: smt.wta_subpixel(vol, 1.0, m),
                             "copy_ms": lambda: dst.copy_(vol)}, 10, SAMPLES)
            r["shape"] = [h, w, d]
            res["wta"].append(r)
            del vol, dst

    Ls, Rs = zip(*[synth.synth_pair(H, W, D, 3 + b) for b in range(PAIRS)])
    L8, R8 = torch.from_numpy(np.stack(Ls)).to(dev), torch.from_numpy(np.stack(Rs)).to(dev)
    pipe = smt.Pipeline(H, W, D, dev)
    res.update(interleaved({"pipeline_batch8_ms": lambda: pipe.run(L8, R8)}, 2, n))
    if full:                                                         # measurement 3
        m = torch.empty((H, W), device=dev)

        def on():
            pipe.set_subpixel(1.0); pipe.run(L8, R8); pipe.set_subpixel(None)

        def composed():
            pipe.run(L8, R8)
            vols = pipe.volumes()
            for _ in range(PAIRS):
                smt.wta_subpixel(vols[3], 1.0, m); smt.wta_subpixel(vols[4], 1.0, m)
        res["pipeline_on_off"] = interleaved({"off_ms": lambda: pipe.run(L8, R8), "on_ms": on, "composed_ms": composed}, 1, SAMPLES)
    pipe.status()
    pipe.close()
    print(json.dumps(res), flush=True)


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", type=int)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--this-first", action="store_true", help="alternate this build, parent, ... instead of parent, this, ...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpixel_time.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.full)

    def child(libpath, full):
        env = dict(os.environ)
        env.pop("SMT_HIP_LIB", None)
        if libpath:
            env["SMT_HIP_LIB"] = libpath
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", str(SAMPLES // args.rounds)] + (["--full"] if full else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("worker failed (%d):\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print("worker", res["lib"], res["pipeline_batch8_ms"], file=sys.stderr, flush=True)
        return res

    keys = ("pipeline_batch8_ms", "scanline_ms", "aggregate_v13_ms")
    this, parent, first = {k: [] for k in keys}, {k: [] for k in keys}, None
    def one_parent():
        if args.parent_lib:
            r = child(args.parent_lib, False)
            for k in keys:
                parent[k] += r[k]

    for rnd in range(args.rounds):                                # parent, this, parent, this, ... (or the other way round)
        if not args.this_first:
            one_parent()
        r = child(None, rnd == 0)
        first = first or r
        for k in keys:
            this[k] += r[k]
        if args.this_first:
            one_parent()
    out = {"shape": [H, W, D], "pairs_per_pipeline_run": PAIRS, "unit": "ms", "rounds": args.rounds,
           "order": "this, parent, ..." if args.this_first else "parent, this, ...",
           "switch_off": {"this_build": {k: summary(v) for k, v in this.items()}}}
    if args.parent_lib:
        out["switch_off"]["parent_build"] = {k: summary(v) for k, v in parent.items()}
        inside = {k: min(parent[k]) <= statistics.median(this[k]) <= max(parent[k]) for k in keys}
        out["switch_off"]["this_median_inside_parent_min_max"] = inside
        out["switch_off"]["sites_to_compose_instead"] = [k for k in keys if statistics.median(this[k]) > max(parent[k])]
    out["fused_stage_same_process"] = {k: summary(first[k]) for k in ("aggregate_v13_ms", "aggregate_v13_on_ms", "scanline_ms", "scanline_on_ms")}
    out["volume_kernel"] = []
    for r in first["wta"]:
        h, w, d = r["shape"]
        gb = h * w * d * 4 / 1e9
        s = {k: summary(r[k]) for k in ("wta_ms", "wta_subpixel_ms", "copy_ms")}
        s["shape"] = r["shape"]
        s["wta_subpixel_inside_wta_min_max"] = s["wta_ms"]["min"] <= s["wta_subpixel_ms"]["median"] <= s["wta_ms"]["max"]
        s["read_GBps"] = {k: round(gb / (s[k]["median"] * 1e-3), 1) for k in ("wta_ms", "wta_subpixel_ms")}
        s["copy_GBps_moved"] = round(2 * gb / (s["copy_ms"]["median"] * 1e-3), 1)
        s["wta_subpixel_fraction_of_copy_rate"] = round(s["read_GBps"]["wta_subpixel_ms"] / s["copy_GBps_moved"], 3)
        out["volume_kernel"].append(s)
    p = first["pipeline_on_off"]
    out["pipeline_on_off"] = {k: summary(p[k]) for k in ("off_ms", "on_ms", "composed_ms")}
    out["pipeline_on_off"]["fused_not_slower_than_composed"] = statistics.median(p["on_ms"]) <= statistics.median(p["composed_ms"])
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
