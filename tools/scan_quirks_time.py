#!/usr/bin/env python3
"""The two measurements of the SMT_QUIRK_* fix flags at 1920x1080 D=192, written to
profiles/scan_quirks_time.json as median [min-max] with the sample count.

  1. The faithful path did not move: ScanLine (its three launches, flags 0) and one Pipeline.run of 8 pairs, this
     build against another build of the library (--parent-lib, e.g. the parent commit's libsmt_hip.so), in worker
     processes that alternate between the two libraries (SMT_HIP_LIB), --rounds of each.
  2. The fixed vertical passes against the faithful ones: same build, same process, interleaved -- the up pass, the
     down pass and the whole ScanLine, with and without QUIRK_FIX_SCAN_VERTICAL.

usage: python tools/scan_quirks_time.py [--parent-lib PATH] [--rounds 3] [--out profiles/scan_quirks_time.json]
       python tools/scan_quirks_time.py --worker [--fixed]      (one process, one library: prints one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, D, PAIRS = 1080, 1920, 192, 8


def worker(fixed):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    from stereo_match_traditional_amd._lib import lib, check
    dev = torch.device("cuda:0")
    L, R = synth.synth_pair(H, W, D, 3)
    Lu, Ru = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    Lf = Lu.float()
    adc = smt.AD_Census().Initialize(Lf, Ru.float(), D, H, W, 10.0, 30.0, placement_search=False, store_calibration=False)
    adc.ComputeBoth()
    ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, dev)
    ca.ComputeArmLengths(Lu)
    agg, out = torch.empty((H, W, D), device=dev), torch.empty((H, W, D), device=dev)
    dL = torch.empty((H, W), device=dev)
    ca.AggregationVertical(adc.GetPtrLeft(), agg)
    adc.close(); ca.close()
    so = smt.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def timed(fn, reps):
        fn(); fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / reps, 4)

    run = lambda: so.ScanLine(agg, Lf, out, dL)
    up = lambda: check(lib().smt_scanline_pass(so._h, p(agg), p(Lf), 2, p(out)), "smt_scanline_pass")
    down = lambda: check(lib().smt_scanline_pass(so._h, p(agg), p(Lf), 3, p(out)), "smt_scanline_pass")
    res = {"lib": os.environ.get("SMT_HIP_LIB", "default"), "scanline_ms": [timed(run, 5) for _ in range(3)]}
    if fixed:                                                     # measurement 2: interleaved in this process
        res["faithful"] = {"up_ms": [], "down_ms": [], "scanline_ms": []}
        res["fixed"] = {"up_ms": [], "down_ms": [], "scanline_ms": []}
        for _ in range(5):
            for key, q in (("faithful", 0), ("fixed", smt.QUIRK_FIX_SCAN_VERTICAL)):
                so.set_quirks(q)
                res[key]["up_ms"].append(timed(up, 5))
                res[key]["down_ms"].append(timed(down, 5))
                res[key]["scanline_ms"].append(timed(run, 5))
        so.set_quirks(0)
    so.close()
    del agg, out
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, 3 + b) for b in range(PAIRS)])
    import numpy as np
    L8, R8 = torch.from_numpy(np.stack(Ls)).to(dev), torch.from_numpy(np.stack(Rs)).to(dev)
    pipe = smt.Pipeline(H, W, D, dev)
    res["pipeline_batch8_ms"] = [timed(lambda: pipe.run(L8, R8), 2) for _ in range(3)]
    pipe.status()
    pipe.close()
    print(json.dumps(res), flush=True)


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--fixed", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_quirks_time.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.fixed)

    def child(libpath, fixed):
        env = dict(os.environ)
        env.pop("SMT_HIP_LIB", None)
        if libpath:
            env["SMT_HIP_LIB"] = libpath
        cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + (["--fixed"] if fixed else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("worker failed (%d):\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print("worker", res["lib"], res["scanline_ms"], res["pipeline_batch8_ms"], file=sys.stderr, flush=True)
        return res

    this = {"scanline_ms": [], "pipeline_batch8_ms": []}
    parent = {"scanline_ms": [], "pipeline_batch8_ms": []}
    fixed = {k: {"up_ms": [], "down_ms": [], "scanline_ms": []} for k in ("faithful", "fixed")}
    for rnd in range(args.rounds):                                # parent, this, parent, this, ...
        if args.parent_lib:
            r = child(args.parent_lib, False)
            for k in parent:
                parent[k] += r[k]
        r = child(None, rnd == 0)
        for k in this:
            this[k] += r[k]
        if rnd == 0:
            for key in fixed:
                for k in fixed[key]:
                    fixed[key][k] += r[key][k]
    out = {"shape": [H, W, D], "pairs_per_pipeline_run": PAIRS, "unit": "ms", "rounds": args.rounds,
           "faithful_path": {"this_build": {k: summary(v) for k, v in this.items()}},
           "vertical_fix_same_process": {key: {k: summary(v) for k, v in fixed[key].items()} for key in fixed}}
    if args.parent_lib:
        out["faithful_path"]["parent_build"] = {k: summary(v) for k, v in parent.items()}
        out["faithful_path"]["this_median_inside_parent_min_max"] = {
            k: parent[k] and min(parent[k]) <= statistics.median(this[k]) <= max(parent[k]) for k in this}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
