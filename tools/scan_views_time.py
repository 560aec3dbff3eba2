#!/usr/bin/env python3
"""The scanline optimiser on both views (include/smt_scan_views.h), timed on one device with HIP
events; median [min - max] of the samples, written to profiles/scan_views_time.json.

  python tools/scan_views_time.py [--sizes hd,kitti,small] [--samples 21] [--pairs 8] [--ab path/to/parent/libsmt_hip.so]
                                  [--ab-rounds 7] [--out profiles/scan_views_time.json]

Sizes: hd 1920x1080 D=192, kitti 1242x375 D=256, small 450x375 D=64.  What is measured, every form of a comparison taking
its samples in turn (sample k of every form, then sample k + 1):
  default   smt_scanline_run and the default pipeline (SMT_VIEW_LEFT, ms per pair over --pairs pairs) of this library
            against the library given with --ab, in alternating child processes (--child: one process = one library,
            samples / ab-rounds samples per size); the medians must lie inside the other library's min - max
  pair      smt_scanline_run_pair (both views stored + maps) against two smt_scanline_run calls
  maps      smt_scanline_run_map against smt_scanline_run on the same inputs (the difference is the last pass's store)
  pipeline  SMT_VIEW_BOTH under SMT_PIPE_SCHEDULE 0, 1, 2 against LEFT under the same schedule, and against LEFT followed
            by what a caller has to do today: smt_scanline_run + smt_lrcheck on the right view on the caller's stream
Per-launch figures come from a kernel trace of `--trace` (one BOTH call under schedule 2 and one call of each scanline
form at the first size), run under rocprofv3 --kernel-trace --stats in a process of its own."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = dict(hd=(1080, 1920, 192), kitti=(375, 1242, 256), small=(375, 450, 64))


def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="hd,kitti,small")
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_views_time.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    sizes = args.sizes.split(",")

    if not args.child and not args.trace and args.ab:
        # alternating processes, this library first in the even rounds and second in the odd ones
        per = max(1, -(-args.samples // args.ab_rounds))
        got = {"this": {}, "parent": {}}
        for r in range(args.ab_rounds):
            order = ("this", "parent") if r % 2 == 0 else ("parent", "this")
            for who in order:
                env = dict(os.environ)
                if who == "parent":
                    env["SMT_HIP_LIB"] = os.path.abspath(args.ab)
                else:
                    env.pop("SMT_HIP_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", args.sizes, "--samples", str(per),
                                      "--pairs", str(args.pairs)], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit(f"child ({who}) failed:\n{out.stdout}{out.stderr}")
                for size, forms in json.loads(out.stdout.strip().splitlines()[-1]).items():
                    for form, v in forms.items():
                        got[who].setdefault(size, {}).setdefault(form, []).extend(v)
            print(f"ab round {r + 1}/{args.ab_rounds} done", file=sys.stderr, flush=True)
        ab = {size: {form: {who: stats(got[who][size][form]) for who in got} for form in got["this"][size]} for size in got["this"]}
        for size in ab:
            for form, d in ab[size].items():
                d["this_median_inside_parent_range"] = d["parent"]["min"] <= d["this"]["median"] <= d["parent"]["max"]
                d["parent_median_inside_this_range"] = d["this"]["min"] <= d["parent"]["median"] <= d["this"]["max"]
    else:
        ab = None

    import ctypes as C

    import numpy as np
    import torch
    from stereo_match_traditional_amd import api, synth
    from stereo_match_traditional_amd._lib import lib
    dev = torch.device("cuda:0")

    def timed(f, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def interleaved(forms, n, reps=1):
        for f in forms.values():                              # warm: allocations, code objects
            f(); f()
        torch.cuda.synchronize()
        out = {k: [] for k in forms}
        for _ in range(n):
            for k, f in forms.items():
                out[k].append(timed(f, reps))
        return out

    def volumes(H, W, D):
        g = torch.Generator(device=dev).manual_seed(H * W + D)
        mk = lambda: torch.randint(0, 64, (H, W, D), device=dev, generator=g).float()
        gr = lambda: torch.randint(0, 256, (H, W), device=dev, generator=g).float()
        return mk(), gr(), mk(), gr()

    def images(H, W, D, P):
        two = [synth.synth_pair(H, W, D, 3 + k) for k in range(2)]
        L = torch.from_numpy(np.stack([two[k % 2][0] for k in range(P)])).to(dev)
        R = torch.from_numpy(np.stack([two[k % 2][1] for k in range(P)])).to(dev)
        return L.contiguous(), R.contiguous()

    def pipeline(H, W, D, sched, views):
        if sched is None:
            os.environ.pop("SMT_PIPE_SCHEDULE", None)
        else:
            os.environ["SMT_PIPE_SCHEDULE"] = sched               # read when the handle is created
        return api.Pipeline(H, W, D, dev, scan_views=views)

    if args.child:
        res = {}
        for size in sizes:
            H, W, D = SIZES[size]
            cL, gL, _, _ = volumes(H, W, D)
            out, dl = torch.empty_like(cL), torch.empty((H, W), device=dev)
            so = api.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)
            L8, R8 = images(H, W, D, args.pairs)
            pipe = pipeline(H, W, D, None, api.VIEW_LEFT)
            forms = {"scanline_run_ms": lambda: so.ScanLine(cL, gL, out, dl),
                     "pipeline_left_ms_per_pair": lambda: pipe.run(L8, R8)}
            got = interleaved(forms, args.samples)
            got["pipeline_left_ms_per_pair"] = [v / args.pairs for v in got["pipeline_left_ms_per_pair"]]
            res[size] = got
            pipe.close(); so.close()
            del cL, gL, out, L8, R8
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        return

    p = lambda t: C.c_void_p(t.data_ptr())
    result = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "pairs": args.pairs, "sizes": {}}
    if ab is not None:
        result["default_paths_this_against_parent"] = ab
    for size in sizes:
        H, W, D = SIZES[size]
        cL, gL, cR, gR = volumes(H, W, D)
        oL, oR = torch.empty_like(cL), torch.empty_like(cR)
        dL, dR = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
        so = api.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)
        so2 = api.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)

        def two_runs():
            so.ScanLine(cL, gL, oL, dL); so.ScanLine(cR, gR, oR, dR)
        forms = {"two_scanline_run_ms": two_runs,
                 "run_pair_ms": lambda: so2.ScanLinePair(cL, gL, cR, gR, out=(oL, oR), disp=(dL, dR)),
                 "run_pair_right_maps_only_ms": lambda: so2.ScanLinePair(cL, gL, cR, gR, out=(oL, None), disp=(dL, dR), maps_only=(False, True)),
                 "scanline_run_ms": lambda: so.ScanLine(cL, gL, oL, dL),
                 "run_map_ms": lambda: so.ScanLineMap(cL, gL, dL)}
        if args.trace:
            for f in forms.values():
                f(); f()
            torch.cuda.synchronize()
            L8, R8 = images(H, W, D, args.pairs)
            pipe = pipeline(H, W, D, "2", api.VIEW_BOTH)
            pipe.run(L8, R8); pipe.run(L8, R8)
            torch.cuda.synchronize()
            pipe.close()
            print("trace run done", flush=True)
            return
        r = {k: stats(v) for k, v in interleaved(forms, args.samples, reps=3).items()}
        r["pair_saves_ms"] = round(r["two_scanline_run_ms"]["median"] - r["run_pair_ms"]["median"], 4)
        r["pair_combined_spread_ms"] = round((r["two_scanline_run_ms"]["max"] - r["two_scanline_run_ms"]["min"]) +
                                             (r["run_pair_ms"]["max"] - r["run_pair_ms"]["min"]), 4)
        r["view_axis_earns_its_place"] = r["pair_saves_ms"] > r["pair_combined_spread_ms"]
        r["maps_only_saves_ms"] = round(r["scanline_run_ms"]["median"] - r["run_map_ms"]["median"], 4)
        so.close(); so2.close()
        del oR, cR
        torch.cuda.empty_cache()

        # the pipeline: BOTH against LEFT and against LEFT + the composed right-view scan, per schedule
        L8, R8 = images(H, W, D, args.pairs)
        N = H * W
        r["pipeline_ms_per_pair"] = {}
        for sched in ("0", "1", "2"):
            left, both = pipeline(H, W, D, sched, api.VIEW_LEFT), pipeline(H, W, D, sched, api.VIEW_BOTH)
            soc = api.ScanlineOptimizer().Initialize(H, W, D, 10, 150, dev)
            cls = torch.empty((H, W), dtype=torch.uint8, device=dev)

            def composed():
                dl, dr, _, _ = left.run(L8, R8)
                agg_right = left.volumes()[3]
                # what the handle still holds is the LAST pair's aggregated right volume: a caller who wants every pair's
                # optimised right map runs the pipeline pair by pair; the cost per pair is one scan and one LR check
                for b in range(args.pairs):
                    soc.ScanLine(agg_right, gL, oL, dR)
                    lib().smt_lrcheck(p(dl[b]), p(dR), H, W, 2, p(cls), None, api.current_stream_ptr(dev))
            forms = {"left": lambda: left.run(L8, R8), "both": lambda: both.run(L8, R8), "left_plus_composed_right_scan": composed}
            got = interleaved(forms, args.samples)
            r["pipeline_ms_per_pair"][sched] = {k: stats([x / args.pairs for x in v]) for k, v in got.items()}
            left.close(); both.close(); soc.close()
            torch.cuda.empty_cache()
        os.environ.pop("SMT_PIPE_SCHEDULE", None)
        result["sizes"][size] = dict(H=H, W=W, D=D, **r)
        print(size, json.dumps(r), file=sys.stderr, flush=True)
        del cL, gL, gR, oL, L8, R8
        torch.cuda.empty_cache()
    result["view_axis_earns_its_place"] = any(v["view_axis_earns_its_place"] for v in result["sizes"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
