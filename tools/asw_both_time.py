"""ASWeight.cpp:60-61's two views, two ways, interleaved in one process: smt_asw left alone, smt_asw right alone (their
sum is what a caller pays today) against smt_asw_both with the rank keys (impl 2) and with the left volume + diagonal
gather (impl 1), and the batched flow (smt_asw_flow_run_batch: padding, both views, cross-check) per pair.  Device
events around every call; medians and spread over the rounds; the maps are compared in the same run.

    python tools/asw_both_time.py [--sizes config4,driver] [--rounds 5] [--reps 2] [--pairs 4] [--out profiles/asw_both_time.json]

Sizes: 960x540 D=128 winSize 16 (config 4), 450x375 D=60 winSize 11 (ASWeight.cpp:43-47's own)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"config4": (540, 960, 128, 16), "driver": (375, 450, 60, 11)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="config4,driver")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    dev = torch.device("cuda:0")
    res = {"note": "ms per call (flow: per pair), device events around each call; median [min, max] over rounds x reps; "
                   "the forms alternate inside every round", "lib": os.environ.get("SMT_HIP_LIB", "in-tree"), "sizes": {}}
    for name in a.sizes.split(","):
        H, W, D, ws = SIZES[name]
        n = a.pairs
        imgs = [synth.synth_pair(H, W, D, 4 + b) for b in range(n)]
        Lb = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
        Rb = torch.from_numpy(np.stack([x[1] for x in imgs])).to(dev)
        Lp = torch.from_numpy(np.pad(imgs[0][0], ws + 1, mode="edge")).to(dev)
        Rp = torch.from_numpy(np.pad(imgs[0][1], ws + 1, mode="edge")).to(dev)
        sp, cm = smt.asw_masks(ws, 50.0, 30.0, dev)
        flow = smt.ASWFlow(H, W, D, dev, winSize=ws)
        out = {}

        def left():
            out["left"] = smt.AdaptiveSupportWeight(Lp, Rp, ws, D, sp, cm, 40, smt.VIEW_LEFT)

        def right():
            out["right"] = smt.AdaptiveSupportWeight(Lp, Rp, ws, D, sp, cm, 40, smt.VIEW_RIGHT)

        def both2():
            smt.asw_both_set_impl(2)
            out["both2"] = smt.AdaptiveSupportWeightBoth(Lp, Rp, ws, D, sp, cm, 40)

        def both1():
            smt.asw_both_set_impl(1)
            out["both1"] = smt.AdaptiveSupportWeightBoth(Lp, Rp, ws, D, sp, cm, 40)
            smt.asw_both_set_impl(2)

        def flow_run():
            out["flow"] = flow.run(Lb, Rb)

        forms = (("left", left, 1), ("right", right, 1), ("both_impl2", both2, 1), ("both_impl1", both1, 1),
                 ("flow_per_pair", flow_run, n))

        def timed(fn, per):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / per

        for _, fn, _ in forms:                                             # warm-up: code objects, arena growth
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k, _, _ in forms}
        for _ in range(a.rounds):
            for k, fn, per in forms:
                for _ in range(a.reps):
                    t[k].append(timed(fn, per))
        st = lambda xs: {"median": float(np.median(xs)), "min": min(xs), "max": max(xs)}
        r = {k + "_ms": st(xs) for k, xs in t.items()}
        med = {k: r[k + "_ms"]["median"] for k in t}
        r["left_plus_right_ms"] = med["left"] + med["right"]
        r["both_impl2_over_left"] = med["both_impl2"] / med["left"]
        r["both_impl1_over_left"] = med["both_impl1"] / med["left"]
        r["both_impl2_over_left_plus_right"] = med["both_impl2"] / r["left_plus_right_ms"]
        r["pairs_in_flow"] = n
        dl, dr = out["both2"]
        r["dispL_equals_smt_asw_left"] = bool(torch.equal(dl, out["left"]) and torch.equal(out["both1"][0], out["left"]))
        r["dispR_impl1_equals_impl2"] = bool(torch.equal(dr, out["both1"][1]))
        r["dispR_pixels_differing_from_smt_asw_right"] = int((dr != out["right"]).sum())
        r["flow_pair0_equals_both"] = bool(torch.equal(out["flow"][0][0], dl) and torch.equal(out["flow"][1][0], dr))
        r["samples"] = {k: [round(x, 4) for x in xs] for k, xs in t.items()}
        res["sizes"][f"{W}x{H}_d{D}_w{2 * ws + 3}"] = r
        print(name, json.dumps({k: v for k, v in r.items() if k != "samples"}), flush=True)
        flow.close()
        ok = r["dispL_equals_smt_asw_left"] and r["dispR_impl1_equals_impl2"] and r["flow_pair0_equals_both"]
        del Lb, Rb, out
        torch.cuda.empty_cache()
        if not ok:
            print("MISMATCH at", name, file=sys.stderr)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
