"""SADmain.cpp:66-67's two views, two ways, interleaved in one process: smt_sad left alone, smt_sad right alone (their
sum is what a caller pays without smt_sad_both) against smt_sad_both with the box kernel forced -- rank keys (impl 2)
and left volume + diagonal gather (impl 1) --, smt_sad_both as dispatched by default, smt_sad_both composing smt_sad,
and the batched flow (smt_sad_flow_run_batch: padding, both views, cross-check) per pair.  Device events around every
call; medians and spread over the rounds; the maps are compared in the same run.

    python tools/sad_both_time.py [--sizes config1,driver,...] [--rounds 7] [--reps 3] [--pairs 4] [--out profiles/sad_both_time.json]

With SMT_HIP_LIB pointing at a library that has no smt_sad_both (the parent commit's), only the two smt_sad calls are
timed: that is how the baseline is confirmed unchanged.

Sizes (W x H, D, winsize): config1 450x375 64 1; driver 450x375 60 3 (SADmain.cpp:33-34); driver21 450x375 60 21 (the
`// 21` beside :34); hd 1920x1080 128 3; hd21 1920x1080 128 21."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"config1": (375, 450, 64, 1), "driver": (375, 450, 60, 3), "driver21": (375, 450, 60, 21),
         "hd": (1080, 1920, 128, 3), "hd21": (1080, 1920, 128, 21)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="config1,driver,driver21,hd,hd21")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    from stereo_match_traditional_amd._lib import lib
    dev = torch.device("cuda:0")
    have_both = hasattr(lib(), "smt_sad_both")
    res = {"note": "ms per call (flow: per pair), device events around each call; median [min, max] over rounds x reps; "
                   "the forms alternate inside every round", "lib": os.environ.get("SMT_HIP_LIB", "in-tree"),
           "has_smt_sad_both": have_both, "sizes": {}}
    bad = False
    for name in a.sizes.split(","):
        H, W, D, ws = SIZES[name]
        n = a.pairs
        imgs = [synth.synth_pair(H, W, D, 4 + b) for b in range(n)]
        Lp = torch.from_numpy(np.pad(imgs[0][0], ws + 1, mode="edge")).to(dev)
        Rp = torch.from_numpy(np.pad(imgs[0][1], ws + 1, mode="edge")).to(dev)
        out = {}

        def left():
            out["left"] = smt.GetPointDepthLeft(Lp, Rp, D, ws)

        def right():
            out["right"] = smt.GetPointDepthRight(Lp, Rp, D, ws)

        forms = [("left", left, 1), ("right", right, 1)]
        if have_both:
            Lb = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
            Rb = torch.from_numpy(np.stack([x[1] for x in imgs])).to(dev)
            flow = smt.SADFlow(H, W, D, dev, winsize=ws)

            def both(key, dispatch, impl):
                def f():
                    smt.sad_both_set_dispatch(dispatch)
                    smt.sad_both_set_impl(impl)
                    out[key] = smt.GetPointDepthBoth(Lp, Rp, D, ws)
                    out[key + "_form"] = smt.sad_both_last_form()
                    smt.sad_both_set_dispatch(0)
                    smt.sad_both_set_impl(2)
                return f

            def flow_run():
                out["flow"] = flow.run(Lb, Rb)

            forms += [("both_box_impl2", both("box2", 1, 2), 1), ("both_box_impl1", both("box1", 1, 1), 1),
                      ("both_default", both("default", 0, 2), 1), ("both_composed", both("composed", 2, 2), 1),
                      ("flow_per_pair", flow_run, n)]

        def timed(fn, per):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / per

        for _, fn, _ in forms:                                             # warm-up: code objects, arena growth
            fn()
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
        if have_both:
            spread = max(r[k + "_ms"]["max"] - r[k + "_ms"]["min"] for k in ("left", "right"))
            r["larger_spread_of_left_right_ms"] = spread
            for k in ("both_box_impl2", "both_box_impl1", "both_default", "both_composed", "flow_per_pair"):
                r[k + "_over_left_plus_right"] = med[k] / r["left_plus_right_ms"]
            r["default_form"] = out["default_form"]
            r["default_within_spread_of_left_plus_right"] = bool(med["both_default"] <= r["left_plus_right_ms"] + spread)
            r["pairs_in_flow"] = n
            same = lambda k: bool(torch.equal(out[k][0], out["left"]) and torch.equal(out[k][1], out["right"]))
            r["maps_equal_smt_sad"] = {k: same(k) for k in ("box2", "box1", "default", "composed")}
            r["flow_pair0_equals_smt_sad"] = bool(torch.equal(out["flow"][0][0], out["left"]) and
                                                  torch.equal(out["flow"][1][0], out["right"]))
            bad |= not (all(r["maps_equal_smt_sad"].values()) and r["flow_pair0_equals_smt_sad"])
            flow.close()
        r["samples"] = {k: [round(x, 4) for x in xs] for k, xs in t.items()}
        res["sizes"][f"{W}x{H}_d{D}_w{2 * ws + 3}"] = r
        print(name, json.dumps({k: v for k, v in r.items() if k != "samples"}), flush=True)
        out.clear()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if bad:
        print("MISMATCH", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
