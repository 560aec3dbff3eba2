"""Sub-pixel SAD (include/smt_sad_subpixel.h), timed three ways; device events around every call,
the forms alternating inside every round, 21 samples per form (7 rounds x 3; a form whose warm-up call takes more than
200 ms gets 7), median [min, max]:

  1. the sub-pixel calls -- smt_sad_both_subpixel as box + keys + k_sad_refine_right, as box + volume + diagonal, and
     composed of two smt_sad_subpixel calls; the two single views -- beside integer smt_sad_both in the same process;
  2. the flows per pair on --pairs pairs: smt_sad_flow_run_batch_subpixel against smt_sad_flow_run_batch;
  3. --ab PARENT_LIB: the integer entry points (smt_sad under both impls, smt_sad_both) of this build against another
     build's library (the parent commit's) in alternating child processes, this build first in half the rounds; the
     condition is that this build's median lies inside the other's own [min, max].

    python tools/sad_subpixel_time.py [--sizes driver9,hd9,hd45,driver181] [--pairs 8] [--ab path/to/parent/libsmt_hip.so]
                                      [--ab-rounds 6] [--out profiles/sad_subpixel_time.json]

k_sad_refine_right alone comes from a kernel trace of this tool (tools/prof_sad_subpixel.sh).
Sizes (W x H, D, winsize): driver9 450x375 60 3 (SADmain.cpp:33-34); hd9 1920x1080 128 3; hd45 1920x1080 128 21;
driver181 450x375 60 89 (the largest window of the box kernel)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"driver9": (375, 450, 60, 3), "hd9": (1080, 1920, 128, 3), "hd45": (1080, 1920, 128, 21), "driver181": (375, 450, 60, 89)}
AB_SIZES = ("driver9", "hd9", "hd45")
SLOW_MS = 200.0


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


def time_forms(forms, rounds, reps):
    """forms: [(key, fn, divisor)] -> {key: [ms]}: one warm-up pair of calls each, then the forms alternate inside every round"""
    import torch

    def timed(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / per

    slow = {}
    for k, fn, per in forms:                                   # warm-up: code objects, arena growth
        fn()
        slow[k] = timed(fn, 1) > SLOW_MS
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in forms}
    for _ in range(rounds):
        for k, fn, per in forms:
            for _ in range(1 if slow[k] else reps):
                t[k].append(timed(fn, per))
    return t


def setup(name, pairs):
    import numpy as np
    import torch
    from stereo_match_traditional_amd import synth
    dev = torch.device("cuda:0")
    H, W, D, ws = SIZES[name]
    imgs = [synth.synth_pair(H, W, D, 4 + b) for b in range(max(pairs, 1))]
    Lp = torch.from_numpy(np.pad(imgs[0][0], ws + 1, mode="edge")).to(dev)
    Rp = torch.from_numpy(np.pad(imgs[0][1], ws + 1, mode="edge")).to(dev)
    Lb = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
    Rb = torch.from_numpy(np.stack([x[1] for x in imgs])).to(dev)
    return H, W, D, ws, Lp, Rp, Lb, Rb


def integer_forms(smt, Lp, Rp, D, ws, out):
    def single(impl, view, key):
        def f():
            smt.sad_set_impl(impl)
            out[key] = (smt.GetPointDepthLeft if view == 0 else smt.GetPointDepthRight)(Lp, Rp, D, ws)
            smt.sad_set_impl(2)
        return f

    def both():
        out["int_both"] = smt.GetPointDepthBoth(Lp, Rp, D, ws)

    return [("int_left_impl2", single(2, 0, "l2"), 1), ("int_right_impl2", single(2, 1, "r2"), 1),
            ("int_left_impl1", single(1, 0, "l1"), 1), ("int_right_impl1", single(1, 1, "r1"), 1), ("int_both", both, 1)]


def child(a):
    """--integer-only: the integer entry points of whatever library SMT_HIP_LIB names; one JSON line"""
    import stereo_match_traditional_amd as smt
    res = {}
    for name in a.sizes.split(","):
        H, W, D, ws, Lp, Rp, _, _ = setup(name, 1)
        t = time_forms(integer_forms(smt, Lp, Rp, D, ws, {}), a.rounds, a.reps)
        res[name] = {k: [round(x, 4) for x in xs] for k, xs in t.items()}
    print("AB " + json.dumps(res), flush=True)


def ab(a):
    """alternating child processes of this tool; nothing here opens the GPU"""
    libs = {"this": None, "parent": os.path.abspath(a.ab)}
    samples = {n: {} for n in libs}
    for r in range(a.ab_rounds):
        for which in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            env = dict(os.environ)
            env.pop("SMT_HIP_LIB", None)
            if libs[which]:
                env["SMT_HIP_LIB"] = libs[which]
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--integer-only", "--sizes", ",".join(AB_SIZES),
                                "--rounds", "2", "--reps", "2"], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"{which} child failed:\n{p.stderr[-2000:]}")
            line = [x for x in p.stdout.splitlines() if x.startswith("AB ")][-1]
            for size, forms in json.loads(line[3:]).items():
                for k, xs in forms.items():
                    samples[which].setdefault(size, {}).setdefault(k, []).extend(xs)
    out = {}
    for size in samples["this"]:
        out[size] = {}
        for k in samples["this"][size]:
            t, p = stat(samples["this"][size][k]), stat(samples["parent"][size][k])
            out[size][k] = {"this_ms": t, "parent_ms": p, "this_median_inside_parent_min_max": bool(p["min"] <= t["median"] <= p["max"])}
        print("ab", size, json.dumps(out[size]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="driver9,hd9,hd45,driver181")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-rounds", type=int, default=6)
    ap.add_argument("--integer-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.integer_only:
        return child(a)
    res = {"note": "ms per call (flows: per pair), device events around each call; median [min, max, n] over rounds x reps; the forms "
                   "alternate inside every round; a form whose warm-up call took more than 200 ms has one sample per round", "sizes": {}}
    if a.ab:
        res["integer_paths_against_parent"] = ab(a)            # before this process opens the GPU
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    bad = False
    for name in a.sizes.split(","):
        H, W, D, ws, Lp, Rp, Lb, Rb = setup(name, a.pairs)
        out = {}

        def sub_both(key, dispatch, impl):
            def f():
                smt.sad_both_set_dispatch(dispatch); smt.sad_both_set_impl(impl)
                out[key] = smt.GetPointDepthBothSubpixel(Lp, Rp, D, ws, 1.0, want_winner=True)
                out[key + "_form"] = smt.sad_both_last_form()
                smt.sad_both_set_dispatch(0); smt.sad_both_set_impl(2)
            return f

        def sub_single(view, key):
            def f():
                out[key] = smt.GetPointDepthSubpixel(Lp, Rp, D, ws, view, 1.0)
            return f

        forms = [f for f in integer_forms(smt, Lp, Rp, D, ws, out) if f[0] == "int_both"]
        forms += [("sub_both_keys_refine", sub_both("keys", 1, 2), 1), ("sub_both_volume_diag", sub_both("volume", 1, 1), 1),
                  ("sub_both_composed", sub_both("composed", 2, 2), 1), ("sub_both_default", sub_both("default", 0, 2), 1),
                  ("sub_left", sub_single(1, "sl"), 1), ("sub_right", sub_single(2, "sr"), 1)]
        flow = None
        if a.pairs > 0:
            flow = smt.SADFlow(H, W, D, torch.device("cuda:0"), winsize=ws)
            forms += [("flow_int_per_pair", lambda: out.__setitem__("fi", flow.run(Lb, Rb)), a.pairs),
                      ("flow_sub_per_pair", lambda: out.__setitem__("fs", flow.run_subpixel(Lb, Rb)), a.pairs)]
        t = time_forms(forms, a.rounds, a.reps)
        r = {k + "_ms": stat(xs) for k, xs in t.items()}
        med = {k: r[k + "_ms"]["median"] for k in t}
        for k in ("sub_both_keys_refine", "sub_both_volume_diag", "sub_both_composed", "sub_both_default"):
            r[k + "_over_int_both"] = med[k] / med["int_both"]
        r["keys_refine_over_composed"] = med["sub_both_keys_refine"] / med["sub_both_composed"]
        r["keys_refine_over_volume_diag"] = med["sub_both_keys_refine"] / med["sub_both_volume_diag"]
        r["default_form"] = out["default_form"]
        if flow is not None:
            r["flow_sub_over_flow_int"] = med["flow_sub_per_pair"] / med["flow_int_per_pair"]
            r["pairs_in_flow"] = a.pairs
        eq = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
        r["forms_bit_equal"] = {k: all(eq(out[k][j], out["keys"][j]) for j in range(4)) for k in ("volume", "composed", "default")}
        r["single_views_bit_equal"] = eq(out["sl"], out["keys"][0]) and eq(out["sr"], out["keys"][1])
        r["winners_equal_integer_maps"] = eq(out["keys"][2], out["int_both"][0]) and eq(out["keys"][3], out["int_both"][1])
        bad |= not (all(r["forms_bit_equal"].values()) and r["single_views_bit_equal"] and r["winners_equal_integer_maps"])
        if flow is not None:
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
