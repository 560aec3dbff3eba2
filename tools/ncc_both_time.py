"""Both NCC views from one cost pass (smt_lrncc, NCCFlow.run_both) against what a caller had before: two smt_ncc calls, the
left one and one on pre-flipped images (the flips outside the timed region).  Interleaved in one process: device events
around every call, 21 samples per form, median [min - max]; the forms alternate inside every round and their maps are
compared in the same run.

    python tools/ncc_both_time.py [--out profiles/ncc_both_time.json] [--parent-lib PATH] [--dry-run]

Cases (450 x 375 throughout): D = 64 at 9x9, 21x21 and 31x31, D = 200 at 21x21 -- each under smt_ncc impl 2 (dot4) and
impl 3 (box) --, D = 64 at 45x45 (box only), and the 8-pair flow at 21x21, D = 200 (default rule and box form).  Per case:
KEYS (smt_lrncc_set_impl(2)), COMPOSED (1) and the baseline.
Regression guard (--parent-lib: the parent commit's libsmt_hip.so): default smt_ncc at 21x21, D = 64 and D = 200, and
NCCFlow.run on 8 pairs at D = 200, in alternating child processes, this tree's library against the parent's
(SMT_HIP_LIB); the child is this file with --guard-child.  The new median must sit inside the parent's own [min - max].

--dry-run stops after the inputs are generated (no GPU needed)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 375, 450
SAMPLES = 21
CASES = [(64, 4, 2), (64, 4, 3), (64, 10, 2), (64, 10, 3), (64, 15, 2), (64, 15, 3), (200, 10, 2), (200, 10, 3), (64, 22, 3)]   # (D, winSize, impl)
FLOW = dict(D=200, win=10, pairs=8)
GUARD = [(64, 10), (200, 10)]


def inputs():
    import numpy as np
    from stereo_match_traditional_amd import synth
    pairs = [synth.synth_pair(H, W, 64, 4 + b) for b in range(FLOW["pairs"])]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "samples": [round(x, 4) for x in xs]}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def interleave(torch, forms, per=1):
    """forms: {name: callable}; two warm-up calls each, then SAMPLES rounds with the forms alternating"""
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(SAMPLES):
        for k, fn in forms.items():
            t[k].append(timed(torch, fn) / per)
    return {k: stat(xs) for k, xs in t.items()}


def brief(r):
    return json.dumps({k: (v if not isinstance(v, dict) else [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)]) for k, v in r.items()})


def guard_child():
    """default smt_ncc and NCCFlow.run at the guard sizes with whatever library SMT_HIP_LIB names; one JSON line"""
    import torch
    import stereo_match_traditional_amd as smt
    Ls, Rs = inputs()
    dev = torch.device("cuda:0")
    L, R = torch.from_numpy(Ls[0]).to(dev), torch.from_numpy(Rs[0]).to(dev)
    Lb, Rb = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
    out = {}
    for D, win in GUARD:
        r = interleave(torch, {"default": lambda: smt.NCC_algorithem(L, R, win, D)})
        out[f"smt_ncc_d{D}_w{2 * win + 1}"] = r["default"]
    flow = smt.NCCFlow(H, W, FLOW["D"], dev, winSize=FLOW["win"])
    r = interleave(torch, {"flow": lambda: flow.run(Lb, Rb)}, per=FLOW["pairs"])
    out[f"flow_run_d{FLOW['D']}_w{2 * FLOW['win'] + 1}_per_pair"] = r["flow"]
    flow.close()
    print(json.dumps(out))


def guard(parent_lib, rounds=3):
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for who in ("parent", "this"):
            env = dict(os.environ)
            env.pop("SMT_HIP_LIB", None)
            if who == "parent":
                env["SMT_HIP_LIB"] = parent_lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--guard-child"], env=env, capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"guard child ({who}) failed with {r.returncode}:\n{r.stderr[-2000:]}")
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"note": "default smt_ncc (impl 2) and NCCFlow.run, ms per call / per pair; alternating child processes, %d per "
                   "library, %d samples each" % (rounds, SAMPLES)}
    for key in runs["this"][0]:
        both = {}
        for who in runs:
            xs = [x for r in runs[who] for x in r[key]["samples"]]
            both[who] = stat(xs)
            both[who]["process_medians"] = [r[key]["median"] for r in runs[who]]
        both["this_median_inside_parent_min_max"] = bool(both["parent"]["min"] <= both["this"]["median"] <= both["parent"]["max"])
        res[key] = both
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--guard-child", action="store_true")
    a = ap.parse_args()
    if a.guard_child:
        return guard_child()
    Ls, Rs = inputs()
    if a.dry_run:
        print(json.dumps({"dry_run": True, "pairs": int(Ls.shape[0]), "H": H, "W": W}))
        return
    # the guard's child processes run before this process opens the GPU: one process on the device at a time
    guard_res = guard(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    import torch
    import stereo_match_traditional_amd as smt
    dev = torch.device("cuda:0")
    L, R = torch.from_numpy(Ls[0]).to(dev), torch.from_numpy(Rs[0]).to(dev)
    fL, fR = torch.flip(R, [1]).contiguous(), torch.flip(L, [1]).contiguous()          # the mirrored pair, made once
    Lb, Rb = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
    fLb, fRb = torch.flip(Rb, [2]).contiguous(), torch.flip(Lb, [2]).contiguous()
    res = {"note": "ms per call (flow: per pair), device events around each call; median, min, max of %d samples; the forms "
                   "alternate inside every round; baseline = smt_ncc on the pair + smt_ncc on the pre-flipped pair" % SAMPLES,
           "size": f"{W}x{H}", "single": {}, "flow": {}}
    bad = False
    for D, win, impl in CASES:
        out = {}

        def both(lr, key):
            def f():
                smt.ncc_set_impl(impl); smt.lrncc_set_impl(lr)
                out[key] = smt.NCC_both(L, R, win, D)
                out[key + "_form"] = smt.lrncc_last_form()
                smt.ncc_set_impl(2); smt.lrncc_set_impl(0)
            return f

        def base():
            smt.ncc_set_impl(impl)
            out["base"] = (smt.NCC_algorithem(L, R, win, D), smt.NCC_algorithem(fL, fR, win, D))
            smt.ncc_set_impl(2)

        r = interleave(torch, {"keys": both(2, "keys"), "composed": both(1, "composed"), "baseline": base})
        r["keys_over_baseline"] = r["keys"]["median"] / r["baseline"]["median"]
        r["composed_over_baseline"] = r["composed"]["median"] / r["baseline"]["median"]
        r["keys_median_below_baseline_min"] = bool(r["keys"]["median"] < r["baseline"]["min"])
        r["forms"] = [out["keys_form"], out["composed_form"]]
        want = (out["base"][0], torch.flip(out["base"][1], [1]))
        r["maps_equal"] = bool(all(torch.equal(out[k][v], want[v]) for k in ("keys", "composed") for v in (0, 1)))
        bad |= not r["maps_equal"]
        key = f"d{D}_w{2 * win + 1}_impl{impl}"
        res["single"][key] = r
        print(key, brief(r), flush=True)
    D, win, P = FLOW["D"], FLOW["win"], FLOW["pairs"]
    for name, form in (("default", 0), ("box", smt.NCC_FORM_BOX)):
        flow = smt.NCCFlow(H, W, D, dev, winSize=win).set_form(form)
        out = {}

        def fboth(lr, key):
            def f():
                smt.lrncc_set_impl(lr)
                out[key] = flow.run_both(Lb, Rb, want=("dispL", "dispR"))[:2]
                out[key + "_form"] = smt.lrncc_last_form()
                smt.lrncc_set_impl(0)
            return f

        def fbase():
            out["base"] = (flow.run(Lb, Rb), flow.run(fLb, fRb))
            out["left_form"] = smt.ncc_last_form()

        r = interleave(torch, {"keys": fboth(2, "keys"), "composed": fboth(1, "composed"), "baseline": fbase}, per=P)
        r["keys_over_baseline"] = r["keys"]["median"] / r["baseline"]["median"]
        r["composed_over_baseline"] = r["composed"]["median"] / r["baseline"]["median"]
        r["keys_median_below_baseline_min"] = bool(r["keys"]["median"] < r["baseline"]["min"])
        r["forms"] = [out["keys_form"], out["composed_form"]]
        r["left_form"] = out["left_form"]
        want = (out["base"][0], torch.flip(out["base"][1], [2]))
        r["maps_equal"] = bool(all(torch.equal(out[k][v], want[v]) for k in ("keys", "composed") for v in (0, 1)))
        bad |= not r["maps_equal"]
        r["pairs"] = P
        res["flow"][f"d{D}_w{2 * win + 1}_{name}"] = r
        print("flow", name, brief(r), flush=True)
        flow.close()
    if guard_res is not None:
        res["regression_guard"] = guard_res
        print("guard", json.dumps({k: (v if not isinstance(v, dict) else {w: [v[w]["median"], v[w]["min"], v[w]["max"]] for w in ("this", "parent")} | {"inside": v["this_median_inside_parent_min_max"]})
                                   for k, v in res["regression_guard"].items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if bad:
        print("MISMATCH", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
