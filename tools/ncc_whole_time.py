"""NCC.h's whole-image ncc() on the device: the integer form against the loop nest of the same entry, and the both-view
flow against two single-view calls, interleaved in one process: device events around every call, 21 samples per form,
median [min - max]; the forms alternate inside every round and their maps are compared in the same run.

    python tools/ncc_whole_time.py [--out profiles/ncc_whole_time.json] [--only KEY] [--dry-run]

Sizes: 450x375 k = 5 O = 79 (the reference's own), 1242x375 O = 128, 1920x1080 O = 192, and k = 15 at 450x375.
Comparisons at each size: form 2 (INT) against form 1 (LOOP) of smt_whole_ncc, left type; NCCWholeFlow on one pair against
two single-view calls; NCCWholeFlow on 8 pairs, per pair; at 450x375 also the INT form with the float64 cost volume (the
torch.full that prefills the volume is inside the timed call).  The loop nest is sampled 5 times where one call takes longer
than 50 ms (its samples are recorded as they are).  No shared-cost flow exists, so there is none to compare.

--dry-run stops after the inputs are generated (no GPU needed)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLES = 21
PAIRS = 8
SIZES = {"450x375_k5_O79": (375, 450, 5, 79), "1242x375_k5_O128": (375, 1242, 5, 128), "1920x1080_k5_O192": (1080, 1920, 5, 192),
         "450x375_k15_O79": (375, 450, 15, 79)}


def inputs(H, W, O):
    import numpy as np
    from stereo_match_traditional_amd import synth
    pairs = [synth.synth_pair(H, W, min(O, 64), 4 + b) for b in range(PAIRS)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "samples": [round(x, 4) for x in xs]}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def interleave(torch, forms, per=None, samples=SAMPLES):
    """forms: {name: callable}; two warm-up calls each, then `samples` rounds with the forms alternating"""
    per = per or {}
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(samples):
        for k, fn in forms.items():
            t[k].append(timed(torch, fn) / per.get(k, 1))
    return {k: stat(xs) for k, xs in t.items()}


def brief(r):
    return json.dumps({k: (v if not isinstance(v, dict) else [round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)]) for k, v in r.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    sizes = {k: v for k, v in SIZES.items() if a.only in (None, k)}
    if a.dry_run:
        for key, (H, W, k, O) in sizes.items():
            Ls, _ = inputs(H, W, O)
            print(json.dumps({"dry_run": True, "size": key, "pairs": int(Ls.shape[0])}))
        return
    import torch
    import stereo_match_traditional_amd as smt
    dev = torch.device("cuda:0")
    res = {"note": "ms per call (8-pair flow: per pair), device events around each call; median, min, max of %d samples (the loop "
                   "nest: 5 where a call exceeds 50 ms); the forms alternate inside every round" % SAMPLES, "sizes": {}}
    bad = False
    for key, (H, W, k, O) in sizes.items():
        Ls, Rs = inputs(H, W, O)
        L, R = torch.from_numpy(Ls[0]).to(dev), torch.from_numpy(Rs[0]).to(dev)
        Lb, Rb = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
        out = {}

        def single(impl, key_, types=("left",)):
            def f():
                smt.ncc_whole_set_impl(impl)
                out[key_] = [smt.ncc(L, R, t, kernel_size=k, max_offset=O, want_offset=True)[1] for t in types]
                smt.ncc_whole_set_impl(0)
            return f

        probe = timed(torch, single(1, "probe"))                # the first call also warms the arena
        probe = timed(torch, single(1, "probe"))
        r = {"loop_probe_ms": probe}
        slow = probe > 50.0
        r.update(interleave(torch, {"int": single(2, "int"), "loop": single(1, "loop")}, samples=5 if slow else SAMPLES))
        r["int_over_loop"] = r["int"]["median"] / r["loop"]["median"]
        diff = int((out["int"][0] != out["loop"][0]).sum().item())
        r["maps_differ_at"] = diff                              # near-ties may differ between the forms (the tests' excuse rule)
        r["loop_runs_of_offsets"] = smt.ncc_whole_last_groups()     # of the last call above, the loop nest's
        if key.startswith("450x375"):                           # the diagnostic cost volume: strided stores under INT

            def with_cost():
                smt.ncc_whole_set_impl(2)
                out["cost"] = smt.ncc(L, R, "left", kernel_size=k, max_offset=O, want_cost=True)[1]
                smt.ncc_whole_set_impl(0)

            r["int_with_cost"] = interleave(torch, {"int_with_cost": with_cost})["int_with_cost"]
            r["with_cost_over_maps_only"] = r["int_with_cost"]["median"] / r["int"]["median"]
        flow = smt.NCCWholeFlow(H, W, dev, kernel_size=k, max_offset=O)

        def flow1():
            out["flow1"] = flow.run(L, R, want=("offL", "offR"))

        def flow8():
            out["flow8"] = flow.run(Lb, Rb, want=("offL", "offR"))

        f = interleave(torch, {"two_single_calls": single(0, "two", ("left", "right")), "flow_1_pair": flow1, "flow_8_pairs": flow8},
                       per={"flow_8_pairs": PAIRS})
        r.update(f)
        r["flow_over_two_calls"] = f["flow_1_pair"]["median"] / f["two_single_calls"]["median"]
        r["flow8_per_pair_over_two_calls"] = f["flow_8_pairs"]["median"] / f["two_single_calls"]["median"]
        r["default_form"] = smt.ncc_whole_last_form()
        same = torch.equal(out["flow1"][2][0], out["two"][0]) and torch.equal(out["flow1"][3][0], out["two"][1]) and \
            torch.equal(out["flow8"][2][0], out["two"][0]) and torch.equal(out["flow8"][3][0], out["two"][1])
        r["flow_equals_single_calls"] = bool(same)
        bad |= not same
        flow.close()
        res["sizes"][key] = r
        print(key, brief(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if bad:
        print("MISMATCH", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
