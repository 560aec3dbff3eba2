"""Cost of MedianFilter(d, d, ...) -- the in-place call of CBLSM.cpp:162 -- on batches of maps, and of the CBLSM.cpp
tail on the CBLSM flow (run under a time limit, e.g.
`timeout -k 10 900 python tools/median_inplace_time.py --out profiles/median_inplace_time.json`):

  a  smt_median_filter_inplace_batch, impl 0 (rings in LDS) and impl 1 (plain), window 3, at 450x375, 1242x375 and
     1920x1080 for 1, 8 and 32 maps (event time)
  b  what a caller does without it: the maps device to host (pinned), the host's MedianFilter in place
     (smt_median_filter_inplace_host: the schedule's host twin, one thread; the faster of its two formulations
     there), host to device (wall time)
  c  smt_median_filter_batch out of place, for scale only: it computes something else (event time)
  d  CBLSMFlow.run_post against CBLSMFlow.run per pair at 450x375 D=60 and 1242x375 D=128, 8 pairs (event time)

The maps are integers 0..59 with 15 % +inf.  a and b must give equal bits before anything is timed.  Rounds interleave
the legs: two warm-up rounds, then --rounds timed ones; every figure is median [min-max].  Next to each kernel time stand
the step count (H - 1) * (r + 1) + W and the time per step.  --dry-run stops after input generation (no GPU needed).
Prints one JSON object; --out FILE also writes it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereo_match_traditional_amd import synth  # noqa: E402

SIZES = ((450, 375), (1242, 375), (1920, 1080))        # W x H
PAIRS = (1, 8, 32)
FLOWS = ((450, 375, 60), (1242, 375, 128))             # W, H, D
WND = 3


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def maps_for(w, h, pairs):
    rng = np.random.default_rng(w + h)
    m = rng.integers(0, 60, (pairs, h, w)).astype(np.float32)
    m[rng.random((pairs, h, w)) < 0.15] = np.inf
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--flow-pairs", type=int, default=8)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    maps = {(w, h): maps_for(w, h, max(PAIRS)) for w, h in SIZES}
    flows = {}
    for w, h, d in FLOWS:
        prs = [synth.synth_pair(h, w, d, 3 + b) for b in range(a.flow_pairs)]
        flows[(w, h, d)] = (np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs]))
    if a.dry_run:
        print(json.dumps({"dry_run": True, "rounds": a.rounds, "sizes": ["%dx%d" % s for s in SIZES], "pairs": PAIRS,
                          "inf_pixels": {"%dx%d" % k: int(np.isinf(v).sum()) for k, v in maps.items()},
                          "flows": ["%dx%d D=%d" % f for f in FLOWS], "flow_pairs": a.flow_pairs}))
        return

    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd._lib import lib, check
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    host_fn = lib().smt_median_filter_inplace_host_ex
    host_fn.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]

    def event_ms(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        f()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    cases = []
    for (w, h) in SIZES:
        for P in PAIRS:
            src = torch.from_numpy(maps[(w, h)][:P]).to(dev)
            cases.append(dict(w=w, h=h, P=P, src=src, work=torch.empty_like(src), out=torch.empty_like(src),
                              pin=torch.empty((P, h, w), dtype=torch.float32).pin_memory(),
                              t={"impl0": [], "impl1": [], "host_roundtrip": [], "out_of_place": []}))
    fl = []
    for (w, h, d), (L, R) in flows.items():
        fl.append(dict(w=w, h=h, d=d, flow=smt.CBLSMFlow(h, w, d, dev), L=torch.from_numpy(L).to(dev),
                       R=torch.from_numpy(R).to(dev), t={"run": [], "run_post": []}))

    def inplace(c, impl):
        smt.median_inplace_set_impl(impl)
        c["work"].copy_(c["src"])
        ms = event_ms(lambda: smt.MedianFilterInPlace(c["work"], WND))
        smt.median_inplace_set_impl(0)
        return ms

    def roundtrip(c):
        c["work"].copy_(c["src"])
        torch.cuda.synchronize()
        t = time.perf_counter()
        c["pin"].copy_(c["work"])                                     # D2H (synchronises)
        a_ = c["pin"].numpy()
        check(host_fn(a_.ctypes.data_as(C.c_void_p), c["P"], 0, c["w"], c["h"], WND, 0, 0, 0), "host median")
        c["work"].copy_(c["pin"], non_blocking=True)                  # H2D
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for r in range(a.rounds + 2):                                     # two warm-up rounds
        for c in cases:
            t0 = inplace(c, 0)
            ref = c["work"].clone()
            t1 = inplace(c, 1)
            if r == 0 and not torch.equal(c["work"].view(torch.int32), ref.view(torch.int32)):
                raise SystemExit("impl 0 and impl 1 differ at %dx%d x%d" % (c["w"], c["h"], c["P"]))
            tb = roundtrip(c)
            if r == 0 and not torch.equal(c["work"].view(torch.int32), ref.view(torch.int32)):
                raise SystemExit("device and host differ at %dx%d x%d" % (c["w"], c["h"], c["P"]))
            tc = event_ms(lambda: check(lib().smt_median_filter_batch(
                C.c_void_p(c["src"].data_ptr()), C.c_void_p(c["out"].data_ptr()), c["P"], C.c_size_t(0), c["w"], c["h"], WND,
                C.c_void_p(st.cuda_stream)), "smt_median_filter_batch"))
            if r >= 2:
                for k, v in (("impl0", t0), ("impl1", t1), ("host_roundtrip", tb), ("out_of_place", tc)):
                    c["t"][k].append(v)
        for f in fl:
            tr = event_ms(lambda: f["flow"].run(f["L"], f["R"]))
            tp = event_ms(lambda: f["flow"].run_post(f["L"], f["R"]))
            f["flow"].status()
            if r >= 2:
                f["t"]["run"].append(tr)
                f["t"]["run_post"].append(tp)

    res = {"device": torch.cuda.get_device_name(0), "window": WND, "rounds": a.rounds, "median_inplace": [], "flows": []}
    for c in cases:
        steps = (c["h"] - 1) * (WND // 2 + 1) + c["w"]
        e = {"W": c["w"], "H": c["h"], "maps": c["P"], "steps": steps}
        for k, v in c["t"].items():
            e[k + "_ms"] = stats(v)
        for k in ("impl0", "impl1"):
            e[k + "_us_per_step"] = e[k + "_ms"]["median"] * 1e3 / steps
        e["impl0_below_host_roundtrip"] = bool(e["impl0_ms"]["median"] < e["host_roundtrip_ms"]["median"])
        res["median_inplace"].append(e)
    for f in fl:
        P = f["L"].shape[0]
        run, post = stats(f["t"]["run"]), stats(f["t"]["run_post"])
        res["flows"].append({"W": f["w"], "H": f["h"], "D": f["d"], "pairs": P, "run_ms": run, "run_post_ms": post,
                             "run_ms_per_pair": run["median"] / P, "run_post_ms_per_pair": post["median"] / P,
                             "tail_ms_per_pair": (post["median"] - run["median"]) / P})
        f["flow"].close()
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
