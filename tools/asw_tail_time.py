"""Cost of the tail of ASW/ASWeight.cpp (:67-78) on the device (run under a time limit, e.g.
`timeout -k 10 600 python tools/asw_tail_time.py --out profiles/asw_tail_time.json`):

  a  smt_asw_tail_batch alone (normalize, filterSpeckles, medianBlur 5, FillImageNew, medianBlur 3; both optional copies
     off) on 8 and 64 maps at 450x375 and 1920x1080, and each of its primitives on the same maps (event time)
  b  ASWFlow.run_post against ASWFlow.run per pair at 450x375 D=60, window 25x25 (winSize 11), 8 pairs (event time)

The maps are cross-check-like: smooth disparities 5..59 with 25 % rejected (0) and an occluded band at the left edge.
Rounds interleave the legs: two warm-up rounds, then --rounds timed ones; every figure is median [min-max].  --dry-run
stops after input generation (no GPU needed).  Prints one JSON object; --out FILE also writes it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereo_match_traditional_amd import synth  # noqa: E402

SIZES = ((450, 375), (1920, 1080))                     # W x H
MAPS = (8, 64)
FLOW = (450, 375, 60, 11)                              # W, H, D, winSize


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def maps_for(w, h, n):
    rng = np.random.default_rng(w + h)
    y, x = np.mgrid[0:h, 0:w]
    base = (5 + (x * 40) // w + (y * 14) // h).astype(np.uint8)
    m = np.repeat(base[None], n, axis=0)
    m[rng.random((n, h, w)) < 0.25] = 0
    m[:, :, : w // 8] = 0
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
    maps = {(w, h): maps_for(w, h, max(MAPS)) for w, h in SIZES}
    fw, fh, fd, fwin = FLOW
    prs = [synth.synth_pair(fh, fw, fd, 3 + b) for b in range(a.flow_pairs)]
    L, R = np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])
    if a.dry_run:
        print(json.dumps({"dry_run": True, "rounds": a.rounds, "sizes": ["%dx%d" % s for s in SIZES], "maps": MAPS,
                          "holes": {"%dx%d" % k: int((v == 0).sum()) for k, v in maps.items()},
                          "flow": "%dx%d D=%d winSize=%d" % FLOW, "flow_pairs": a.flow_pairs}))
        return

    import torch
    import stereo_match_traditional_amd as smt
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()

    def event_ms(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        f()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    legs = {"tail": lambda m: smt.ASWTail(m),
            "normalize": lambda m: smt.MinMaxNormalizeU8(m, out=m),
            "filter_speckles": lambda m: smt.FilterSpecklesU8(m, 0, 40, 2),
            "median5": lambda m: smt.MedianBlurU8(m, 5),
            "fill_image_new": lambda m: smt.FillImageNew(m),
            "median3": lambda m: smt.MedianBlurU8(m, 3)}
    cases = []
    for (w, h) in SIZES:
        for n in MAPS:
            src = torch.from_numpy(maps[(w, h)][:n]).to(dev)
            cases.append(dict(w=w, h=h, n=n, src=src, work=torch.empty_like(src), t={k: [] for k in legs}))
    flow = smt.ASWFlow(fh, fw, fd, dev, winSize=fwin)
    gl, gr = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    ft = {"run": [], "run_post": []}
    counts = {}

    for r in range(a.rounds + 2):                                     # two warm-up rounds
        for c in cases:
            for k, f in legs.items():
                c["work"].copy_(c["src"])
                ms = event_ms(lambda: f(c["work"]))
                if r >= 2:
                    c["t"][k].append(ms)
            if r == 0:
                c["work"].copy_(c["src"])
                counts[(c["w"], c["h"], c["n"])] = smt.ASWTail(c["work"])[1].sum(0).tolist()
        if r % 2 == 0:                                                # the two legs swap places from round to round
            tr = event_ms(lambda: flow.run(gl, gr))
            tp = event_ms(lambda: flow.run_post(gl, gr))
        else:
            tp = event_ms(lambda: flow.run_post(gl, gr))
            tr = event_ms(lambda: flow.run(gl, gr))
        flow.status()
        if r >= 2:
            ft["run"].append(tr)
            ft["run_post"].append(tp)
    flow.close()

    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "tail": [], "flow": None}
    for c in cases:
        e = {"W": c["w"], "H": c["h"], "maps": c["n"], "fill_counts_sum": counts[(c["w"], c["h"], c["n"])]}
        for k, v in c["t"].items():
            e[k + "_ms"] = stats(v)
        e["tail_us_per_map"] = e["tail_ms"]["median"] * 1e3 / c["n"]
        res["tail"].append(e)
    P = gl.shape[0]
    run, post = stats(ft["run"]), stats(ft["run_post"])
    res["flow"] = {"W": fw, "H": fh, "D": fd, "winSize": fwin, "pairs": P, "run_ms": run, "run_post_ms": post,
                   "run_ms_per_pair": run["median"] / P, "run_post_ms_per_pair": post["median"] / P,
                   "tail_ms_per_pair": (post["median"] - run["median"]) / P}
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as fh_:
            fh_.write(out + "\n")


if __name__ == "__main__":
    main()
