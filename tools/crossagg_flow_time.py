"""smt_crossagg_flow_run_batch two ways on one pair of handles, interleaved in one process: impl 1, the composed path
(smt_cblsm_ad, eight aggregation passes, smt_wta per pair and view: 72 B per hypothesis), against impl 0, the fused
kernels (first horizontal pass from the gray rows, WTA inside the last dividing pass, no volume store for all pairs
but the last: 56 / 52 B per hypothesis).  Device events around every batch call, ms per pair; median [min-max] over
the samples; maps and last-pair volumes of the two forms are compared in the same run.

    python tools/crossagg_flow_time.py [--sizes 720p,cblsm] [--samples 21] [--pairs 8] [--out profiles/crossagg_flow_time.json]
    python tools/crossagg_flow_time.py --dry-run        # stops after input generation (no GPU)

Sizes: 1280x720 D=128 (the size of the CrossAggregator figure, profiles/r2f), 450x375 D=60 (CBLSM.cpp:28-32)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"720p": (720, 1280, 128), "cblsm": (375, 450, 60)}


def inputs(H, W, D, n):
    """n gray pairs (synth.synth_pair) and BGR images = gray + per-channel (byte mod 3), the oracle's synth_bgr."""
    import numpy as np
    from stereo_match_traditional_amd import synth
    L, R, bL, bR = [], [], [], []
    for b in range(n):
        l, r = synth.synth_pair(H, W, D, 50 + b)
        for g, dst, seed in ((l, bL, 150 + b), (r, bR, 250 + b)):
            off = (synth.lcg_bytes(seed, H * W * 3)[0] % 3).reshape(H, W, 3).astype(np.int32)
            dst.append(np.clip(g.astype(np.int32)[..., None] + off, 0, 255).astype(np.uint8))
        L.append(l)
        R.append(r)
    return tuple(np.stack(x) for x in (L, R, bL, bR))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="720p,cblsm")
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    import numpy as np
    data = {name: inputs(*SIZES[name], a.pairs) for name in a.sizes.split(",")}
    if a.dry_run:
        print(json.dumps({name: [list(x.shape) for x in v] for name, v in data.items()}))
        return
    import torch
    import stereo_match_traditional_amd as smt
    dev = torch.device("cuda:0")
    try:
        head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        head = None
    res = {"note": "ms per pair, device events around each batch call of %d pairs; median [min, max] over %d interleaved "
                   "samples; impl 1 = composed path, impl 0 = fused kernels" % (a.pairs, a.samples),
           "git_head": head, "num_iters": a.iters, "sizes": {}}
    bad = False
    for name, arrs in data.items():
        H, W, D = SIZES[name]
        L, R, bL, bR = (torch.from_numpy(x).to(dev) for x in arrs)
        flows = {impl: smt.CrossAggFlow(H, W, D, dev, num_iters=a.iters).set_impl(impl) for impl in (1, 0)}
        entry = {"pairs": a.pairs}
        for views, vname in ((smt.VIEW_LEFT, "left"), (smt.VIEW_BOTH, "both")):
            dl = {impl: torch.zeros((a.pairs, H, W), dtype=torch.float32, device=dev) for impl in flows}
            dr = {impl: torch.zeros((a.pairs, H, W), dtype=torch.float32, device=dev) for impl in flows}

            def timed(impl):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                flows[impl].run(bL, bR, L, R, views=views, dispL=dl[impl], dispR=dr[impl])
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / a.pairs

            for impl in flows:                                            # warm-up: code objects, first touches
                timed(impl)
            t = {1: [], 0: []}
            for _ in range(a.samples):
                for impl in (1, 0):
                    t[impl].append(timed(impl))
            v = {impl: flows[impl].volumes() for impl in flows}
            equal = bool(torch.equal(dl[0], dl[1]) and torch.equal(dr[0], dr[1]))
            vol_equal = bool(torch.equal(v[0][0].view(torch.int32), v[1][0].view(torch.int32)) and
                             (views != smt.VIEW_BOTH or torch.equal(v[0][1].view(torch.int32), v[1][1].view(torch.int32))))
            st = {k: {"median": float(np.median(x)), "min": min(x), "max": max(x)} for k, x in t.items()}
            entry[vname] = {"composed_ms_per_pair": st[1], "fused_ms_per_pair": st[0],
                            "speedup": st[1]["median"] / st[0]["median"], "maps_equal": equal,
                            "last_pair_volumes_equal": vol_equal,
                            "samples": {"composed": [round(x, 4) for x in t[1]], "fused": [round(x, 4) for x in t[0]]}}
            print(name, vname, "composed %.3f [%.3f-%.3f]  fused %.3f [%.3f-%.3f] ms/pair  x%.3f  equal %s %s" % (
                st[1]["median"], st[1]["min"], st[1]["max"], st[0]["median"], st[0]["min"], st[0]["max"],
                entry[vname]["speedup"], equal, vol_equal), flush=True)
            bad = bad or not equal or not vol_equal
        res["sizes"]["%dx%d_d%d" % (W, H, D)] = entry
        for f in flows.values():
            f.close()
        del L, R, bL, bR, flows
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
