"""CBLSM.cpp's active flow two ways, interleaved in one process: the composed single calls (two crossarm handles,
smt_cblsm_ad for both views, four smt_crossarm_aggregate(order 1), six caller-held volumes -- host/cblsm_main.cpp's
sequence) against smt_cblsm_flow_run_batch (summed-area first pass, three volumes).  Device events around every batch
call, ms per pair; medians and spread over the rounds; the maps of the two forms are compared in the same run.

    python tools/cblsm_time.py [--sizes small,kitti,1080p] [--rounds 5] [--reps 3] [--out profiles/cblsm_time.json]

Sizes: 450x375 D=60 (CBLSM.cpp:28-32's class, 64 pairs), 1242x375 D=128 (16 pairs), 1920x1080 D=192 (4 pairs)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"small": (375, 450, 60, 64), "kitti": (375, 1242, 128, 16), "1080p": (1080, 1920, 192, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,kitti,1080p")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    from stereo_match_traditional_amd._lib import lib, check, CrossArmParams
    L_ = lib()
    dev = torch.device("cuda:0")
    P = lambda t: C.c_void_p(t.data_ptr())
    res = {"note": "ms per pair, device events around each batch call; median [min, max] over rounds x reps",
           "sizes": {}}
    for name in a.sizes.split(","):
        H, W, D, n = SIZES[name]
        imgs = [synth.synth_pair(H, W, D, 50 + b) for b in range(n)]
        Lb = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
        Rb = torch.from_numpy(np.stack([x[1] for x in imgs])).to(dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # composed: two crossarm handles with CBLSM.cpp's constants, six caller-held volumes
        cp = CrossArmParams()
        L_.smt_crossarm_cblsm_params(C.byref(cp))
        ca = [C.c_void_p(), C.c_void_p()]
        for h in ca:
            check(L_.smt_crossarm_create_on(0, H, W, D, C.byref(cp), C.byref(h)), "smt_crossarm_create_on")
            check(L_.smt_crossarm_set_stream(h, st), "smt_crossarm_set_stream")
        vols = [torch.empty((H, W, D), dtype=torch.float32, device=dev) for _ in range(6)]
        cdl = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        cdr = torch.empty_like(cdl)

        def composed():
            adl, adr, cl, cr, cl2, cr2 = vols
            for b in range(n):
                check(L_.smt_crossarm_arms(ca[0], P(Lb[b]), 1), "arms L")                          # :64-67
                check(L_.smt_crossarm_arms(ca[1], P(Rb[b]), 1), "arms R")                          # :101-104
                check(L_.smt_cblsm_ad(P(Lb[b]), P(Rb[b]), H, W, D, smt.VIEW_LEFT, P(adl), st), "ad L")     # :133
                check(L_.smt_cblsm_ad(P(Lb[b]), P(Rb[b]), H, W, D, smt.VIEW_RIGHT, P(adr), st), "ad R")    # :134
                check(L_.smt_crossarm_aggregate(ca[1], P(adr), P(cr), 1, None), "agg R")           # :146
                check(L_.smt_crossarm_aggregate(ca[0], P(adl), P(cl), 1, None), "agg L")           # :147
                check(L_.smt_crossarm_aggregate(ca[0], P(cl), P(cl2), 1, P(cdl[b])), "agg L2")     # :149, :152
                check(L_.smt_crossarm_aggregate(ca[0], P(cr), P(cr2), 1, P(cdr[b])), "agg R2")     # :150, :153

        flow = smt.CBLSMFlow(H, W, D, dev)
        out = {}

        def batch():
            out["maps"] = flow.run(Lb, Rb)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / n

        composed(); batch(); torch.cuda.synchronize()                     # warm-up: code objects, first touches
        t = {"composed": [], "batch": []}
        for _ in range(a.rounds):
            for k, fn in (("composed", composed), ("batch", batch)):
                for _ in range(a.reps):
                    t[k].append(timed(fn))
        flow.status()
        for h in ca:
            check(L_.smt_crossarm_status(h), "smt_crossarm_status")
        dl, dr = out["maps"]
        equal = bool(torch.equal(dl, cdl) and torch.equal(dr, cdr))
        v = flow.volumes()
        vol_equal = bool(torch.equal(v[0].view(torch.int32), vols[2].view(torch.int32)) and
                         torch.equal(v[1].view(torch.int32), vols[3].view(torch.int32)))
        med = {k: float(np.median(x)) for k, x in t.items()}
        res["sizes"][f"{W}x{H}_d{D}"] = {
            "pairs": n,
            "composed_ms_per_pair": {"median": med["composed"], "min": min(t["composed"]), "max": max(t["composed"])},
            "batch_ms_per_pair": {"median": med["batch"], "min": min(t["batch"]), "max": max(t["batch"])},
            "speedup": med["composed"] / med["batch"],
            "maps_equal": equal, "last_pair_first_pass_volumes_equal": vol_equal,
            "samples": {k: [round(x, 4) for x in xs] for k, xs in t.items()}}
        print(name, json.dumps({k: v for k, v in res["sizes"][f"{W}x{H}_d{D}"].items() if k != "samples"}), flush=True)
        flow.close()
        for h in ca:
            L_.smt_crossarm_destroy(h)
        del vols, Lb, Rb, cdl, cdr, out
        torch.cuda.empty_cache()
        if not equal or not vol_equal:
            print("MISMATCH at", name, file=sys.stderr)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {"composed": v["composed_ms_per_pair"]["median"], "batch": v["batch_ms_per_pair"]["median"],
                          "speedup": round(v["speedup"], 3)} for k, v in res["sizes"].items()}))


if __name__ == "__main__":
    main()
