"""The per-hypothesis-arm CBLSM flow two ways, interleaved in one process: the composed single calls (two crossarm
handles, smt_cblsm_ad, four smt_cblsm_choose_arm_length, smt_cblsm_cost_aggregation_v4 with its WTA; six caller-held
[H][W][D] volumes) against smt_cblsm_flow_run_batch_v4 (arms derived in the kernel, rectangle sums from the summed-area
table; two volumes).  Device events around every batch call, ms per pair; median [min-max] over the rounds; the maps
and the last pair's volume of the two forms are compared in the same run.

    python tools/cblsm_v4_time.py [--sizes small,kitti] [--rounds 5] [--reps 3] [--out profiles/cblsm_v4_time.json]

Sizes: 450x375 D=60 (CBLSM.cpp:28-32's class, 32 pairs), 1242x375 D=128 (8 pairs)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"small": (375, 450, 60, 32), "kitti": (375, 1242, 128, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,kitti")
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
        cp = CrossArmParams()
        L_.smt_crossarm_cblsm_params(C.byref(cp))
        ca = [C.c_void_p(), C.c_void_p()]
        maps = []
        for h in ca:
            check(L_.smt_crossarm_create_on(0, H, W, D, C.byref(cp), C.byref(h)), "smt_crossarm_create_on")
            check(L_.smt_crossarm_set_stream(h, st), "smt_crossarm_set_stream")
            m = [C.c_void_p() for _ in range(4)]
            check(L_.smt_crossarm_arm_maps(h, *[C.byref(x) for x in m]), "smt_crossarm_arm_maps")
            maps.append(m)
        (LL, LR, LU, LD), (RL, RR, RU, RD) = maps
        ad, out = (torch.empty((H, W, D), dtype=torch.float32, device=dev) for _ in range(2))
        av = [torch.empty((H, W, D), dtype=torch.int32, device=dev) for _ in range(4)]
        ub = torch.zeros(1, dtype=torch.int32, device=dev)
        cdl = torch.empty((n, H, W), dtype=torch.float32, device=dev)

        def composed():
            for b in range(n):
                check(L_.smt_crossarm_arms(ca[0], P(Lb[b]), 1), "arms L")                                      # :64-67
                check(L_.smt_crossarm_arms(ca[1], P(Rb[b]), 1), "arms R")                                      # :101-104
                check(L_.smt_cblsm_choose_arm_length(0, LL, None, RL, RR, H, W, D, P(av[0]), st), "choose L")  # :108
                check(L_.smt_cblsm_choose_arm_length(1, LR, None, RL, RR, H, W, D, P(av[1]), st), "choose R")  # :109
                check(L_.smt_cblsm_choose_arm_length(2, LU, RU, RL, RR, H, W, D, P(av[2]), st), "choose Up")   # :110
                check(L_.smt_cblsm_choose_arm_length(3, LD, RD, RL, RR, H, W, D, P(av[3]), st), "choose Down")  # :111
                check(L_.smt_cblsm_ad(P(Lb[b]), P(Rb[b]), H, W, D, smt.VIEW_LEFT, P(ad), st), "ad")            # :133
                check(L_.smt_cblsm_cost_aggregation_v4(P(ad), P(av[0]), P(av[1]), P(av[2]), P(av[3]), H, W, D, P(out),
                                                       P(cdl[b]), P(ub), st), "v4")                           # V4, :152

        flow = smt.CBLSMFlow(H, W, D, dev)
        got = {}

        def fused():
            got["map"] = flow.run_v4(Lb, Rb)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / n

        composed(); fused(); torch.cuda.synchronize()                     # warm-up: code objects, first touches
        t = {"composed": [], "fused": []}
        for _ in range(a.rounds):
            for k, fn in (("composed", composed), ("fused", fused)):
                for _ in range(a.reps):
                    t[k].append(timed(fn))
        flow.status()
        for h in ca:
            check(L_.smt_crossarm_status(h), "smt_crossarm_status")
        equal = bool(torch.equal(got["map"], cdl)) and int(ub.item()) == 0
        fv = flow.volumes()[0]
        nan_f, nan_c = torch.isnan(fv), torch.isnan(out)
        vol_equal = bool(torch.equal(nan_f, nan_c) and
                         torch.equal(fv[~nan_f].view(torch.int32), out[~nan_c].view(torch.int32)))
        med = {k: float(np.median(x)) for k, x in t.items()}
        key = f"{W}x{H}_d{D}"
        res["sizes"][key] = {
            "pairs": n,
            "composed_ms_per_pair": {"median": med["composed"], "min": min(t["composed"]), "max": max(t["composed"])},
            "fused_ms_per_pair": {"median": med["fused"], "min": min(t["fused"]), "max": max(t["fused"])},
            "speedup": med["composed"] / med["fused"],
            "nan_fraction_of_last_volume": float(nan_f.float().mean()),
            "maps_equal": equal, "last_pair_volumes_equal": vol_equal,
            "samples": {k: [round(x, 4) for x in xs] for k, xs in t.items()}}
        print(name, json.dumps({k: v for k, v in res["sizes"][key].items() if k != "samples"}), flush=True)
        flow.close()
        for h in ca:
            L_.smt_crossarm_destroy(h)
        del ad, out, av, Lb, Rb, cdl, got
        torch.cuda.empty_cache()
        if not equal or not vol_equal:
            print("MISMATCH at", name, file=sys.stderr)
            sys.exit(1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: {"composed": v["composed_ms_per_pair"]["median"], "fused": v["fused_ms_per_pair"]["median"],
                          "speedup": round(v["speedup"], 3)} for k, v in res["sizes"].items()}))


if __name__ == "__main__":
    main()
