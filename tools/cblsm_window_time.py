"""CBLSM's window cost volumes (smt_cblsm_window_cost_batch) timed on the device, everything interleaved in one process:
per size and view the tap loop (impl 1), the box kernel with plain and with non-temporal stores (impl 2), and a
store-only fill of the same volume (torch's fill kernel on the same tensor: the ceiling of a kernel that writes
4 bytes per hypothesis and reads almost nothing).  Device events around every call; median [min-max] of --samples
interleaved samples; the two formulations are compared bit for bit in the same run.  Then the flow: run_window against
run per pair on 8 pairs.

    python tools/cblsm_window_time.py [--sizes cblsm,kitti,hd5,hd11] [--samples 21] [--flow cblsm,hd] [--out profiles/cblsm_window_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (H, W, D, winSize)
SIZES = {"cblsm": (375, 450, 60, 1), "kitti": (375, 1242, 128, 1), "hd5": (1080, 1920, 192, 1), "hd11": (1080, 1920, 192, 4)}
FLOWS = {"cblsm": (375, 450, 60, 1), "hd": (1080, 1920, 192, 1)}


def stats(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "samples": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="cblsm,kitti,hd5,hd11")
    ap.add_argument("--flow", default="cblsm,hd")
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--flow-samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"note": "ms per call, device events; median [min, max] of interleaved samples in one process",
           "device": torch.cuda.get_device_name(0), "volumes": {}, "flow": {}}
    for name in [s for s in a.sizes.split(",") if s]:
        H, W, D, ws = SIZES[name]
        w = ws + 1
        L, R = synth.synth_pair(H, W, D, 50)
        Lp = smt.copyMakeBorder_replicate(torch.from_numpy(L).to(dev), w)
        Rp = smt.copyMakeBorder_replicate(torch.from_numpy(R).to(dev), w)
        vol = torch.empty((H, W, D), dtype=torch.float32, device=dev)
        ref = torch.empty_like(vol)
        for view, f in (("left", smt.ComputeDispLeft), ("right", smt.ComputeDispRight)):
            def run(impl, store):
                smt.cblsm_window_set_impl(impl); smt.cblsm_window_set_store(store)
                f(Lp, Rp, ws, D, out=vol)

            forms = {"tap": lambda: run(1, 0), "box_plain": lambda: run(2, 1), "box_nt": lambda: run(2, 2),
                     "store_only": lambda: vol.fill_(1.0)}
            run(1, 0); ref.copy_(vol)
            equal = True
            for k in ("box_plain", "box_nt"):
                vol.fill_(float("nan")); forms[k]()
                equal = equal and bool(torch.equal(vol.view(torch.int32), ref.view(torch.int32)))
            torch.cuda.synchronize()
            t = {k: [] for k in forms}
            for _ in range(a.samples):
                for k, fn in forms.items():
                    t[k].append(timed(fn))
            smt.cblsm_window_set_impl(0); smt.cblsm_window_set_store(0)
            row = {k: stats(x) for k, x in t.items()}
            best = min(row["box_plain"]["median"], row["box_nt"]["median"])
            row.update(bits_equal=equal, bytes=int(vol.numel() * 4), box_over_tap=best / row["tap"]["median"],
                       frac_of_store_ceiling=row["store_only"]["median"] / best)
            res["volumes"][f"{W}x{H}_d{D}_side{2 * w + 1}_{view}"] = row
            print(name, view, json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
            if not equal:
                print("MISMATCH at", name, view, file=sys.stderr)
                sys.exit(1)
        del vol, ref
        torch.cuda.empty_cache()
    for name in [s for s in a.flow.split(",") if s]:
        H, W, D, ws = FLOWS[name]
        n = 8
        imgs = [synth.synth_pair(H, W, D, 60 + b) for b in range(n)]
        Lb = torch.from_numpy(np.stack([x[0] for x in imgs])).to(dev)
        Rb = torch.from_numpy(np.stack([x[1] for x in imgs])).to(dev)
        flow = smt.CBLSMFlow(H, W, D, dev)
        forms = {"run": lambda: flow.run(Lb, Rb), "run_window": lambda: flow.run_window(Lb, Rb, ws)}
        for fn in forms.values():
            fn()
        flow.status()
        t = {k: [] for k in forms}
        for _ in range(a.flow_samples):
            for k, fn in forms.items():
                t[k].append(timed(fn) / n)
        flow.status()
        flow.close()
        row = {k + "_ms_per_pair": stats(x) for k, x in t.items()}
        row["pairs"] = n
        res["flow"][f"{W}x{H}_d{D}_side{2 * ws + 3}"] = row
        print("flow", name, json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        del Lb, Rb
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
