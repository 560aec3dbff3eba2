"""Cost of main.cpp:93-94 (RemoveSpeckles, MedianFilter) on the device, in two parts (run each under its own time
limit, e.g. `timeout -k 10 300 python tools/post_time.py --part speckle`):

  --part speckle   smt_remove_speckles (one map, synchronising, allocates per call) against smt_remove_speckles_batch
                   (asynchronous, arena scratch) on the config-3 pair's LR-checked map and on a 1080p serpentine map
                   (one one-pixel-wide region through every tile); host wall time per call, both ending in a stream
                   synchronisation, plus event time of the batch entry alone.  Rounds interleave the two entries.
  --part pipeline  ms per pair of smt_pipeline_run_batch against smt_pipeline_run_batch_post at 1920x1080 D=192,
                   8 pairs per call, on one handle, rounds interleaved.

Prints one JSON object; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stereo_match_traditional_amd as smt  # noqa: E402
from stereo_match_traditional_amd import synth  # noqa: E402

DEV = torch.device("cuda:0")
INT_MIN = -(2 ** 31)
H, W, D = 1080, 1920, 192


def serpentine():
    a = np.full((H, W), 50.0, np.float32)
    a[0::2] = 1.0
    for r in range(1, H, 2):
        a[r, W - 1 if (r // 2) % 2 == 0 else 0] = 1.0
    return a


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def part_speckle(rounds):
    L, R = synth.synth_pair(H, W, D, 3)
    pipe = smt.Pipeline(H, W, D, DEV)
    lr = pipe.run(torch.from_numpy(L[None]).to(DEV), torch.from_numpy(R[None]).to(DEV))[0][0].clone()
    pipe.close()
    torch.cuda.synchronize()
    out = {}
    for name, src in (("config3_lr_map", lr), ("serpentine", torch.from_numpy(serpentine()).to(DEV))):
        old_ms, new_ms, new_ev_ms = [], [], []
        work = torch.empty_like(src)
        st = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(rounds + 2):                                   # two warm-up rounds (arena, code objects)
            work.copy_(src)
            torch.cuda.synchronize()
            t = time.perf_counter()
            smt.RemoveSpeckles(work, W, H, 1, 30, INT_MIN)
            torch.cuda.synchronize()
            t_old = (time.perf_counter() - t) * 1e3
            ref = work.clone()
            work.copy_(src)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record(st)
            smt.RemoveSpecklesBatch(work[None], 1, 30, INT_MIN)
            e1.record(st)
            torch.cuda.synchronize()
            t_new = (time.perf_counter() - t) * 1e3
            if not torch.equal(work.view(torch.int32), ref.view(torch.int32)):
                raise SystemExit(f"{name}: batch and single-map results differ")
            if r >= 2:
                old_ms.append(t_old)
                new_ms.append(t_new)
                new_ev_ms.append(e0.elapsed_time(e1))
        changed = int((src.view(torch.int32) != work.view(torch.int32)).sum())
        out[name] = {"smt_remove_speckles_wall_ms": stats(old_ms), "smt_remove_speckles_batch_wall_ms": stats(new_ms),
                     "smt_remove_speckles_batch_event_ms": stats(new_ev_ms), "pixels_changed": changed}
    return out


def part_pipeline(rounds, pairs):
    L, R = [], []
    for b in range(pairs):
        l, r = synth.synth_pair(H, W, D, 3 + b)
        L.append(l)
        R.append(r)
    Lb, Rb = torch.from_numpy(np.stack(L)).to(DEV), torch.from_numpy(np.stack(R)).to(DEV)
    pipe = smt.Pipeline(H, W, D, DEV)
    plain, post = [], []
    for r in range(rounds + 1):                                       # round 0: warm-up (tail scratch, code objects)
        for which in (0, 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if which == 0:
                pipe.run(Lb, Rb)
            else:
                pipe.run_post(Lb, Rb)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) * 1e3 / pairs
            if r >= 1:
                (plain if which == 0 else post).append(ms)
    pipe.status()
    pipe.close()
    a, b = stats(plain), stats(post)
    return {"pairs_per_call": pairs, "run_batch_ms_per_pair": a, "run_batch_post_ms_per_pair": b,
            "post_over_plain_median_pct": 100.0 * (b["median"] / a["median"] - 1.0),
            "schedule": os.environ.get("SMT_PIPE_SCHEDULE", "default")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["speckle", "pipeline"], required=True)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"part": a.part, "H": H, "W": W, "D": D, "device": torch.cuda.get_device_name(0)}
    res.update(part_speckle(a.rounds) if a.part == "speckle" else part_pipeline(a.rounds, a.pairs))
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
