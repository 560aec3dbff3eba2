"""Cost of FillTheHole on a batch of LR-checked maps at 1920x1080, D=192, 8 pairs, two ways (run under a time limit,
e.g. `timeout -k 10 600 python tools/fill_time.py --out profiles/fill_batch_time.json`):

  composed   per pair: cls copied device to host, smt_lrcheck_lists on the host, smt_fill_the_hole (uploads the lists,
             allocates per call, synchronises; third list not requested, the cheapest form of the call)
  batch      smt_fill_the_hole_batch on the whole batch (one memset and eight launches, arena scratch, no sync)

  case a     the pipeline's LR-checked maps with their cls (Pipeline.run on synth pairs): no 65535 entries
  case b     the same maps with a seeded 2 % of the pixels set to 65535 after the LR check

Both paths must give equal bits before anything is timed.  Rounds interleave the two entries: two warm-up rounds, then
--rounds (>= 11) timed ones; host wall time ending in a stream synchronisation for both, event time for the batch entry.
--dry-run stops after argument parsing and input generation (no GPU needed).  Prints one JSON object; --out FILE also
writes it."""
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

H, W, D = 1080, 1920, 192


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def inputs(pairs, h, w, d):
    """synth pairs and, for case b, the seeded 2 % hole masks."""
    L, R, holes = [], [], []
    for b in range(pairs):
        l, r = synth.synth_pair(h, w, d, 3 + b)
        L.append(l)
        R.append(r)
        holes.append(np.random.default_rng(100 + b).random((h, w)) < 0.02)
    return np.stack(L), np.stack(R), np.stack(holes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--size", default="%dx%d" % (W, H), help="WxH")
    ap.add_argument("--disp", type=int, default=D)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds must be at least 11")
    w, h = (int(x) for x in a.size.split("x"))
    d, P = a.disp, a.pairs
    L, R, holes = inputs(P, h, w, d)
    if a.dry_run:
        print(json.dumps({"dry_run": True, "H": h, "W": w, "D": d, "pairs": P, "rounds": a.rounds,
                          "hole_pixels_case_b": [int(x.sum()) for x in holes]}))
        return

    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd._lib import lib, check
    dev = torch.device("cuda:0")
    pipe = smt.Pipeline(h, w, d, dev)
    dl, _, cls, _ = pipe.run(torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev))
    torch.cuda.synchronize()
    pipe.close()
    n = h * w
    occ, mis = np.empty((n, 2), np.int32), np.empty((n, 2), np.int32)
    st = torch.cuda.current_stream()

    def composed(maps):
        for b in range(P):
            ch = cls[b].cpu().numpy()
            no, nm = C.c_int(), C.c_int()
            check(lib().smt_lrcheck_lists(ch.ctypes.data_as(C.c_void_p), h, w, occ.ctypes.data_as(C.c_void_p), C.byref(no),
                                          mis.ctypes.data_as(C.c_void_p), C.byref(nm)), "smt_lrcheck_lists")
            check(lib().smt_fill_the_hole(C.c_void_p(maps[b].data_ptr()), h, w, d, occ.ctypes.data_as(C.c_void_p), no.value,
                                          mis.ctypes.data_as(C.c_void_p), nm.value, None, None,
                                          C.c_void_p(st.cuda_stream)), "smt_fill_the_hole")

    res = {"H": h, "W": w, "D": d, "pairs": P, "device": torch.cuda.get_device_name(0)}
    for name in ("a_lr_maps", "b_lr_maps_2pct_holes"):
        src = dl.clone()
        if name.startswith("b"):
            src[torch.from_numpy(holes).to(dev)] = 65535.0
        work = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        old_ms, new_ms, new_ev_ms = [], [], []
        status = None
        for r in range(a.rounds + 2):                                 # two warm-up rounds (arena, code objects)
            work.copy_(src)
            torch.cuda.synchronize()
            t = time.perf_counter()
            composed(work)
            torch.cuda.synchronize()
            t_old = (time.perf_counter() - t) * 1e3
            ref = work.clone()
            work.copy_(src)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record(st)
            status = smt.FillTheHoleBatch(work, cls, d)
            e1.record(st)
            torch.cuda.synchronize()
            t_new = (time.perf_counter() - t) * 1e3
            if not torch.equal(work.view(torch.int32), ref.view(torch.int32)):
                raise SystemExit(f"{name}: batch and composed results differ")
            if r >= 2:
                old_ms.append(t_old)
                new_ms.append(t_new)
                new_ev_ms.append(e0.elapsed_time(e1))
        s = status.cpu().numpy()
        if s[:, 3].any():
            raise SystemExit(f"{name}: flagged pairs {s[:, 3].tolist()}")
        o, m = stats(old_ms), stats(new_ms)
        res[name] = {"composed_wall_ms": o, "batch_wall_ms": m, "batch_event_ms": stats(new_ev_ms),
                     "batch_median_below_composed_median": bool(m["median"] < o["median"]),
                     "n_occ": s[:, 0].tolist(), "n_mis": s[:, 1].tolist(), "n_third": s[:, 2].tolist(),
                     "pixels_changed": int((src.view(torch.int32) != work.view(torch.int32)).sum())}
    out = json.dumps(res, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
