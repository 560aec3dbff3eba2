"""Host-fed AD-Census at config 5 (256 KITTI pairs, 375 x 1242, D = 256) against the device-resident batch.

Cases, alternated round by round in one process after a warm-up round:
  a  smt_adcensus_compute_batch, float32 inputs already on the device (the reference rate)
  b  ADCensusHostBatch, gray uint8 in, uint8 maps out, pinned
  c  gray in, float32 maps out, pinned
  d  BGR in, uint8 maps out, pinned
  e  b with pageable tensors
  link  pinned H2D of b's input bytes and D2H of b's output bytes on their own (torch copies): the link in this run
and a sweep of `chunk` for b.  Per case: ms/pair (host clock around the synchronising call, median over rounds),
Mdisp/s (H*W*D per pair and view), H2D / D2H GB/s and wall_ms - compute_ms (exposed copy time) from the run's device
events, and the pair rate as a fraction of a's.

    python tools/hostfeed_time.py [--rounds 5] [--out profiles/hostfeed_cfg5.json] [--only b]
"""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_match_traditional_amd as smt  # noqa: E402
from stereo_match_traditional_amd import synth  # noqa: E402

H, W, D, P = 375, 1242, 256, 256
DEV = torch.device("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", default="2,4,8,16,32")
    ap.add_argument("--chunk", type=int, default=None, help="chunk of cases b-e (default: the class default)")
    ap.add_argument("--only", default=None, help="run only this host case once (profiling)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, 1000 + b) for b in range(P)])
    Lg, Rg = np.stack(Ls), np.stack(Rs)
    pin = lambda x: torch.from_numpy(x).pin_memory()
    gray = (pin(Lg), pin(Rg))
    bgr = (pin(np.repeat(Lg[..., None], 3, axis=3)), pin(np.repeat(Rg[..., None], 3, axis=3)))   # gray of it = Lg
    pageable = (torch.from_numpy(Lg.copy()), torch.from_numpy(Rg.copy()))
    kw = {} if a.chunk is None else {"chunk": a.chunk}

    def host_case(inputs, out_dtype, channels, pinned_out=True, **k):
        hb = smt.ADCensusHostBatch(H, W, D, 10.0, 30.0, channels=channels, out_dtype=out_dtype, **{**kw, **k})
        shp = (P, H, W)
        outs = (torch.empty(shp, dtype=out_dtype, pin_memory=pinned_out), torch.empty(shp, dtype=out_dtype, pin_memory=pinned_out))

        def run():
            t0 = time.perf_counter()
            hb.run(*inputs, *outs)
            return (time.perf_counter() - t0) * 1e3, hb.stats()
        return run, hb, outs

    cases = {
        "b_gray_u8_pinned": host_case(gray, torch.uint8, 1),
        "c_gray_f32_pinned": host_case(gray, torch.float32, 1),
        "d_bgr_u8_pinned": host_case(bgr, torch.uint8, 3),
        "e_gray_u8_pageable": host_case(pageable, torch.uint8, 1, pinned_out=False),
    }
    if a.only:
        run, hb, _ = cases[a.only]
        run()
        ms, st = run()
        print(json.dumps({"case": a.only, "ms": ms, "stats": st}))
        return

    # a: device-resident batch
    Lf = torch.from_numpy(Lg.astype(np.float32)).to(DEV)
    Rf = torch.from_numpy(Rg.astype(np.float32)).to(DEV)
    dl = torch.empty((P, H, W), device=DEV)
    dr = torch.empty((P, H, W), device=DEV)
    adc = smt.AD_Census().Initialize(Lf[0], Rf[0], D, H, W, 10.0, 30.0)

    def device_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        adc.ComputeBatch(Lf, Rf, dl, dr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, None

    # link ceiling: the same byte counts as b, pinned, one direction at a time
    h2d_src = torch.from_numpy(np.concatenate([Lg, Rg])).pin_memory()
    h2d_dst = torch.empty(h2d_src.shape, dtype=torch.uint8, device=DEV)
    d2h_dst = torch.empty(h2d_src.shape, dtype=torch.uint8, pin_memory=True)

    def link_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h2d_dst.copy_(h2d_src, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d2h_dst.copy_(h2d_dst, non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    sweep = {f"b_chunk{c}": host_case(gray, torch.uint8, 1, chunk=int(c)) for c in a.chunks.split(",")}
    order = [("a_device", device_run)] + [(k, v[0]) for k, v in cases.items()] + [(k, v[0]) for k, v in sweep.items()]
    res = {k: [] for k, _ in order}
    link = []
    for r in range(a.rounds + 1):
        for k, f in order:
            out = f()
            if r:
                res[k].append(out)
        out = link_run()
        if r:
            link.append(out)
    a_ms = statistics.median(ms for ms, _ in res["a_device"]) / P
    in_bytes, out_bytes = h2d_src.numel(), d2h_dst.numel()
    report = {"config": {"H": H, "W": W, "D": D, "pairs": P, "rounds": a.rounds,
                         "default_chunk": inspect.signature(smt.ADCensusHostBatch).parameters["chunk"].default if a.chunk is None else a.chunk,
                         "device": torch.cuda.get_device_name(0)},
              "link_pinned": {"h2d_bytes": in_bytes, "d2h_bytes": out_bytes,
                              "h2d_GBps": in_bytes / statistics.median(t for t, _ in link) / 1e6,
                              "d2h_GBps": out_bytes / statistics.median(t for _, t in link) / 1e6},
              "cases": {}}
    for k, runs in res.items():
        ms = statistics.median(m for m, _ in runs)
        rec = {"ms_per_pair": ms / P, "ms_per_pair_all_rounds": [m / P for m, _ in runs],
               "Mdisp_per_s": 2 * H * W * D * P / ms / 1e3, "rate_vs_a": a_ms / (ms / P)}
        st = [s for _, s in runs if s]
        if st:
            med = lambda f: statistics.median(f(s) for s in st)
            rec.update({"h2d_GBps": med(lambda s: s["h2d_bytes"] / s["h2d_ms"] / 1e6),
                        "d2h_GBps": med(lambda s: s["d2h_bytes"] / s["d2h_ms"] / 1e6),
                        "wall_ms": med(lambda s: s["wall_ms"]), "compute_ms": med(lambda s: s["compute_ms"]),
                        "h2d_ms": med(lambda s: s["h2d_ms"]), "d2h_ms": med(lambda s: s["d2h_ms"]),
                        "exposed_copy_ms": med(lambda s: s["wall_ms"] - s["compute_ms"]),
                        "h2d_bytes": st[-1]["h2d_bytes"], "d2h_bytes": st[-1]["d2h_bytes"], "chunks": st[-1]["chunks"],
                        "pinned_in": st[-1]["pinned_in"], "pinned_out": st[-1]["pinned_out"]})
        report["cases"][k] = rec
    txt = json.dumps(report, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")
    for _, hb, _ in list(cases.values()) + list(sweep.values()):
        hb.close()
    adc.close()


if __name__ == "__main__":
    main()
