"""Disparity ranges above 256 on the window matchers and the CrossAggregator: time per call and per 64 hypotheses at
D = 256, 320 and 512, and the D <= 256 headline case of each family against the parent library, the two libraries
alternating on one box.  Device events around every call, medians over the reps of a round, interleaved rounds.

    python tools/wide_d_time.py [--rounds 3] [--reps 5] [--old-lib tools/_old_libsmt_hip.so] [--out profiles/wide_d_time.json]

Each round runs one worker process per library (SMT_HIP_LIB selects the library before it loads): new, old, new, old...
The wide cases only exist in the new library and run in the new library's workers."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE = [("sad5x5_960x540", "sad", dict(H=540, W=960, ws=1)), ("sad9x9_960x540", "sad", dict(H=540, W=960, ws=3)),
        ("ncc21x21_960x540", "ncc", dict(H=540, W=960, win=10)), ("asw35x35_960x540", "asw", dict(H=540, W=960, ws=16)),
        ("crossagg_720p_x4", "ca", dict(H=720, W=1280, iters=4))]
WIDE_D = (256, 320, 512)
HEADLINE = [("cfg1_sad5x5_450x375_d64", "sad", dict(H=375, W=450, ws=1, D=64)),
            ("ncc21x21_450x375_d200", "ncc", dict(H=375, W=450, win=10, D=200)),
            ("cfg4_asw35x35_960x540_d128", "asw", dict(H=540, W=960, ws=16, D=128)),
            ("crossagg_720p_d128_x4", "ca", dict(H=720, W=1280, iters=4, D=128))]


def worker(which, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import synth
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pairs = {}

    def pair(H, W):
        if (H, W) not in pairs:
            pairs[(H, W)] = synth.synth_pair(H, W, 64, 4)
        return pairs[(H, W)]

    def make(fam, p, D):
        L, R = pair(p["H"], p["W"])
        if fam == "sad":
            w = p["ws"] + 1
            Lp, Rp = T(np.pad(L, w, mode="edge")), T(np.pad(R, w, mode="edge"))
            return lambda: smt.GetPointDepthLeft(Lp, Rp, D, p["ws"])
        if fam == "ncc":
            Lt, Rt = T(L), T(R)
            return lambda: smt.NCC_algorithem(Lt, Rt, p["win"], D)
        if fam == "asw":
            w = p["ws"] + 1
            Lp, Rp = T(np.pad(L, w, mode="edge")), T(np.pad(R, w, mode="edge"))
            sp, cm = smt.asw_masks(p["ws"], 50.0, 30.0, dev)
            return lambda: smt.AdaptiveSupportWeight(Lp, Rp, p["ws"], D, sp, cm, 40, smt.VIEW_LEFT)
        bgr = T(np.stack([L, L // 2 + 7, 255 - L], axis=2).astype(np.uint8))
        cost = torch.rand((p["H"], p["W"], D), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        agg = smt.CrossAggregator()
        assert agg.Initialize(p["W"], p["H"], 0, D, dev)
        agg.SetData(bgr, bgr, cost)
        agg.SetParams(34, 17, 20, 6)
        return lambda: agg.Aggregate(p["iters"])

    def time(fn):
        fn(); fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    out = {}
    for name, fam, p in HEADLINE:
        out[name] = time(make(fam, p, p["D"]))
    if which == "new":
        for name, fam, p in WIDE:
            for D in WIDE_D:
                out[f"{name}_d{D}"] = time(make(fam, p, D))
    print("__RESULT__" + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-lib", default=os.path.join(ROOT, "tools", "_old_libsmt_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_d_time.json"))
    ap.add_argument("--worker", choices=["new", "old"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps)
    rounds = {"new": [], "old": []}
    for r in range(a.rounds):
        for which in ("new", "old"):
            env = dict(os.environ)
            env.pop("SMT_HIP_LIB", None)
            if which == "old":
                env["SMT_HIP_LIB"] = a.old_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", which, "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"worker {which} round {r} exited with {p.returncode}")
            res = json.loads(p.stdout.split("__RESULT__")[-1])
            rounds[which].append(res)
            print(which, r, json.dumps(res), flush=True)
    import numpy as np
    med = lambda which, k: float(np.median([x[k] for x in rounds[which]]))
    spread = lambda which, k: (max(x[k] for x in rounds[which]) - min(x[k] for x in rounds[which])) / med(which, k)
    head = {}
    for name, _, _ in HEADLINE:
        n, o = med("new", name), med("old", name)
        head[name] = {"new_ms": n, "old_ms": o, "new_over_old": n / o, "spread_new": spread("new", name),
                      "spread_old": spread("old", name)}
    wide = {}
    for name, _, _ in WIDE:
        per = {D: med("new", f"{name}_d{D}") for D in WIDE_D}
        wide[name] = {"ms": {str(D): per[D] for D in WIDE_D},
                      "ms_per_64": {str(D): per[D] / (D / 64) for D in WIDE_D},
                      "d512_per_64_over_d256_per_64": (per[512] / 8) / (per[256] / 4),
                      "spread": {str(D): spread("new", f"{name}_d{D}") for D in WIDE_D}}
    import torch
    doc = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None, "rounds": a.rounds,
           "reps": a.reps, "headline_parent_vs_new": head, "wide": wide, "raw": rounds}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({"headline_parent_vs_new": head, "wide": {k: (v["ms"], v["d512_per_64_over_d256_per_64"]) for k, v in wide.items()}}, indent=1))


if __name__ == "__main__":
    main()
