"""Sad.h's FillHolesInDispMap (include/smt_fill_holes.h), timed on the pipeline's own LR-checked
maps for orc.synth_pair inputs: device events around every call, the entries alternating inside every round, 21 samples
per entry (7 rounds x 3), median [min, max].

    python tools/fill_holes_time.py [--sizes teddy,kitti,hd] [--ab path/to/the/parent/commit's/libsmt_hip.so] [--no-host]
                                    [--out profiles/fill_holes_time.json]

Sizes (W x H, D), 8 pairs each: teddy 450x375 D=64, kitti 1242x375 D=256, hd 1920x1080 D=192.  The maps are dispL of
Pipeline.run (after the LR check: +inf holes), cls the LR check's.  Per size:
  fill_holes                  smt_fill_holes_batch on the 8 maps (one workgroup per map), and on 1 map
  refine                      smt_refine_batch on the same maps (the library's own rule, for scale)
  run_post, run_refined, run_filled   the pipeline per call (divide by 8 for a pair)
and, at every size, the host twin smt_fill_holes_batch_host on one pair on one core (5 samples), with the device's map
and status of that pair compared bit for bit with the host twin's in the same run.  A line is printed after every round,
so a long size is seen to move.

--ab: run_batch_post and run_batch of this build and of the library named (the parent commit's) in alternating child
processes, this build first in half of the rounds, 6 rounds of 4 samples (24 per library and entry); `inside` says whether
this build's median lies inside the parent's own min-max spread."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"teddy": (375, 450, 64), "kitti": (375, 1242, 256), "hd": (1080, 1920, 192)}
PAIRS = 8
ROUNDS, REPS = 7, 3
AB_ROUNDS, AB_REPS = 6, 4


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs), "samples": [round(x, 4) for x in xs]}


def timed(fn, before=None):
    import torch
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def pairs_of(name):
    import numpy as np
    import torch
    from oracle import oracle as orc
    H, W, D = SIZES[name]
    prs = [orc.synth_pair(H, W, D, 3 + k) for k in range(PAIRS)]
    dev = torch.device("cuda:0")
    return (torch.from_numpy(np.stack([p[0] for p in prs])).to(dev), torch.from_numpy(np.stack([p[1] for p in prs])).to(dev))


def child(names):
    """the two existing pipeline entries of whatever library SMT_HIP_LIB names -> one JSON line"""
    import torch
    import stereo_match_traditional_amd as smt
    out = {}
    for name in names:
        H, W, D = SIZES[name]
        L8, R8 = pairs_of(name)
        pipe = smt.Pipeline(H, W, D)
        entries = {"run_batch_post": lambda: pipe.run_post(L8, R8), "run_batch": lambda: pipe.run(L8, R8)}
        for fn in entries.values():
            fn(); fn()
        torch.cuda.synchronize()
        out[name] = {k: [timed(fn) for _ in range(AB_REPS)] for k, fn in entries.items()}
        pipe.close()
    print("AB " + json.dumps(out), flush=True)


def against_parent(parent_lib, names):
    def run(lib):
        env = dict(os.environ)
        env.pop("SMT_HIP_LIB", None)
        if lib:
            env["SMT_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", ",".join(names)], capture_output=True, text=True,
                           env=env, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("child failed:\n" + r.stdout + r.stderr)
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:])
    pooled = {"this": {}, "parent": {}}
    for rnd in range(AB_ROUNDS):
        order = ("this", "parent") if rnd % 2 == 0 else ("parent", "this")
        for who in order:
            got = run(parent_lib if who == "parent" else None)
            for name, ent in got.items():
                for k, v in ent.items():
                    pooled[who].setdefault(name, {}).setdefault(k, []).extend(v)
    res = {"protocol": f"{AB_ROUNDS} rounds of alternating child processes, {AB_REPS} samples per entry and process, ms per call of {PAIRS} pairs"}
    for name in names:
        res[name] = {}
        for k in pooled["this"][name]:
            t, p = stat(pooled["this"][name][k]), stat(pooled["parent"][name][k])
            res[name][k] = {"this": t, "parent": p, "inside": p["min"] <= t["median"] <= p["max"]}
            print("ab", name, k, "this %.3f [%.3f-%.3f]" % (t["median"], t["min"], t["max"]),
                  "parent %.3f [%.3f-%.3f]" % (p["median"], p["min"], p["max"]), "inside" if res[name][k]["inside"] else "OUTSIDE", flush=True)
    return res


def measure(name, host):
    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import _lib
    H, W, D = SIZES[name]
    L8, R8 = pairs_of(name)
    pipe = smt.Pipeline(H, W, D)
    dl, _, cls, _ = pipe.run(L8, R8)
    ca = smt.CrossArmAggregation().Initialize(H, W, 30, D)
    arms = []
    for b in range(PAIRS):
        ca.ComputeArmLengths(L8[b])
        arms.append([a.clone() for a in ca.arm_maps()])
    ca.close()
    arms = [torch.stack([arms[b][k] for b in range(PAIRS)]) for k in range(4)]
    work = dl.clone()
    status = smt.FillHolesInDispMap(work, cls)
    torch.cuda.synchronize()
    res = {"H": H, "W": W, "D": D, "pairs": PAIRS, "steps_per_pass": 2 * (H - 1) + W, "status": status.cpu().tolist(),
           "holes_left": [int(torch.isinf(work[b]).sum()) for b in range(PAIRS)]}
    print(name, "status", res["status"][0], "holes left", res["holes_left"][0], flush=True)
    if host:
        m = np.ascontiguousarray(dl[0].cpu().numpy())
        c = np.ascontiguousarray(cls[0].cpu().numpy())
        st = np.zeros(4, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        src = m.copy()
        host_ms = []
        for _ in range(5):
            m[...] = src
            t0 = time.perf_counter()
            rc = _lib.lib().smt_fill_holes_batch_host(vp(m), vp(c), 1, C.c_size_t(0), C.c_size_t(0), H, W, C.c_float(float("inf")), vp(st))
            host_ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        res["host_twin_one_pair_one_core"] = stat(host_ms)
        res["host_twin_one_pair_one_core_ms"] = res["host_twin_one_pair_one_core"]["median"]
        res["device_equals_host_twin"] = bool(np.array_equal(m.view(np.uint32), work[0].cpu().numpy().view(np.uint32))
                                              and st.tolist() == res["status"][0])
        print(name, "host twin %.1f ms, device equals it: %s" % (res["host_twin_one_pair_one_core_ms"], res["device_equals_host_twin"]), flush=True)
    reset = lambda: work.copy_(dl)
    one = work[:1]
    entries = {
        "fill_holes": (lambda: smt.FillHolesInDispMap(work, cls), reset),
        "fill_holes_one_map": (lambda: smt.FillHolesInDispMap(one, cls[:1]), reset),
        "refine": (lambda: smt.Refine(work, arms, cls, L8, D), reset),
        "run_post": (lambda: pipe.run_post(L8, R8), None),
        "run_refined": (lambda: pipe.run_refined(L8, R8), None),
        "run_filled": (lambda: pipe.run_filled(L8, R8), None),
    }
    for fn, before in entries.values():
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in entries}
    for rnd in range(ROUNDS):
        for k, (fn, before) in entries.items():
            for _ in range(REPS):
                samples[k].append(timed(fn, before))
        print(name, "round", rnd + 1, "of", ROUNDS, flush=True)
    pipe.close()
    res["ms"] = {k: stat(v) for k, v in samples.items()}
    med = {k: v["median"] for k, v in res["ms"].items()}
    res["per_pair_ms"] = {"fill_holes_in_a_call_of_8": med["fill_holes"] / PAIRS, "fill_holes_alone": med["fill_holes_one_map"],
                          "refine": med["refine"] / PAIRS, "run_post": med["run_post"] / PAIRS,
                          "run_refined": med["run_refined"] / PAIRS, "run_filled": med["run_filled"] / PAIRS}
    res["us_per_step"] = med["fill_holes_one_map"] * 1e3 / (3 * res["steps_per_pass"])
    for k, v in res["ms"].items():
        print(name, k, "%.3f [%.3f-%.3f] ms" % (v["median"], v["min"], v["max"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="teddy,kitti,hd")
    ap.add_argument("--ab", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_holes_time.json"))
    a = ap.parse_args()
    names = [n for n in a.sizes.split(",") if n]
    if a.child:
        return child(names)
    import torch
    out = {"tool": "tools/fill_holes_time.py", "rounds": ROUNDS, "reps": REPS, "pairs": PAIRS, "cases": {}}
    for k, name in enumerate(names):
        out["cases"][name] = measure(name, host=not a.no_host)
    if a.ab:
        out["existing_entries_this_against_parent"] = against_parent(os.path.abspath(a.ab), names)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
