"""Region voting and outlier interpolation (include/smt_refine.h), timed on the pipeline's own
outputs for orc.synth_pair inputs: device events around every call, the entries alternating inside every round, 21 samples
per entry (7 rounds x 3), median [min, max].

    python tools/refine_time.py [--sizes teddy,kitti,hd] [--ab path/to/the/parent/commit's/libsmt_hip.so] [--no-host]
                                [--out profiles/refine_time.json]

Sizes (W x H, D), 8 pairs each: teddy 450x375 D=64, kitti 1242x375 D=256, hd 1920x1080 D=192.  The maps are dispL of
Pipeline.run after RemoveSpeckles, the arms those of every pair's left image, cls the LR check's.  Per size:
  vote_wave_first, vote_direct_first   one voting iteration (the first: every outlier is still there), each formulation
  vote_wave_5                          the five default iterations, wave form; per iteration = a fifth
  interpolate                          the interpolation on the voted maps
  refine                               smt_refine_batch, the default dispatch
  run_post, run_refined                the pipeline per call (divide by 8 for a pair)
and, at the first size, the host twin smt_refine_batch_host on one pair on one core, once.  The forms' maps are compared
bit for bit in the same run.

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
INT_MIN = -2 ** 31


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="teddy,kitti,hd")
    ap.add_argument("--ab", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_time.json"))
    a = ap.parse_args()
    names = a.sizes.split(",")
    if a.child:
        return child(names)
    res = {"tool": "tools/refine_time.py", "rounds": ROUNDS, "reps": REPS, "pairs": PAIRS, "cases": {}}
    if a.ab:
        res["existing_entries_this_against_parent"] = against_parent(os.path.abspath(a.ab), names)

    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import _lib
    res["device"] = torch.cuda.get_device_name(0)
    for name in names:
        H, W, D = SIZES[name]
        L8, R8 = pairs_of(name)
        pipe = smt.Pipeline(H, W, D)
        dl, dr, cls, counts = pipe.run(L8, R8)
        smt.RemoveSpecklesBatch(dl, 1, 30, INT_MIN)
        ca = smt.CrossArmAggregation().Initialize(H, W, 30, D)
        arms = [[], [], [], []]
        for b in range(PAIRS):
            ca.ComputeArmLengths(L8[b])
            for k, m in enumerate(ca.arm_maps()):
                arms[k].append(m.clone())
        ca.close()
        arms = [torch.stack(x) for x in arms]
        work = torch.empty_like(dl)
        voted = dl.clone()
        _, _, st0 = smt.RegionVote(voted, arms, D)
        one, five = smt.refine_params(irv_iters=1), smt.refine_params()
        outs = {}

        def fresh(src):
            return lambda: work.copy_(src)

        def vote(impl, p, key):
            def f():
                smt.refine_set_impl(impl)
                smt.RegionVote(work, arms, D, p)
                outs[key] = work.clone() if key not in outs else outs[key]
            return f

        entries = [("vote_wave_first", vote(_lib.REFINE_FORM_WAVE, one, "w1"), fresh(dl)),
                   ("vote_direct_first", vote(_lib.REFINE_FORM_DIRECT, one, "d1"), fresh(dl)),
                   ("vote_wave_5", vote(_lib.REFINE_FORM_WAVE, five, "w5"), fresh(dl)),
                   ("interpolate", lambda: smt.InterpolateOutliers(work, cls, L8, D), fresh(voted)),
                   ("refine", lambda: (smt.refine_set_impl(0), smt.Refine(work, arms, cls, L8, D)), fresh(dl)),
                   ("run_post", lambda: pipe.run_post(L8, R8), None),
                   ("run_refined", lambda: pipe.run_refined(L8, R8), None)]
        for _, fn, before in entries:
            for _ in range(2):
                if before:
                    before()
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _, _ in entries}
        for _ in range(ROUNDS):
            for k, fn, before in entries:
                for _ in range(REPS):
                    ms[k].append(timed(fn, before))
        smt.refine_set_impl(0)
        assert torch.equal(outs["w1"].view(torch.int32), outs["d1"].view(torch.int32)), name
        assert torch.equal(outs["w5"].view(torch.int32), voted.view(torch.int32)), name
        _, _, _, _, _, state, status = pipe.run_refined(L8, R8)
        case = {"H": H, "W": W, "D": D, "pairs": PAIRS, "status_of_the_voting_alone": st0.cpu().tolist(),
                "status_of_run_refined": status.cpu().tolist(), "ms": {k: stat(v) for k, v in ms.items()}}
        m = case["ms"]
        case["per_iteration_ms"] = {"wave_first": m["vote_wave_first"]["median"], "direct_first": m["vote_direct_first"]["median"],
                                    "wave_mean_of_5": m["vote_wave_5"]["median"] / 5}
        case["faster_form"] = "wave" if m["vote_wave_first"]["median"] <= m["vote_direct_first"]["median"] else "direct"
        case["per_pair_ms"] = {"run_post": m["run_post"]["median"] / PAIRS, "run_refined": m["run_refined"]["median"] / PAIRS,
                               "refinement": (m["run_refined"]["median"] - m["run_post"]["median"]) / PAIRS}
        if name == names[0] and not a.no_host:
            vp = lambda x: x.ctypes.data_as(C.c_void_p)
            hm = np.ascontiguousarray(dl[0].cpu().numpy())
            ha = [np.ascontiguousarray(x[0].cpu().numpy()) for x in arms]
            hc, hg = np.ascontiguousarray(cls[0].cpu().numpy()), np.ascontiguousarray(L8[0].cpu().numpy())
            z = C.c_size_t(0)
            t0 = time.perf_counter()
            rc = _lib.lib().smt_refine_batch_host(vp(hm), 1, z, *[vp(x) for x in ha], z, vp(hc), z, vp(hg), z, H, W, D, None, None, z, None)
            case["host_twin_one_pair_one_core_ms"] = (time.perf_counter() - t0) * 1e3
            work.copy_(dl)
            smt.Refine(work, arms, cls, L8, D)
            assert rc == 0 and np.array_equal(hm.view(np.uint32), work[0].cpu().numpy().view(np.uint32)), name
        pipe.close()
        res["cases"][name] = case
        print(name, {k: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"]) for k, v in m.items()}, case["per_pair_ms"],
              case.get("host_twin_one_pair_one_core_ms"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
