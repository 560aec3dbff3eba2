"""The bilateral image filter (include/smt_bilateral.h), timed: the staged form against the direct
form, device events around every call, the two forms alternating inside every round, 21 samples per form (7 rounds x 3),
median [min, max]; and the host twin on the CPU at the first size, once, as the reference-shaped baseline.

    python tools/bilateral_time.py [--sizes teddy25,teddy23,hd23,hd23gray] [--valu-rate path/to/valu_rate] [--no-host]
                                   [--out profiles/bilateral_time.json]

Sizes (W x H x channels, window, sigma space / colour): teddy25 450x375x3 25x25 50/25 (TeddyBilateral.cpp:39-46);
teddy23 450x375x3 23x23 10/30; hd23 1920x1080x3 23x23 10/30; hd23gray 1920x1080x1 23x23 10/30.

Beside the samples, per case: the float64 operation count -- per sample and tap two in pass 1 (the weight's product, the
sum) and four in pass 2 (the weight's product, its scaling by 1 / S, the product with the sample, the sum) plus one
integer-to-float64 conversion -- and the rate it implies.  --valu-rate names a build of tools/valu_rate.hip; it is run
once, in a process of its own, and the issue costs it prints for v_mul_f64, v_add_f64 and v_cvt_f64_u32 (ns per wave
instruction per SIMD at the best occupancy it measures) give the time those seven instructions alone would take on the
1 024 SIMDs: the floor the staged form is held against.  The staged form is also timed on a flat image and on uniform
noise of the same size (7 samples each): the two ends of the colour gather's bank behaviour."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"teddy25": (375, 450, 3, (25, 25), 50, 25), "teddy23": (375, 450, 3, (23, 23), 10, 30),
         "hd23": (1080, 1920, 3, (23, 23), 10, 30), "hd23gray": (1080, 1920, 1, (23, 23), 10, 30)}
ROUNDS, REPS = 7, 3
SIMDS = 1024


def stat(xs):
    import numpy as np
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs), "samples": [round(x, 4) for x in xs]}


def image(H, W, ch, seed):
    """a synthetic scene with edges, texture and noise: the colour table is read near 0 mostly, as on a photograph"""
    import numpy as np
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([128 + 60 * np.sin(x / (23.0 + 5 * k)) * np.cos(y / (31.0 - 4 * k)) + 50 * (((x // 60) + (y // 45) + k) & 1) for k in range(ch)], -1)
    a = a + rng.randint(-6, 7, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def valu_costs(exe):
    """{instruction: ns per wave-instruction per SIMD, the smallest over the occupancies measured}, and the raw text"""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("valu_rate failed:\n" + r.stdout + r.stderr)
    costs = {}
    for line in r.stdout.splitlines():
        name = line.split()[0] if line.split() else ""
        ns = [float(v) for v in re.findall(r"\(([0-9.]+) ns\)", line)]
        if name.startswith("v_") and ns:
            costs[name] = min(ns + ([costs[name]] if name in costs else []))
    return costs, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="teddy25,teddy23,hd23,hd23gray")
    ap.add_argument("--valu-rate", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilateral_time.json"))
    a = ap.parse_args()
    res = {"tool": "tools/bilateral_time.py", "rounds": ROUNDS, "reps": REPS, "cases": {}}
    costs = None
    if a.valu_rate:
        costs, raw = valu_costs(a.valu_rate)
        res["valu_rate"] = {"ns_per_wave_instruction_per_simd": costs, "output": raw.splitlines()}

    import numpy as np
    import torch
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import _lib
    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_name(0)
    names = a.sizes.split(",")
    for name in names:
        H, W, ch, wsize, ss, sc = SIZES[name]
        img = image(H, W, ch, 7)
        t = torch.from_numpy(img if ch == 3 else img[:, :, 0].copy()).to(dev)
        tabs = smt.bilateral_masks(wsize, ss, sc, dev)
        out = {}

        def form(impl):
            def f():
                smt.bilateral_set_impl(impl)
                out[impl] = smt.bilateralfiter(t, wsize, tables=tabs)
            return f

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            return e0.elapsed_time(e1)

        forms = [("staged", form(_lib.BILATERAL_FORM_STAGED)), ("direct", form(_lib.BILATERAL_FORM_DIRECT))]
        for _, fn in forms:
            fn(); fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in forms}
        for _ in range(ROUNDS):
            for k, fn in forms:
                for _ in range(REPS):
                    ms[k].append(timed(fn))
        smt.bilateral_set_impl(0)
        assert torch.equal(out[_lib.BILATERAL_FORM_STAGED], out[_lib.BILATERAL_FORM_DIRECT]), name
        taps = (2 * ((wsize[0] - 1) // 2) + 1) * (2 * ((wsize[1] - 1) // 2) + 1)
        samples = H * W * ch
        ops = samples * taps * 6
        case = {"H": H, "W": W, "channels": ch, "wsize": list(wsize), "sigma_space": ss, "sigma_color": sc, "taps": taps,
                "float64_operations": ops, "conversions": samples * taps,
                "ms": {k: stat(v) for k, v in ms.items()}}
        for k in ms:
            case["ms"][k]["float64_gop_per_s"] = ops / (case["ms"][k]["median"] * 1e-3) / 1e9
        case["faster"] = min(ms, key=lambda k: case["ms"][k]["median"])
        if costs and all(n in costs for n in ("v_mul_f64", "v_add_f64", "v_cvt_f64_u32")):
            per_tap = 4 * costs["v_mul_f64"] + 2 * costs["v_add_f64"] + costs["v_cvt_f64_u32"]
            floor_ms = (samples / 64.0) * taps * per_tap / SIMDS * 1e-6
            case["float64_issue_floor_ms"] = floor_ms
            case["staged_over_floor"] = case["ms"]["staged"]["median"] / floor_ms
        # the colour gather's bank behaviour: a flat image reads one entry (a broadcast), uniform noise spreads the 64 lanes
        # over all 256 entries (8 entries per pair of banks), the scene lies between
        case["staged_ms_by_content"] = {"scene": case["ms"]["staged"]["median"]}
        for content in ("flat", "noise"):
            other = np.full_like(img, 128) if content == "flat" else np.random.RandomState(3).randint(0, 256, img.shape).astype(np.uint8)
            to = torch.from_numpy(other if ch == 3 else other[:, :, 0].copy()).to(dev)
            smt.bilateral_set_impl(_lib.BILATERAL_FORM_STAGED)
            smt.bilateralfiter(to, wsize, tables=tabs)
            case["staged_ms_by_content"][content] = stat([timed(lambda: smt.bilateralfiter(to, wsize, tables=tabs)) for _ in range(7)])["median"]
            smt.bilateral_set_impl(0)
        if name == names[0] and not a.no_host:
            src = np.ascontiguousarray(img if ch == 3 else img[:, :, 0])
            sp, cm = (x.cpu().numpy() for x in tabs)
            dst = np.empty_like(src)
            vp = lambda x: x.ctypes.data_as(C.c_void_p)
            t0 = time.perf_counter()
            rc = _lib.lib().smt_bilateral_filter_host(vp(src), 1, H, W, ch, wsize[0], wsize[1], vp(sp), vp(cm), 0, vp(dst), None)
            case["host_twin_cpu_ms"] = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and np.array_equal(dst, out[_lib.BILATERAL_FORM_STAGED].cpu().numpy()), name
        res["cases"][name] = case
        print(name, {k: "%.3f [%.3f-%.3f]" % (v["median"], v["min"], v["max"]) for k, v in case["ms"].items()},
              {k: case[k] for k in ("float64_issue_floor_ms", "staged_over_floor", "host_twin_cpu_ms", "staged_ms_by_content") if k in case}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
