#!/usr/bin/env python3
"""Generates tests/golden/*.npz.  Run in the build container (needs /root/reference for the
CrossAggregator fixtures, whose expected outputs come from the reference's own
cross_aggregator.cpp compiled into oracle/_ref by oracle/Makefile).

The AD-Census LUT fixture records the two expf tables of this image's glibc so that a
different libm on a GPU node would be noticed.

crossagg_ref_hashes.json records FNV-1a hashes (orc_fnv1a) of the reference build's CrossAggregator
outputs on the cases of tests/test_cpu_oracle.py::test_crossagg_oracle_vs_reference_build, so that the
oracle stays pinned to the reference where oracle/_ref cannot be built.
`python tests/golden/make_golden.py ref-hashes` writes only that file.

ref_pin_hashes.json does the same for the reference's own AD-CensusV1 and CBLSM.h code (oracle/_ref/libadcensus_ref.so,
libcblsm_ref.so) on the cases of tests/golden/ref_pin_cases.py: per case its parameters, the hashes of its inputs and
the hashes of every output of the reference builds (NaN canonicalised, see ref_pin_cases.canon).  Hashes only, no
arrays.  `python tests/golden/make_golden.py ref-pin` writes only that file; `ref-pin-dump DIR` writes the admitted
cases' inputs for the sanitizer run of the reference builds (`make -C oracle ref-asan`).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402


def main():
    O.build()
    assert O.have_ref(), "oracle/_ref missing: needs /root/reference"
    cases = [("a", 40, 56, 8, 7, False, (34, 17, 20, 6, 4)),
             ("b", 33, 47, 5, 11, True, (34, 17, 20, 6, 4)),
             ("c", 36, 90, 24, 3, False, (20, 9, 25, 8, 3))]
    for tag, H, W, D, seed, noise, prm in cases:
        L, _ = O.synth_pair(H, W, 16, seed, noise)
        bgr = O.synth_bgr(L, seed + 5)
        cost = (np.random.default_rng(seed).random((H, W, D), dtype=np.float32) * 2).astype(np.float32)
        arms, out = O.ref_crossagg(bgr, cost, *prm)
        np.savez_compressed(os.path.join(HERE, f"crossagg_{tag}.npz"), bgr=bgr, cost_init=cost, arms=arms,
                            cost_out=out, params=np.array(prm, np.int32))
    a, c = O.fuse_luts(10.0, 30.0)
    np.savez(os.path.join(HERE, "adcensus_luts_sc10_ss30.npz"), lutA=a, lutC=c)
    print("golden fixtures written")


# the cases of test_crossagg_oracle_vs_reference_build (default parameters 34, 17, 20, 6)
REF_HASH_CASES = [(40, 56, 8, 7, False), (33, 47, 5, 11, True), (48, 64, 16, 3, False)]
REF_HASH_ITERS = (1, 4)


def ref_hash_inputs(H, W, D, seed, noise):
    L, _ = O.synth_pair(H, W, D, seed, noise)
    bgr = O.synth_bgr(L, seed + 5)
    cost = np.random.default_rng(seed).random((H, W, D), dtype=np.float32) * 2
    return bgr, cost


def ref_hashes():
    O.build()
    assert O.have_ref(), "oracle/_ref missing: make -C oracle ref REF=<reference tree>"
    hx = lambda a: "%016x" % O.fnv1a(a)
    recs = []
    for (H, W, D, seed, noise) in REF_HASH_CASES:
        bgr, cost = ref_hash_inputs(H, W, D, seed, noise)
        for iters in REF_HASH_ITERS:
            arms, out = O.ref_crossagg(bgr, cost, iters=iters)
            recs.append({"H": H, "W": W, "D": D, "seed": seed, "noise": noise, "iters": iters,
                         "bgr": hx(bgr), "cost_init": hx(cost), "arms": hx(arms), "cost": hx(out)})
    with open(os.path.join(HERE, "crossagg_ref_hashes.json"), "w") as f:
        json.dump({"produced_by": "reference build (oracle/_ref/libcrossagg_ref.so), parameters 34 17 20 6",
                   "cases": recs}, f, indent=1)
        f.write("\n")
    print("crossagg_ref_hashes.json written")


def _ref_pin_cases():
    sys.path.insert(0, HERE)
    import ref_pin_cases as RP
    return RP


def ref_pin():
    RP = _ref_pin_cases()
    O.build()
    assert O.have_ref_adcensus() and O.have_ref_cblsm(), "oracle/_ref missing: make -C oracle ref REF=<reference tree>"
    recs = []
    for case in RP.CASES:
        inp = RP.inputs(case, O)
        assert RP.admitted(case, inp, O), "%s: the reference is undefined on this case; take it off the list" % case["name"]
        out = RP.run(case, inp, O, "ref")
        recs.append({"case": {k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items()},
                     "inputs": RP.hashes(inp, O), "outputs": RP.hashes(out, O)})
    with open(os.path.join(HERE, "ref_pin_hashes.json"), "w") as f:
        json.dump({"produced_by": "reference builds (oracle/_ref/libadcensus_ref.so, libcblsm_ref.so); orc_fnv1a, "
                                  "NaN hashed as 0x7fc00000", "cases": recs}, f, indent=1)
        f.write("\n")
    print("ref_pin_hashes.json written (%d cases)" % len(recs))


def ref_pin_dump(out_dir):
    """Inputs of every admitted case as raw files + a manifest for oracle/ref_build/ref_asan_main.cpp:
    one line per case, `kind name p0..p7 file...`; arrays little-endian, C order."""
    RP = _ref_pin_cases()
    O.build()
    os.makedirs(out_dir, exist_ok=True)
    lines = []
    for case in RP.CASES:
        inp = RP.inputs(case, O)
        if not RP.admitted(case, inp, O):
            continue
        k = case["kind"]
        g = lambda n: int(case.get(n, 0))
        prm = {"adcensus": [g("H"), g("W"), g("D")],
               "arms": [g("H"), g("W"), g("ch"), g("tau"), len(case.get("dirs", ()))] + list(case.get("dirs", ())),
               "agg": [g("H"), g("W"), g("D"), g("order")],
               "scan": [g("H"), g("W"), g("D"), g("p1"), g("p2")],
               "lrcheck": [g("H"), g("W"), g("gate")], "lrvariant": [g("H"), g("W"), g("gate")],
               "fill": [g("row"), g("col"), g("D"), len(inp.get("occ", ())), len(inp.get("mis", ()))],
               "speckle": [g("H"), g("W"), g("diff"), g("area"), g("inv")],
               "median": [g("H"), g("W"), g("wnd")],
               "cblsm_arms": [g("H"), g("W"), g("ch"), g("tau")],
               "cblsm_ad": [g("H"), g("W"), g("D")], "cblsm_disp": [g("H"), g("W"), g("D")],
               "choose": [g("H"), g("W"), g("D")]}[k]
        prm = (prm + [0] * 9)[:9]
        files = []
        for name, a in inp.items():
            fn = "%s.%s.bin" % (case["name"], name)
            np.ascontiguousarray(a).tofile(os.path.join(out_dir, fn))
            files.append(fn)
        lines.append(" ".join([k, case["name"]] + [str(v) for v in prm] + [str(len(files))] + files))
    with open(os.path.join(out_dir, "manifest.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases dumped to %s" % (len(lines), out_dir))


if __name__ == "__main__":
    if sys.argv[1:] == ["ref-hashes"]:
        ref_hashes()
    elif sys.argv[1:] == ["ref-pin"]:
        ref_pin()
    elif sys.argv[1:2] == ["ref-pin-dump"] and len(sys.argv) == 3:
        ref_pin_dump(sys.argv[2])
    else:
        main()
