"""Records tests/golden/fill_holes_ref.npz from the reference's own FillHolesInDispMap (SAD/Sad.h:317-400).

    python tests/golden/make_fill_holes_golden.py /path/to/reference

Compiles tests/golden/fill_holes_ref/record_main.cpp, which includes SAD/Sad.h unmodified from the reference tree,
against the container-only opencv2/opencv.hpp beside it (no OpenMP, so the pragma on the pass loop is ignored), runs it
on the maps below and stores, per map k: in_k, invalid_k, occ_k, mis_k, pass0_k, pass1_k, pass2_k; and `constants`, sinf and
cosf of the eight float32 angles from the C library that build links (through ctypes: the function's sin(float) and
cos(float) are those calls).  Only data is stored; the program is built in a temporary
directory and deleted."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fill_holes_cases as FH  # noqa: E402

SHAPES = [(2, 3, 50), (5, 7, 51), (9, 33, 52), (17, 40, 53), (48, 64, 54), (31, 64, 55), (48, 5, 56), (24, 24, 57)]
# std::sort leaves the order of -0.0f and +0.0f open and the library writes +0.0f (include/smt_fill_holes.h), so only the
# last map holds a -0.0f: the test compares that one with the sign of zero put aside, every other one bit for bit


def maps():
    out = []
    for H, W, seed in SHAPES:
        M, cls = FH.case(H, W, seed, neg_zero=False)
        out.append((M, cls, FH.INF))
    for name in ("borders", "listed_valid", "occ_two_values", "mis_two_values", "all_holes"):
        M, cls, inv, _ = FH.crafted()[name]
        out.append((M, cls, inv))
    M, cls = FH.case(9, 33, 58, invalid=FH.INT_MIN_F, neg_zero=False)
    out.append((M, cls, FH.INT_MIN_F))
    M, cls = FH.case(9, 33, 59, invalid=0.0)
    out.append((M, cls, 0.0))
    M, cls = FH.case(24, 24, 57)                                       # with -0.0f
    out.append((M, cls, FH.INF))
    return out


def main(ref):
    ms = maps()
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, n) for n in ("record", "in.bin", "out.bin"))
        cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-I" + os.path.join(HERE, "fill_holes_ref"),
               "-I" + os.path.join(ref, "SAD"), os.path.join(HERE, "fill_holes_ref", "record_main.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(ms)))
            for M, cls, inv in ms:
                occ, mis = FH.lists_of(cls)
                f.write(struct.pack("<iiiif", M.shape[0], M.shape[1], len(occ), len(mis), inv))
                f.write(np.ascontiguousarray(M, np.float32).tobytes())
                f.write(np.array(occ, np.int32).reshape(-1, 2).tobytes())
                f.write(np.array(mis, np.int32).reshape(-1, 2).tobytes())
        subprocess.run([exe, fin, fout], check=True)
        raw = np.fromfile(fout, np.float32)
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    m.sinf.restype = m.cosf.restype = ctypes.c_float
    m.sinf.argtypes = m.cosf.argtypes = [ctypes.c_float]
    consts = np.array([m.sinf(float(a)) for a in FH.ANGLE1] + [m.cosf(float(a)) for a in FH.ANGLE1], np.float32)
    rec = {"count": np.int32(len(ms)), "constants": consts, "negative_zero_map": np.int32(len(ms) - 1)}
    at = 0
    for k, (M, cls, inv) in enumerate(ms):
        n = M.size
        occ, mis = FH.lists_of(cls)
        rec[f"in_{k}"], rec[f"invalid_{k}"] = np.ascontiguousarray(M, np.float32), np.float32(inv)
        rec[f"occ_{k}"], rec[f"mis_{k}"] = np.array(occ, np.int32).reshape(-1, 2), np.array(mis, np.int32).reshape(-1, 2)
        for p in range(3):
            rec[f"pass{p}_{k}"] = raw[at:at + n].reshape(M.shape).copy()
            at += n
    assert at == raw.size
    np.savez_compressed(os.path.join(HERE, "fill_holes_ref.npz"), **rec)
    print("wrote", len(ms), "maps")


if __name__ == "__main__":
    main(sys.argv[1])
