"""Regenerates tests/golden/ncc_whole_ref.npz: what the reference's own ncc() and bgr_to_grey() (NCC/NCC.h) return on the
seeded inputs of tests/ncc_whole_cases.py.

NCC.h is compiled unmodified, found through -I where the reference lies, against the container-only header
ncc_whole_ref/opencv2/opencv.hpp and the recording program ncc_whole_ref/record_main.cpp (both our own text).  The build
goes into a temporary directory that is removed afterwards: nothing compiled is kept.  The fixture holds recorded results
only -- the depth maps of both types for the six pairs and one bgr_to_grey image.  add_constant is not recorded (it is
OpenCV's `Mat += int`, an aborting stub in the container).

    python tests/golden/make_ncc_whole_golden.py [reference root]

exits cleanly, writing nothing, when the reference tree is absent."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

OUT = os.path.join(HERE, "ncc_whole_ref.npz")
DEFAULT_REFERENCE = os.environ.get("SMT_REFERENCE", "/root/reference")


def record(reference):
    """-> {name: array}, or None when the reference tree is absent; with the tree present a missing C++ compiler is an
    error that names the compiler looked for"""
    import ncc_whole_cases as WC
    ncc_dir = os.path.join(reference, "NCC")
    if not os.path.exists(os.path.join(ncc_dir, "NCC.h")):
        return None
    want = os.environ.get("CXX", "g++")
    cxx = shutil.which(want)
    if cxx is None:
        raise RuntimeError(f"the reference tree is at {reference} but no C++ compiler {want!r} was found (set CXX)")
    tmp = tempfile.mkdtemp(prefix="ncc_whole_ref_")
    try:
        exe = os.path.join(tmp, "record_main")
        # -O1 without contraction: every float64 operation of NCC.h stays the IEEE operation it is written as
        subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-w", "-I", os.path.join(HERE, "ncc_whole_ref"), "-I", ncc_dir,
                        os.path.join(HERE, "ncc_whole_ref", "record_main.cpp"), "-o", exe], check=True)

        def run(mode, H, W, data):
            r = subprocess.run([exe, mode, str(H), str(W)], input=data, stdout=subprocess.PIPE, check=True)
            return np.frombuffer(r.stdout, np.uint8).reshape(H, W).copy()

        out = {}
        for name, L, R in WC.fixture_pairs():
            H, W = L.shape
            for mode in ("left", "right"):
                out[f"{name}_{mode}"] = run(mode, H, W, L.tobytes() + R.tobytes())
        bgr = WC.fixture_bgr()
        out["grey"] = run("grey", bgr.shape[0], bgr.shape[1], bgr.tobytes())
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    out = record(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_REFERENCE)
    if out is None:
        print("the reference tree is absent: nothing written")
        return 0
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
