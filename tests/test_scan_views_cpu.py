"""The scanline optimiser on both views where there is no device (include/smt_scan_views.h):
the library exports what the header declares; the oracle's scanline on right-view inputs is the reference's own ScanLine
(oracle.ref_scanline_all where the reference build exists, hashes recorded from it in
tests/golden/scan_views_ref_hashes.json where it does not); the pipeline cases meet their input conditions on the oracle
alone; host/smt_scan_views.hpp compiles warning-free and holds its contract against a stub in a stand-alone program under
AddressSanitizer (nothing is loaded into Python)."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scan_views_cases as SV  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smt_scan_views.h")
HASHES = os.path.join(ROOT, "tests", "golden", "scan_views_ref_hashes.json")
SRC = os.path.join(ROOT, "tests", "cpp_mirror_scan_views")
NEW = ("smt_scanline_run_pair", "smt_scanline_run_map", "smt_pipeline_set_scan_views", "smt_pipeline_scan_right_volume")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _plain():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_new_entries_and_the_library_exports_them():
    from stereo_match_traditional_amd import _lib
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", _plain()))
    assert declared == set(NEW), declared ^ set(NEW)
    assert '#include "smt.h"' in _plain() and "__cplusplus" in _plain()
    smt_h = open(os.path.join(ROOT, "include", "smt.h")).read()
    for n in NEW:
        assert n not in smt_h, f"{n} is declared in smt.h as well"
        assert hasattr(_lib.lib(), n), n


def test_header_is_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "smt_scan_views.h"\nint main(void) { return smt_scanline_run_map(0, 0, 0, 0) == SMT_ERR_ARG ? 0 : 1; }\n')
    r = subprocess.run([shutil.which("gcc") or "cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only",
                        "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def right_view_inputs(O):
    """[(name, cost, gray)]: view 1 of every scanline shape, and the aggregated right volume with the float right image
    of the first pair of every pipeline case"""
    out = [("x".join(map(str, s)), *SV.inputs(*s, 1)) for s in SV.SHAPES]
    for case in SV.PIPE_CASES:
        L, R = SV.pipe_pairs(O, case)[0]
        out.append(("pipe_" + case["name"], SV.pipe_pair_oracle(O, case, 0)["vols"]["agg_right"], R.astype(np.float32)))
    return out


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_oracle_right_view_scanline_is_the_references(O):
    golden = json.load(open(HASHES))
    ins = right_view_inputs(O)
    assert sorted(golden) == sorted(n for n, _, _ in ins)
    for name, cost, gray in ins:
        s = O.scanline(cost, gray, SV.P1, SV.P2)
        d = O.wta(s)
        assert not np.isnan(s).any()
        if O.have_ref_adcensus():
            ref = O.ref_scanline_all(cost, gray, SV.P1, SV.P2)
            assert np.array_equal(ref["sum"].view(np.uint32), s.view(np.uint32)), name
            assert np.array_equal(ref["disp"], d), name
            assert golden[name] == dict(sum=_sha(ref["sum"]), disp=_sha(ref["disp"])), f"{name}: the recorded hashes are stale"
        else:
            assert golden[name] == dict(sum=_sha(s), disp=_sha(d)), name


@pytest.mark.parametrize("case", SV.PIPE_CASES, ids=[c["name"] for c in SV.PIPE_CASES])
def test_pipeline_cases_meet_their_conditions_on_the_oracle(O, case):
    SV.check_pipe_conditions(O, case)
    pairs = SV.pipe_pairs(O, case)
    assert len(pairs) == sum(SV.PIPE_BATCHES) and len({p[0].tobytes() + p[1].tobytes() for p in pairs}) == len(pairs)
    for k in range(2):                                       # sub-pixel right maps carry fractions
        dr = SV.pipe_pair_oracle(O, case, k, 1.0)["both"]["dr"]
        assert dr.dtype == np.float32 and dr.shape == (case["H"], case["W"])


def test_fixed_vertical_identity_restated(O):
    """scan_views_cases.scan_pass_ref against bounds_cases._scan_ref, which it restates"""
    import bounds_cases as BC
    cost, gray = SV.inputs(6, 10, 70, 1)
    for which in ("left", "right", "up", "down"):
        for fixed in (False, True):
            assert np.array_equal(SV.scan_pass_ref(O, cost, gray, which, fixed), BC._scan_ref(O, cost, gray, which, fixed))
    assert not np.array_equal(SV.scan_sum(O, cost, gray, True), SV.scan_sum(O, cost, gray, False))


def test_mirror_compiles_clean_and_holds_its_contract_under_asan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a C++ compiler is needed"
    exe = tmp_path / "scan_views_main"
    cmd = [cxx] + FLAGS + [os.path.join(SRC, "scan_views_stub.cpp"), os.path.join(SRC, "scan_views_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr         # -Wall -Wextra -Werror clean
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scan views: contract held" in r.stdout
