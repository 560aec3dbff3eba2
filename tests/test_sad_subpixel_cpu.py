"""Sub-pixel SAD where there is no device: the host twin smt_sad_subpixel_host (direct loops through the rule header the
kernels include) against the NumPy restatement of tests/sad_subpixel_cases.py on the whole table, bit for bit; the
restatement's integer winners against oracle.sad; the table's own claims; argument errors; exports and the C99 header."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import sad_subpixel_cases as SS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smt_sad_subpixel.h")
SMT_ERR_ARG = -1
NEW = ("smt_sad_subpixel", "smt_sad_both_subpixel", "smt_sad_subpixel_host", "smt_sad_flow_run_batch_subpixel")


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd import _lib
    _lib.lib()
    return _lib


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host(L, name, min_den, want=(True, True, True, True)):
    """the host twin into prefilled maps -> [dispL, dispR, winL, winR] (None where not asked for)"""
    Lp, Rp, D, ws = SS.pair(name)
    H, W = Lp.shape[0] - 2 * (ws + 1), Lp.shape[1] - 2 * (ws + 1)
    outs = [np.full((H, W), np.nan, np.float32) if want[0] else None, np.full((H, W), np.nan, np.float32) if want[1] else None,
            np.full((H, W), -77777777, np.int32) if want[2] else None, np.full((H, W), -77777777, np.int32) if want[3] else None]
    p = None if min_den is None else C.byref(L.SubpixelParams(min_den))
    rc = L.lib().smt_sad_subpixel_host(vp(Lp), vp(Rp), H, W, D, ws, p, *[vp(o) for o in outs])
    assert rc == 0, rc
    return outs


@pytest.mark.parametrize("name", SS.NAMES)
def test_the_restatements_winners_are_the_oracles(O, name):
    """the rows are pinned first: OptimalDisparity / GetMinSadIndex on them give oracle.sad's maps"""
    Lp, Rp, D, ws = SS.pair(name)
    _, _, winL, winR = SS.winners(name)
    assert np.array_equal(winL, O.sad(Lp, Rp, D, ws, 0)), "left"
    assert np.array_equal(winR, O.sad(Lp, Rp, D, ws, 1)), "right"


@pytest.mark.parametrize("name", SS.NAMES)
def test_host_twin_equals_the_restatement(L, O, name):
    Lp, Rp, D, ws = SS.pair(name)
    for min_den in SS.MIN_DENS:
        dl, dr, wl, wr = host(L, name, min_den)
        rl, rr, rwl, rwr = SS.restate(name, min_den)
        assert np.array_equal(wl, rwl) and np.array_equal(wr, rwr), min_den
        assert np.array_equal(wl, O.sad(Lp, Rp, D, ws, 0)) and np.array_equal(wr, O.sad(Lp, Rp, D, ws, 1)), min_den
        for got, ref, what in ((dl, rl, "dispL"), (dr, rr, "dispR")):
            bad = SS.bits(got) != SS.bits(ref)
            assert not bad.any(), (what, min_den, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_null_params_are_the_defaults_and_any_output_may_be_null(L):
    name = "D65"
    full = host(L, name, 1.0)
    for got, ref in zip(host(L, name, None), full):
        assert arena.same_bytes(got, ref)
    for k in range(4):
        only = host(L, name, 1.0, tuple(j == k for j in range(4)))
        assert arena.same_bytes(only[k], full[k]) and all(only[j] is None for j in range(4) if j != k)


def test_host_twin_in_the_arena(L):
    """guards on both sides of every tensor, both prefill seeds, the inputs untouched"""
    for name in ("W65-H7", "D130", "win8-sat"):
        Lp, Rp, D, ws = SS.pair(name)
        H, W = Lp.shape[0] - 2 * (ws + 1), Lp.shape[1] - 2 * (ws + 1)

        def make(A):
            A.inp("Lp", Lp); A.inp("Rp", Rp)
            for n, dt in (("dispL", np.float32), ("dispR", np.float32), ("winL", np.int32), ("winR", np.int32)):
                A.out(n, (H, W), dt)
            return lambda A: L.lib().smt_sad_subpixel_host(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, C.byref(L.SubpixelParams(64.0)),
                                                           A.ptr("dispL"), A.ptr("dispR"), A.ptr("winL"), A.ptr("winR"))
        out, _ = arena.run_two_seeds(make)
        rl, rr, wl, wr = SS.restate(name, 64.0)
        assert np.array_equal(SS.bits(out["dispL"]), SS.bits(rl)) and np.array_equal(SS.bits(out["dispR"]), SS.bits(rr)), name
        assert np.array_equal(out["winL"], wl) and np.array_equal(out["winR"], wr), name


def test_the_table_holds_what_it_says():
    seen_chain = seen_tail = seen_frac = 0
    for name in SS.NAMES:
        Lp, Rp, D, ws = SS.pair(name)
        rowsL, rowsR, winL, winR = SS.winners(name)
        H, W = winL.shape
        x = np.arange(W)[None, :]
        seen_chain += int(((winL == x) & (winL > 0)).sum())                  # r == x: the winner is the chain's first entry
        dmax = np.minimum(D - 1, W - 1 - x)
        real = np.zeros((H, W), bool); real[:H - 1, :W - 1] = True
        seen_tail += int((real & (winR == dmax) & (dmax < D - 1) & (winR > 0)).sum())   # w == dmax: row[w + 1] is the copy
        dl, dr, _, _ = SS.restate(name, 1.0)
        seen_frac += int((dl != np.floor(dl)).sum() + (dr != np.floor(dr)).sum())
        if name.startswith("planted-"):
            d0 = int(name.split("-")[1])
            w = ws + 1                                                       # windows clear of the replicated border
            xs, xr = slice(d0 + w, W - w), slice(w, W - d0 - w)
            assert (winL[:, xs] == d0).all() and (rowsL[:, xs, d0] == 0).all(), name
            assert (winR[:H - 1, xr] == d0).all() and (rowsR[:H - 1, xr, d0] == 0).all(), name
            assert (dl[:, xs] != d0).any() and (dr[:H - 1, xr] != d0).any(), name   # the parabola moves them
        if name == "win8-sat":
            assert (rowsL == 19 * 19 * 255).all() and (winL == 65535).all() and (dl == np.float32(65535)).all()
            assert (winR == 0).all() and (dr == 0).all()
        if name == "tie-0":
            assert (winL == 0).all() and (winR == 0).all()                     # equal minima: left 0, right the first
            assert (rowsL[:, 10:W - 2, 4] == 0).all() and (rowsL[:, 10:W - 2, 8] == 0).all()
        if name == "tie-2":
            assert (winR[:-1, 2:40] == 2).all() and (rowsR[:-1, 2:40, 6] == 0).all()
    assert seen_chain > 0, "no case has r == x"
    assert seen_tail > 0, "no right pixel has w == dmax < D - 1"
    assert seen_frac > 2000
    assert {1, 62, 63, 64, 65, 127, 128, 129, SS.PLANTED_D - 2} == set(SS.PLANTED)


def test_argument_errors(L):
    l = L.lib()
    Lp, Rp, D, ws = SS.pair("win1")
    H, W = Lp.shape[0] - 4, Lp.shape[1] - 4
    d = np.zeros((H, W), np.float32)
    ok = C.byref(L.SubpixelParams(1.0))
    a, b, dp = vp(Lp), vp(Rp), vp(d)
    for hh, ww, dd, w_ in ((0, W, D, ws), (H, 0, D, ws), (H, W, 0, ws), (-1, W, D, ws), (H, -3, D, ws), (H, W, -8, ws), (H, W, 513, ws),
                           (H, W, D, -1)):
        assert l.smt_sad_subpixel_host(a, b, hh, ww, dd, w_, ok, dp, dp, None, None) == SMT_ERR_ARG, (hh, ww, dd, w_)
        # the device entries reject before any HIP call
        assert l.smt_sad_subpixel(a, b, hh, ww, dd, w_, L.VIEW_LEFT, ok, dp, None, None) == SMT_ERR_ARG, (hh, ww, dd, w_)
        assert l.smt_sad_both_subpixel(a, b, hh, ww, dd, w_, ok, dp, dp, None, None, None, None) == SMT_ERR_ARG, (hh, ww, dd, w_)
    for m in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        bad = C.byref(L.SubpixelParams(m))
        assert l.smt_sad_subpixel_host(a, b, H, W, D, ws, bad, dp, dp, None, None) == SMT_ERR_ARG, m
        assert l.smt_sad_subpixel(a, b, H, W, D, ws, L.VIEW_RIGHT, bad, dp, None, None) == SMT_ERR_ARG, m
        assert l.smt_sad_both_subpixel(a, b, H, W, D, ws, bad, dp, dp, None, None, None, None) == SMT_ERR_ARG, m
    assert l.smt_sad_subpixel_host(None, b, H, W, D, ws, ok, dp, dp, None, None) == SMT_ERR_ARG
    assert l.smt_sad_subpixel_host(a, None, H, W, D, ws, ok, dp, dp, None, None) == SMT_ERR_ARG
    assert l.smt_sad_subpixel(None, b, H, W, D, ws, L.VIEW_LEFT, ok, dp, None, None) == SMT_ERR_ARG
    assert l.smt_sad_subpixel(a, b, H, W, D, ws, L.VIEW_LEFT, ok, None, None, None) == SMT_ERR_ARG
    assert l.smt_sad_subpixel(a, b, H, W, D, ws, 0, ok, dp, None, None) == SMT_ERR_ARG          # neither view
    assert l.smt_sad_both_subpixel(a, b, H, W, D, ws, ok, None, dp, None, None, None, None) == SMT_ERR_ARG
    assert l.smt_sad_both_subpixel(a, b, H, W, D, ws, ok, dp, None, None, None, None, None) == SMT_ERR_ARG
    assert l.smt_sad_flow_run_batch_subpixel(None, a, b, 1, ok, dp, dp, dp, None) == SMT_ERR_ARG
    assert l.smt_sad_subpixel_host(a, b, H, W, D, ws, ok, dp, None, None, None) == 0


def test_the_header_declares_what_the_library_exports_and_is_c99(L, tmp_path):
    hdr = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", plain))
    assert declared == set(NEW), declared ^ set(NEW)
    for name in NEW:
        assert hasattr(L.lib(), name), name
    assert "//" not in plain, "the header stays plain C: no // comments"
    assert '#include "smt.h"' in plain and "__cplusplus" in plain
    # nothing of it entered the two enumerated surfaces
    smt_h = open(os.path.join(ROOT, "include", "smt.h")).read()
    assert not any(n in smt_h for n in NEW)
    src = tmp_path / "c99.c"
    src.write_text('#include "smt_sad_subpixel.h"\nint main(void) { return smt_sad_subpixel_host(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == SMT_ERR_ARG ? 0 : 1; }\n')
    lib_dir = os.path.join(ROOT, "stereo_match_traditional_amd", "lib")
    exe = tmp_path / "c99"
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L" + lib_dir, "-lsmt_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_cpp_mirror_compiles_beside_smt_host(tmp_path):
    src = tmp_path / "m.cpp"
    src.write_text('#include "smt_sad_subpixel.hpp"\nint main() { return sizeof(smt::SadSubpixelFlow) && &smt::GetPointDepthSubpixel && '
                   '&smt::GetPointDepthBothSubpixel ? 0 : 1; }\n')
    lib_dir = os.path.join(ROOT, "stereo_match_traditional_amd", "lib")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "stereo_match_traditional_amd", "host"),
                        str(src), "-o", str(tmp_path / "m"), "-L" + lib_dir, "-lsmt_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
