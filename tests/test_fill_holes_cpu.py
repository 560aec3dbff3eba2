"""Sad.h's FillHolesInDispMap where there is no device: the NumPy restatement of tests/fill_holes_cases.py and the host
twin smt_fill_holes_batch_host (raster-order loops through the rule header the kernel includes) against the recorded
results of the reference's own code (tests/golden/fill_holes_ref.npz), pass by pass; the host twin against the
restatement over the case table and the crafted cases, bit for bit on maps and status; the sixteen constants against the
host's sinf / cosf and the fixture; the ordering property the device wavefront rests on, re-derived through the
library's own probe function; angle2 immaterial; several maps, strides and guards; argument errors; exports, the C99
header, the Python names; the C++ mirror against a contract stub under AddressSanitizer."""
import ctypes as C
import ctypes.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import fill_holes_cases as FH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smt_fill_holes.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "fill_holes_ref.npz")
MIRROR = os.path.join(ROOT, "tests", "cpp_mirror_fill_holes")
NEW = ("smt_fill_holes_batch", "smt_fill_holes_batch_host", "smt_fill_holes_constants", "smt_fill_holes_probe",
       "smt_fill_holes_walk", "smt_fill_holes_host_passes", "smt_pipeline_run_batch_filled")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
F = np.float32


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def host(L, M, cls, invalid=FH.INF):
    """the host twin on one map into a prefilled status -> (map, status)"""
    H, W = M.shape
    m = np.ascontiguousarray(M, F).copy()
    status = np.full(4, -77, np.int32)
    z = C.c_size_t(0)
    rc = L.lib().smt_fill_holes_batch_host(vp(m), vp(np.ascontiguousarray(cls, np.uint8)), 1, z, z, H, W, C.c_float(invalid),
                                           vp(status))
    assert rc == 0, rc
    return m, status


def same(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, "map", np.argwhere(bits(got[0]) != bits(want[0]))[:4].tolist())
    assert list(got[1]) == list(want[1]), (what, "status", list(got[1]), list(want[1]))


# ---- the pin: the reference's own code, recorded -----------------------------------------------------------------------
def test_the_constants(L, golden):
    """the rule header's literals == the restatement's == the host's sinf / cosf == what the reference's build computed"""
    got = np.zeros(16, F)
    L.lib().smt_fill_holes_constants(vp(got))
    assert np.array_equal(bits(got), bits(FH.constants()))
    m = C.CDLL(ctypes.util.find_library("m"))
    m.sinf.restype = m.cosf.restype = C.c_float
    m.sinf.argtypes = m.cosf.argtypes = [C.c_float]
    libm = np.array([m.sinf(float(a)) for a in FH.ANGLE1] + [m.cosf(float(a)) for a in FH.ANGLE1], F)
    assert np.array_equal(bits(got), bits(libm))
    assert np.array_equal(bits(got), bits(golden["constants"]))
    # what the kernel's ordering rests on: the three near-zero constants are positive, so the axis rays stay on their
    # row or column; sinf(pi) is the value the header names
    assert got[0] == F(float.fromhex("0x1.4442d2p-23")) and got[8 + 2] > 0 and got[8 + 6] > 0 and got[4] == 0
    # angle2 holds the same eight angles
    assert sorted(bits(np.array(FH.ANGLE1, F)).tolist()) == sorted(bits(np.array(FH.ANGLE2, F)).tolist())


def test_restatement_and_host_twin_equal_the_reference_pass_by_pass(L, golden):
    n = int(golden["count"])
    assert n >= 10
    nz = int(golden["negative_zero_map"])
    assert np.signbit(golden[f"in_{nz}"][golden[f"in_{nz}"] == 0]).any()
    assert not any(np.signbit(golden[f"in_{k}"][golden[f"in_{k}"] == 0]).any() for k in range(n) if k != nz)

    def bits(a, k=None):
        # the one map with -0.0f: std::sort leaves the order of the two zeros open, the library writes +0.0f
        a = np.ascontiguousarray(a, F)
        return (a + F(0.0) if k == nz else a).view(np.uint32)
    for k in range(n):
        M, invalid = golden[f"in_{k}"], float(golden[f"invalid_{k}"])
        occ, mis = golden[f"occ_{k}"].reshape(-1, 2), golden[f"mis_{k}"].reshape(-1, 2)
        H, W = M.shape
        assert H <= 48 and W <= 64
        cls = np.zeros((H, W), np.uint8)
        cls[occ[:, 0], occ[:, 1]] = 1
        cls[mis[:, 0], mis[:, 1]] = 2
        assert FH.lists_of(cls) == ([tuple(p) for p in occ.tolist()], [tuple(p) for p in mis.tolist()]), k   # raster order, disjoint
        after, st = FH.fill_holes(M, cls, invalid)
        for p in range(3):
            assert np.array_equal(bits(after[p], k), bits(golden[f"pass{p}_{k}"], k)), (k, p)
        for p in range(3):
            m = np.ascontiguousarray(M, F).copy()
            assert L.lib().smt_fill_holes_host_passes(vp(m), vp(cls), H, W, C.c_float(invalid), p + 1) == 0
            assert np.array_equal(bits(m, k), bits(golden[f"pass{p}_{k}"], k)), (k, p, "host twin")
        m, got_st = host(L, M, cls, invalid)
        assert np.array_equal(bits(m, k), bits(golden[f"pass2_{k}"], k)) and list(got_st) == list(st), (k, "host twin")
    assert any((golden[f"pass0_{k}"] != golden[f"pass1_{k}"]).any() for k in range(n))
    assert any((bits(golden[f"pass1_{k}"]) != bits(golden[f"pass2_{k}"])).any() for k in range(n))


# ---- host twin against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", [t[0] for t in FH.TABLE])
def test_host_twin_equals_the_restatement(L, gid):
    M, cls = FH.table_case(gid)
    after, st = FH.table_expected(gid)
    same(host(L, M, cls), (after[2], st), gid)


CRAFTED = FH.crafted()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted(L, name):
    M, cls, invalid, chk = CRAFTED[name]
    after, st = FH.expected(("crafted", name), M, cls, invalid)
    assert chk is None or chk(after, st), name
    same(host(L, M, cls, invalid), (after[2], st), name)


def test_the_run_of_holes_tells_in_place_from_collect_then_write():
    M, cls, invalid, _ = CRAFTED["run_1x9"]
    occ, mis = FH.lists_of(cls)
    in_place, _ = FH.fill_holes_lists(M, occ, mis, invalid)
    jacobi, _ = FH.fill_holes_lists(M, occ, mis, invalid, collect_then_write=True)
    assert (in_place[1][0, :8] == 3).all()                         # every pixel took its left neighbour's fresh fill
    assert not np.array_equal(bits(in_place[1]), bits(jacobi[1]))
    assert jacobi[1][0, 1] == 3 and (jacobi[1][0, 2:] == 7).all()


def test_the_table_reaches_every_branch():
    seen = set()
    for gid, H, W, seed in FH.TABLE:
        M, cls = FH.table_case(gid)
        after, st = FH.table_expected(gid)
        hole = np.isinf(M)
        if (cls[hole] == 0).any():
            seen.add("third pass only")
        if (cls[~hole] == 1).any() or (cls[~hole] == 2).any():
            seen.add("listed and valid")
        if np.isinf(after[2]).any():
            seen.add("left a hole")
        if (bits(after[0]) != bits(M)).any() and (bits(after[1]) != bits(after[0])).any() and (bits(after[2]) != bits(after[1])).any():
            seen.add("every pass writes")
    assert seen >= {"third pass only", "listed and valid", "every pass writes"}, seen


def test_angle2_is_immaterial():
    for gid in ("9x33", "17x65"):
        M, cls = FH.table_case(gid)
        with_switch = FH.table_expected(gid)[0]
        without, _ = FH.fill_holes(M, cls, use_angle2=False)
        assert any(y == M.shape[0] // 2 for y, _ in sum(FH.lists_of(cls), []))   # the switch happens
        for p in range(3):
            assert np.array_equal(bits(with_switch[p]), bits(without[p])), (gid, p)


# ---- the ordering property of the wavefront ----------------------------------------------------------------------------
def walk(L, H, W, y, x, ray):
    """the pixels ray `ray` of (y, x) can touch in an H x W image, through the library's probe (the rule header)"""
    cap = 2 * max(H, W) + 8
    yy, xx = np.empty(cap, np.int32), np.empty(cap, np.int32)
    n = L.lib().smt_fill_holes_walk(H, W, y, x, ray, vp(yy), vp(xx), cap)
    assert n >= 0, "a ray that does not leave"
    return list(zip(yy[:n].tolist(), xx[:n].tolist()))


def ordering_holds(L, H, W, pixels, skew):
    """every pixel a ray touches that is earlier in raster order has a strictly smaller step skew * i + j, every later
    one an equal or larger step"""
    for (y, x) in pixels:
        s = skew * y + x
        for ray in range(8):
            for (yy, xx) in walk(L, H, W, y, x, ray):
                t = skew * yy + xx
                if (yy, xx) < (y, x):
                    if not t < s:
                        return False
                elif (yy, xx) > (y, x):
                    if not t >= s:
                        return False
    return True


def test_probe_equals_the_restatement(L):
    yy, xx = C.c_int(), C.c_int()
    c = FH.constants()
    for (y, x, n) in ((0, 0, 1), (5, 7, 3), (1079, 1919, 1500), (8191, 8191, 11000), (1, 1, 1), (4096, 1, 2)):
        for ray in range(8):
            assert L.lib().smt_fill_holes_probe(y, x, ray, n, C.byref(yy), C.byref(xx)) == 0
            assert (yy.value, xx.value) == (FH.probe(y, n, c[ray]), FH.probe(x, n, c[8 + ray])), (y, x, n, ray)
    for ray in range(8):                                           # the walk is the probes up to the first one outside
        got = walk(L, 40, 50, 17, 23, ray)
        for n, p in enumerate(got + [None], 1):
            q = (FH.probe(17, n, c[ray]), FH.probe(23, n, c[8 + ray]))
            assert p == q if p is not None else not (0 <= q[0] < 40 and 0 <= q[1] < 50), (ray, n)
    assert L.lib().smt_fill_holes_probe(0, 0, 8, 1, C.byref(yy), C.byref(xx)) == FH.ERR_ARG
    assert L.lib().smt_fill_holes_probe(0, 0, 0, 0, C.byref(yy), C.byref(xx)) == FH.ERR_ARG


def test_skew_two_orders_every_ray_of_a_small_grid_and_skew_one_does_not(L):
    H, W = 40, 50
    every = [(y, x) for y in range(H) for x in range(W)]
    assert ordering_holds(L, H, W, every, 2)
    assert not ordering_holds(L, H, W, every, 1)
    # the axis rays stay on their row / column, and the border self-visit exists
    assert all(p[0] == 7 for ray in (0, 4) for p in walk(L, H, W, 7, 20, ray))
    assert all(p[1] == 20 for ray in (2, 6) for p in walk(L, H, W, 7, 20, ray))
    assert walk(L, H, W, 0, 9, 6) == [] and walk(L, H, W, 0, 9, 5) == [(0, 9)] and walk(L, H, W, 4, 0, 7) == [(3, 0)]


@pytest.mark.parametrize("H,W", [(1100, 2000), (FH.MAX_DIM, FH.MAX_DIM)], ids=["1100x2000", "max"])
def test_skew_two_orders_border_and_sampled_pixels_of_a_large_grid(L, H, W):
    rng = np.random.default_rng(H)
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (1, 1), (H - 2, W - 2)]
    for _ in range(6):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        pixels += [(0, x), (H - 1, x), (y, 0), (y, W - 1), (y, x)]
    assert ordering_holds(L, H, W, pixels, 2)
    # the axis rays of the far corner stay on their row and column for the whole extent
    assert all(p[0] == H - 1 for p in walk(L, H, W, H - 1, W - 1, 0)) and all(p[1] == W - 1 for p in walk(L, H, W, H - 1, W - 1, 6))


# ---- the contract on the host --------------------------------------------------------------------------------------------
def test_three_maps_strides_and_guards_on_the_host(L):
    H, W = 9, 33
    N = H * W
    cases = [FH.case(H, W, s) for s in (4, 21, 22)]
    z = C.c_size_t

    def make(A):
        A.inout("maps", np.stack([c[0] for c in cases]), stride=N + 5)
        A.inp("cls", np.stack([c[1] for c in cases]), stride=N + 7)
        A.out("status", (3, 4), np.int32)
        return lambda A: L.lib().smt_fill_holes_batch_host(A.ptr("maps"), A.ptr("cls"), 3, z(N + 5), z(N + 7), H, W,
                                                           C.c_float(FH.INF), A.ptr("status"))
    out, _ = arena.run_two_seeds(make)
    for k, c in enumerate(cases):
        after, st = FH.fill_holes(*c)
        same((out["maps"][k], out["status"][k]), (after[2], st), k)
        same(host(L, *c), (after[2], st), (k, "one call"))


def test_a_nan_map_beside_a_clean_one_on_the_host(L):
    maps, cls = FH.nan_pair()
    m = maps.copy()
    status = np.full((2, 4), -77, np.int32)
    z = C.c_size_t(0)
    assert L.lib().smt_fill_holes_batch_host(vp(m), vp(cls), 2, z, z, 9, 33, C.c_float(FH.INF), vp(status)) == 0
    assert np.array_equal(bits(m[0]), bits(maps[0])) and status[0, 3] == FH.UB_NAN and status[0, 2] == 0
    after, st = FH.fill_holes(maps[1], cls[1])
    same((m[1], status[1]), (after[2], st), "the clean map")
    assert list(FH.fill_holes(maps[0], cls[0])[1]) == list(status[0])


def test_argument_errors(L):
    l = L.lib()
    H, W = 4, 5
    m, c, st = np.zeros((H, W), F), np.zeros((H, W), np.uint8), np.zeros(4, np.int32)
    z = C.c_size_t
    inf = C.c_float(FH.INF)
    for fn, tail in ((l.smt_fill_holes_batch_host, ()), (l.smt_fill_holes_batch, (None,))):
        def call(maps=vp(m), cls=vp(c), pairs=1, ms=0, cs=0, h=H, w=W, invalid=inf):
            return fn(maps, cls, pairs, z(ms), z(cs), h, w, invalid, vp(st) if not tail else None, *tail)
        assert call(maps=None) == FH.ERR_ARG and call(cls=None) == FH.ERR_ARG
        assert call(pairs=-1) == FH.ERR_ARG
        assert call(h=0) == FH.ERR_ARG and call(w=0) == FH.ERR_ARG and call(h=-3) == FH.ERR_ARG
        assert call(h=FH.MAX_DIM + 1) == FH.ERR_ARG and call(w=FH.MAX_DIM + 1) == FH.ERR_ARG
        assert call(ms=H * W - 1) == FH.ERR_ARG and call(cs=H * W - 1) == FH.ERR_ARG
        assert call(invalid=C.c_float(float("nan"))) == FH.ERR_ARG
        assert call(pairs=0) == 0                                   # a no-op: no device is touched
    assert l.smt_fill_holes_batch_host(vp(m), vp(c), 1, z(0), z(0), H, W, inf, None) == 0     # status may be NULL
    assert l.smt_pipeline_run_batch_filled(None, vp(c), vp(c), 1, vp(m), vp(m), vp(c), None, 3, inf, None, None) == FH.ERR_ARG
    l.smt_fill_holes_constants(None)


def test_the_header_declares_what_the_library_exports_and_is_c99(L, tmp_path):
    hdr = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", plain))
    assert declared == set(NEW), declared ^ set(NEW)
    for name in NEW:
        assert hasattr(L.lib(), name), name
    assert "//" not in plain, "the header stays plain C: no // comments"
    assert '#include "smt.h"' in plain and "__cplusplus" in plain
    smt_h = open(os.path.join(ROOT, "include", "smt.h")).read()
    assert not any(n in smt_h for n in NEW) and "smt_fill_holes" not in smt_h
    src = tmp_path / "c99.c"
    src.write_text('#include "smt_fill_holes.h"\nint main(void) { float c[16]; smt_fill_holes_constants(c);\n'
                   ' return smt_fill_holes_batch_host(0, 0, 0, 0, 0, 1, 1, 0.0f, 0) == SMT_ERR_ARG && c[4] == 0.0f && c[12] == 1.0f'
                   ' && SMT_FILLHOLES_UB_NAN == 1 && SMT_FILLHOLES_MAX_DIM == 8192 ? 0 : 1; }\n')
    lib_dir = os.path.join(ROOT, "stereo_match_traditional_amd", "lib")
    exe = tmp_path / "c99"
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L" + lib_dir, "-lsmt_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_names(L):
    from stereo_match_traditional_amd import _lib, api, shard
    assert callable(api.FillHolesInDispMap) and "FillHolesInDispMap" in api.__all__
    for n in ("FILLHOLES_UB_NAN", "FILLHOLES_MAX_DIM"):
        assert n in api.__all__ and getattr(api, n) == getattr(_lib, n), n
    assert (_lib.FILLHOLES_UB_NAN, _lib.FILLHOLES_MAX_DIM) == (FH.UB_NAN, FH.MAX_DIM)
    assert callable(api.Pipeline.run_filled) and callable(shard.pipeline_filled_batch)
    assert len(_lib.lib().smt_fill_holes_batch.argtypes) == 10 and len(_lib.lib().smt_pipeline_run_batch_filled.argtypes) == 12


def test_cpp_mirror_against_the_contract_stub_under_asan(tmp_path):
    """host/smt_fill_holes.hpp and a main of its own against a host-only stub of the entries it calls, with exact-size
    heap buffers, as its own process"""
    cxx = os.environ.get("CXX", "g++")
    exe = tmp_path / "fill_holes_mirror"
    cmd = [cxx] + FLAGS + [os.path.join(MIRROR, "fill_holes_stub.cpp"), os.path.join(MIRROR, "fill_holes_mirror_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr         # -Wall -Wextra -Werror clean
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fill_holes: contract held" in r.stdout
