"""Region voting and outlier interpolation where there is no device: the host twins smt_region_vote_batch_host,
smt_interpolate_outliers_batch_host and smt_refine_batch_host (plain loops through the rule header the kernels include)
against the NumPy restatement of tests/refine_cases.py, bit for bit on maps, state and status: the whole case table, the
crafted cases of the rule's sentences, arm maps at their limits and the reference's scrambled right arms; several maps,
strides and guards; argument errors; exports, the C99 header, the Python names; the C++ mirror against a contract stub
under AddressSanitizer."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import refine_cases as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smt_refine.h")
MIRROR = os.path.join(ROOT, "tests", "cpp_mirror_refine")
SMT_ERR_ARG = -1
NEW = ("smt_refine_default_params", "smt_region_vote_batch", "smt_interpolate_outliers_batch", "smt_refine_batch",
       "smt_region_vote_batch_host", "smt_interpolate_outliers_batch_host", "smt_refine_batch_host", "smt_refine_set_impl",
       "smt_refine_last_form", "smt_pipeline_run_batch_refined")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd import _lib
    _lib.lib()
    return _lib


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def cparams(L, p):
    return L.RefineParams(p["irv_ts"], p["irv_th"], p["irv_iters"], p["search"])


def host(L, which, M, arms, cls, gray, D, p):
    """a host twin on one map into prefilled outputs -> (map, state, status)"""
    H, W = M.shape
    m = np.ascontiguousarray(M, np.float32).copy()
    state = np.full((H, W), 0xEE, np.uint8)
    status = np.full(4, -77, np.int32)
    q = cparams(L, p)
    z = C.c_size_t(0)
    a = [np.ascontiguousarray(x, np.int32) for x in arms] if arms is not None else None
    c = np.ascontiguousarray(cls) if cls is not None else None
    g = np.ascontiguousarray(gray) if gray is not None else None
    tail = (H, W, D, C.byref(q), vp(state), z, vp(status))
    if which == "vote":
        rc = L.lib().smt_region_vote_batch_host(vp(m), 1, z, *[vp(x) for x in a], z, *tail)
    elif which == "interpolate":
        rc = L.lib().smt_interpolate_outliers_batch_host(vp(m), 1, z, vp(c), z, vp(g), z, *tail)
    else:
        rc = L.lib().smt_refine_batch_host(vp(m), 1, z, *[vp(x) for x in a], z, vp(c), z, vp(g), z, *tail)
    assert rc == 0, rc
    return m, state, status


def same(got, want, what):
    m, s, t = got
    rm, rs, rt = want
    assert np.array_equal(R.bits(m), R.bits(rm)), (what, "map", np.argwhere(R.bits(m) != R.bits(rm))[:4].tolist())
    assert np.array_equal(s, rs), (what, "state", np.argwhere(s != rs)[:4].tolist())
    assert list(t) == list(rt), (what, "status", list(t), list(rt))


@pytest.mark.parametrize("gid,H,W,D,seed", R.TABLE, ids=[t[0] for t in R.TABLE])
def test_host_twins_equal_the_restatement(L, gid, H, W, D, seed):
    M, arms, cls, gray = R.case(H, W, D, seed)
    for which in ("vote", "interpolate", "refine"):
        same(host(L, which, M, arms, cls, gray, D, R.TABLE_PARAMS), R.table_expected(H, W, D, seed, which), (gid, which))


def test_the_table_reaches_every_outcome():
    """over the table the restatement alone fills by voting, fills by interpolation and leaves outliers, at every
    iteration number it runs"""
    tot, states = np.zeros(4, np.int64), set()
    for gid, H, W, D, seed in R.TABLE:
        m, s, t = R.table_expected(H, W, D, seed, "vote")
        states |= set(np.unique(s).tolist())
        tot += R.table_expected(H, W, D, seed, "refine")[2]
        left = int((R.table_expected(H, W, D, seed, "refine")[1] == R.OUTLIER).sum())
        tot[3] += left
    assert tot[1] > 0 and tot[2] > 0 and tot[3] > 0, tot.tolist()
    assert {0, 1, 2, 3, 255} <= states, states


VOTE = R.crafted_vote()
INTERP = R.crafted_interp()


@pytest.mark.parametrize("name", sorted(VOTE))
def test_voting_crafted(L, name):
    M, arms, D, p, chk = VOTE[name]
    want = R.vote(M, arms, D, p)
    assert chk is None or chk(*want), (name, "the restatement itself", want[2].tolist())
    same(host(L, "vote", M, arms, None, None, D, p), want, name)


@pytest.mark.parametrize("name", sorted(INTERP))
def test_interpolation_crafted(L, name):
    M, cls, gray, D, p, chk = INTERP[name]
    want = R.interpolate(M, cls, gray, D, p)
    assert chk is None or chk(*want), (name, "the restatement itself", want[2].tolist())
    same(host(L, "interpolate", M, None, cls, gray, D, p), want, name)


def test_in_place_updating_would_fill_the_chain_at_once():
    """the chain case tells Jacobi from Gauss-Seidel: one sweep in raster order over a map updated in place fills all six"""
    M, arms, D, p, _ = VOTE["a-chain-fills-one-pixel-per-iteration"]
    m = M.copy()
    for j in range(1, 7):
        one = m.copy()
        out, filled = R.vote_once(one, R.clamp_arms(arms)[0], D, p["irv_ts"], p["irv_th"])
        m[0, j] = out[0, j]
    assert (m == 2.0).all()
    assert (R.vote(M, arms, D, R.params(irv_ts=0, irv_iters=1))[0][0, 2:] == R.INT_MIN_F).all()


def test_the_reference_arms_scrambled_at_w_above_h(L):
    """the faithful right arms of CrossArm.cpp (the _row stride, W > H) are read as they are: lengths that point past the
    border are clipped by the region's own bounds"""
    from oracle import oracle as orc
    H, W, D = 17, 65, 64
    M, _, cls, gray = R.case(H, W, D, 4)
    img, _ = orc.synth_pair(H, W, D, 3)
    arms = orc.arms_all(img)
    fixed = orc.arms_all(img, right_row_bug=False)
    assert not np.array_equal(arms[1], fixed[1]), "the right arms are not scrambled here: the case shows nothing"
    for p in (R.params(), R.params(irv_ts=2, irv_th=0.2)):
        same(host(L, "refine", M, arms, cls, gray, D, p), R.refine(M, arms, cls, gray, D, p), p)


def test_three_maps_strides_and_guards_on_the_host(L):
    """three different maps in one call equal three single calls; every output between guards under both prefills, the
    strides in elements, the inputs untouched"""
    H, W, D = 9, 33, 192
    cases = [R.case(H, W, D, s) for s in (3, 12, 13)]
    N = H * W
    p = R.TABLE_PARAMS

    def make(A):
        A.inout("maps", np.stack([c[0] for c in cases]), stride=N + 5)
        for k, n in enumerate("LRTB"):
            A.inp("a" + n, np.stack([c[1][k] for c in cases]), stride=N + 3)
        A.inp("cls", np.stack([c[2] for c in cases]), stride=N + 7)
        A.inp("gray", np.stack([c[3] for c in cases]), stride=N + 1)
        A.out("state", (3, H, W), np.uint8, stride=N + 9)
        A.out("status", (3, 4), np.int32)
        q = cparams(L, p)
        z = C.c_size_t
        return lambda A: L.lib().smt_refine_batch_host(A.ptr("maps"), 3, z(N + 5), A.ptr("aL"), A.ptr("aR"), A.ptr("aT"), A.ptr("aB"),
                                                       z(N + 3), A.ptr("cls"), z(N + 7), A.ptr("gray"), z(N + 1), H, W, D, C.byref(q),
                                                       A.ptr("state"), z(N + 9), A.ptr("status"))
    out, _ = arena.run_two_seeds(make)
    for k, c in enumerate(cases):
        same((out["maps"][k], out["state"][k], out["status"][k]), R.refine(*c, D, p), k)


def test_argument_errors(L):
    l = L.lib()
    H, W, D = 4, 5, 16
    N = H * W
    m = np.zeros((2, H, W), np.float32)
    a = np.zeros((2, H, W), np.int32)
    u = np.zeros((2, H, W), np.uint8)
    st = np.zeros((2, 4), np.int32)
    z = C.c_size_t
    bad = [dict(maps=None), dict(aR=None), dict(aT=None), dict(cls=None), dict(gray=None), dict(pairs=-1), dict(H=0), dict(W=-2),
           dict(D=0), dict(D=513), dict(iters=-1), dict(iters=17), dict(search=-1), dict(ms=N - 1), dict(as_=N - 1), dict(cs=1),
           dict(gs=N - 1), dict(ss=N - 1)]
    for kw in bad:
        k = dict(maps=vp(m), pairs=2, ms=N, aL=vp(a), aR=vp(a), aT=vp(a), aB=vp(a), as_=0, cls=vp(u), cs=0, gray=vp(u), gs=0, H=H, W=W,
                 D=D, iters=5, search=0, state=vp(u.copy()), ss=0, status=vp(st))
        k.update(kw)
        q = L.RefineParams(20, 0.4, k["iters"], k["search"])
        args = (k["maps"], k["pairs"], z(k["ms"]), k["aL"], k["aR"], k["aT"], k["aB"], z(k["as_"]), k["cls"], z(k["cs"]), k["gray"],
                z(k["gs"]), k["H"], k["W"], k["D"], C.byref(q), k["state"], z(k["ss"]), k["status"])
        assert l.smt_refine_batch_host(*args) == SMT_ERR_ARG, kw
        assert l.smt_refine_batch(*args, None) == SMT_ERR_ARG, kw                  # rejected before any HIP call
        vote = args[:8] + args[12:]
        interp = args[:3] + args[8:]
        if not ({"cls", "gray", "cs", "gs"} & set(kw)):
            assert l.smt_region_vote_batch_host(*vote) == SMT_ERR_ARG and l.smt_region_vote_batch(*vote, None) == SMT_ERR_ARG, kw
        if not ({"aR", "aT", "as_"} & set(kw)):
            assert l.smt_interpolate_outliers_batch_host(*interp) == SMT_ERR_ARG, kw
            assert l.smt_interpolate_outliers_batch(*interp, None) == SMT_ERR_ARG, kw
    q = L.RefineParams(20, 0.4, 5, 0)
    ok = (vp(m), 2, z(0), vp(a), vp(a), vp(a), vp(a), z(0), vp(u), z(0), vp(u), z(0), H, W, D)
    assert l.smt_refine_batch_host(*ok, None, None, z(0), None) == 0              # the defaults, no state, no status
    assert l.smt_refine_batch_host(vp(m), 0, *ok[2:], C.byref(q), None, z(0), None) == 0     # no maps: nothing to do
    assert l.smt_refine_batch(vp(m), 0, *ok[2:], C.byref(q), None, z(0), None, None) == 0
    assert l.smt_pipeline_run_batch_refined(None, None, None, 1, *([None] * 9)) == SMT_ERR_ARG      # no handle
    d = L.RefineParams()
    l.smt_refine_default_params(C.byref(d))
    assert (d.irv_ts, d.irv_iters, d.search) == (20, 5, 0) and d.irv_th == np.float32(0.4)
    l.smt_refine_default_params(None)
    for impl in (3, -1, 7):
        assert l.smt_refine_set_impl(impl) == SMT_ERR_ARG, impl
    for impl in (1, 2, 0):
        assert l.smt_refine_set_impl(impl) == 0, impl


def test_the_header_declares_what_the_library_exports_and_is_c99(L, tmp_path):
    hdr = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(smt_\w+)\s*\(", plain))
    assert declared == set(NEW), declared ^ set(NEW)
    for name in NEW:
        assert hasattr(L.lib(), name), name
    assert "//" not in plain, "the header stays plain C: no // comments"
    assert '#include "smt.h"' in plain and "__cplusplus" in plain
    assert "arity unpinned: no reference code" in hdr
    smt_h = open(os.path.join(ROOT, "include", "smt.h")).read()
    assert not any(n in smt_h for n in NEW) and "smt_refine" not in smt_h
    src = tmp_path / "c99.c"
    src.write_text('#include "smt_refine.h"\nint main(void) { smt_refine_params p; smt_refine_default_params(&p);\n'
                   ' return smt_refine_batch_host(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &p, 0, 0, 0) == SMT_ERR_ARG'
                   ' && p.irv_ts == 20 && p.irv_iters == 5 && SMT_REFINE_STATE_OUTLIER == 255 ? 0 : 1; }\n')
    lib_dir = os.path.join(ROOT, "stereo_match_traditional_amd", "lib")
    exe = tmp_path / "c99"
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L" + lib_dir, "-lsmt_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_names(L):
    from stereo_match_traditional_amd import _lib, api, shard
    for n in ("RegionVote", "InterpolateOutliers", "Refine", "refine_params", "refine_set_impl", "refine_last_form"):
        assert callable(getattr(api, n)) and n in api.__all__, n
    for n in ("REFINE_ARM_CLAMPED", "REFINE_STATE_INTERPOLATED", "REFINE_STATE_OUTLIER", "REFINE_FORM_DIRECT", "REFINE_FORM_WAVE"):
        assert n in api.__all__ and getattr(api, n) == getattr(_lib, n), n
    assert (_lib.REFINE_ARM_CLAMPED, _lib.REFINE_STATE_INTERPOLATED, _lib.REFINE_STATE_OUTLIER) == (R.ARM_CLAMPED, R.INTERPOLATED, R.OUTLIER)
    assert (_lib.REFINE_FORM_DIRECT, _lib.REFINE_FORM_WAVE) == (R.DIRECT, R.WAVE)
    assert callable(api.Pipeline.run_refined) and callable(shard.pipeline_refined_batch)
    p = api.refine_params()
    assert (p.irv_ts, p.irv_iters, p.search) == (20, 5, 0) and p.irv_th == np.float32(0.4)
    o = api.ADCensusOption(irv_ts=11, irv_th=0.25)
    p = api.refine_params(o, irv_iters=2)
    assert (p.irv_ts, p.irv_th, p.irv_iters, p.search) == (11, 0.25, 2, 0)
    p = api.refine_params(api.ADCensusOption())                                   # adcensus_types.h:72
    assert p.irv_ts == 20 and p.irv_th == np.float32(0.4)
    with pytest.raises(AttributeError):
        api.refine_params(irv_tz=1)
    assert len(_lib.lib().smt_refine_batch.argtypes) == 20 and len(_lib.lib().smt_pipeline_run_batch_refined.argtypes) == 13


def test_cpp_mirror_against_the_contract_stub_under_asan(tmp_path):
    """host/smt_refine.hpp and a main of its own against a host-only stub of the entries it calls, with exact-size heap
    buffers, as its own process"""
    cxx = os.environ.get("CXX", "g++")
    exe = tmp_path / "refine_mirror"
    cmd = [cxx] + FLAGS + [os.path.join(MIRROR, "refine_stub.cpp"), os.path.join(MIRROR, "refine_mirror_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr         # -Wall -Wextra -Werror clean
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine: contract held" in r.stdout
