"""The bilateral image filter where there is no device: the host twin smt_bilateral_filter_host (direct loops through the
rule header the kernels include) against the NumPy restatement of tests/bilateral_cases.py on the whole table, on the
float64 sums and on the bytes, bit for bit, under both norms; the tables; the flat cases; the restatement against exact
rational arithmetic; argument errors; exports, the C99 header, the Python names; the C++ mirror against a contract stub
under AddressSanitizer."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bilateral_cases as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smt_bilateral.h")
MIRROR = os.path.join(ROOT, "tests", "cpp_mirror_bilateral")
SMT_ERR_ARG = -1
NEW = ("smt_bilateral_masks", "smt_bilateral_filter_batch", "smt_bilateral_filter_host", "smt_bilateral_set_impl",
       "smt_bilateral_last_form")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd import _lib
    _lib.lib()
    return _lib


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host(L, img, wsize, space, color, norm, want_acc=True, images=1):
    """the host twin into prefilled outputs -> (dst, acc)"""
    img = np.ascontiguousarray(img)
    shape = img.shape[1:] if images != 1 or img.ndim == 4 else img.shape
    H, W = shape[0], shape[1]
    ch = shape[2] if len(shape) == 3 else 1
    dst = np.full(img.shape, 0xEE, np.uint8)
    acc = np.full(img.shape, np.nan, np.float64) if want_acc else None
    sp, cm = np.ascontiguousarray(space), np.ascontiguousarray(color)
    rc = L.lib().smt_bilateral_filter_host(vp(img), images, H, W, ch, wsize[0], wsize[1], vp(sp), vp(cm), norm, vp(dst), vp(acc))
    assert rc == 0, rc
    return dst, acc


@pytest.mark.parametrize("gid,kind,H,W,ch", B.groups(), ids=[g[0] for g in B.groups()])
def test_host_twin_equals_the_restatement(L, gid, kind, H, W, ch):
    img = B.image(kind, H, W, ch)
    for wsize, ss, sc in B.windows_for((H, W)):
        space, color = B.tables(wsize, ss, sc)
        for norm in B.NORMS:
            dst, acc = host(L, img, wsize, space, color, norm)
            rdst, racc = B.restate(kind, H, W, ch, wsize, ss, sc, norm)
            assert np.array_equal(B.bits(acc), B.bits(racc)), (gid, wsize, norm, "acc", B.first_diff(acc, racc))
            assert np.array_equal(dst, rdst), (gid, wsize, norm, "bytes", B.first_diff(dst, rdst))
            only, none = host(L, img, wsize, space, color, norm, want_acc=False)
            assert none is None and np.array_equal(only, rdst), (gid, wsize, norm, "without acc")


def test_the_norms_differ_and_an_even_side_acts_as_the_odd_side_below(L):
    """the two forms of Mask / S give different sums on a good part of random pixels -- they are two rules, not one -- and
    the 4 x 6 window reads rows 0..2 and columns 0..4 of a table whose row stride is 6"""
    H, W, ch = 17, 65, 3
    a = B.restate("noise", H, W, ch, (23, 23), 10, 30, B.RECIPROCAL)[1]
    b = B.restate("noise", H, W, ch, (23, 23), 10, 30, B.DIVIDE)[1]
    differ = float((B.bits(a) != B.bits(b)).mean())
    print("sums that differ between the norms at 23 x 23 on noise:", differ)
    assert 0.02 < differ < 0.6, differ
    img = B.image("noise", 9, 33, 1)
    s46, color = B.tables((4, 6), 10, 30)
    s35 = np.ascontiguousarray(s46[:3, :5])
    for norm in B.NORMS:
        d46, a46 = host(L, img, (4, 6), s46, color, norm)
        d35, a35 = host(L, img, (3, 5), s35, color, norm)
        assert np.array_equal(B.bits(a46), B.bits(a35)) and np.array_equal(d46, d35), norm


def ulps(a, b):
    ia, ib = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def test_masks(L):
    """smt_bilateral_masks against math.exp within 1 ulp; for the reference's own parameters (TeddyBilateral.cpp:39-46:
    side 2 * 11 + 3, sigma 50 / 25) exactly smt_asw_masks' tables, where the shapes coincide"""
    for wsize, ss, sc in B.WINDOWS + B.WIDE + (((1, 5), 10, 30), ((64, 1), 0.75, 3.5)):
        h, w = wsize
        sp, cm = np.full((h, w), np.nan), np.full(256, np.nan)
        assert L.lib().smt_bilateral_masks(h, w, ss, sc, vp(sp), vp(cm)) == 0
        rs, rc = B.masks(wsize, ss, sc)
        assert ulps(sp, rs).max() <= 1 and ulps(cm, rc).max() <= 1, (wsize, int(ulps(sp, rs).max()), int(ulps(cm, rc).max()))
        assert sp[(h - 1) // 2, (w - 1) // 2] == 1.0 and cm[0] == 1.0
    sp, cm = np.empty((25, 25)), np.empty(256)
    asp, acm = np.empty((25, 25)), np.empty(256)
    assert L.lib().smt_bilateral_masks(25, 25, 50.0, 25.0, vp(sp), vp(cm)) == 0
    assert L.lib().smt_asw_masks(11, C.c_double(50.0), C.c_double(25.0), vp(asp), vp(acm)) == 0
    assert arena.same_bytes(sp, asp) and arena.same_bytes(cm, acm)
    for bad in ((0, 3), (3, 0), (65, 3), (3, 65), (-1, 1)):
        assert L.lib().smt_bilateral_masks(bad[0], bad[1], 10.0, 30.0, vp(sp), vp(cm)) == SMT_ERR_ARG, bad
    assert L.lib().smt_bilateral_masks(3, 3, 10.0, 30.0, None, vp(cm)) == SMT_ERR_ARG
    assert L.lib().smt_bilateral_masks(3, 3, 10.0, 30.0, vp(sp), None) == SMT_ERR_ARG


@pytest.mark.parametrize("value,wsize,want", B.FLAT, ids=[f"flat{v}-{w[0]}x{w[1]}" for v, w, _ in B.FLAT])
def test_flat_images_lose_a_grey_level_where_the_sums_say_so(L, value, wsize, want):
    """the table's own claim first -- the restatement's bytes are the listed ones under the default norm --, then the
    host twin under both norms on 1 and 3 channels"""
    space, color = B.tables(wsize, 10, 30)
    for ch in B.CHANNELS:
        rdst, racc = B.restate(("flat", value), *B.FLAT_SHAPE, ch, wsize, 10, 30, B.RECIPROCAL)
        assert (rdst == want).all(), (value, wsize, ch, np.unique(rdst).tolist())
        for norm in B.NORMS:
            rdst, racc = B.restate(("flat", value), *B.FLAT_SHAPE, ch, wsize, 10, 30, norm)
            dst, acc = host(L, B.image(("flat", value), *B.FLAT_SHAPE, ch), wsize, space, color, norm)
            assert np.array_equal(dst, rdst) and np.array_equal(B.bits(acc), B.bits(racc)), (value, wsize, ch, norm)
    if value == 1:      # one of the rare bytes on which the norms differ
        assert (B.restate(("flat", 1), *B.FLAT_SHAPE, 1, wsize, 10, 30, B.DIVIDE)[0] == 1).all()


EXACT = [("noise", 4, 5, 1, (5, 5), 10, 30), ("noise", 3, 4, 3, (23, 23), 10, 30), ("noise", 2, 3, 1, (63, 63), 10, 30),
         ("stairs", 3, 8, 1, (4, 6), 10, 30), ("noise", 3, 3, 3, (25, 25), 50, 25)]


@pytest.mark.parametrize("kind,H,W,ch,wsize,ss,sc", EXACT, ids=[f"{e[0]}-{e[1]}x{e[2]}x{e[3]}-{e[4][0]}x{e[4][1]}" for e in EXACT])
def test_the_restatement_against_exact_arithmetic(kind, H, W, ch, wsize, ss, sc):
    """The exact value of a sample is (sum of q_t wt_t) / (sum of wt_t) with wt_t = color[|q_t - centre|] space[t] the
    exact product of the two float64 table entries, evaluated in rational arithmetic (every float64 is an integer over
    2^1100, so the products and sums are integers and the quotient a fractions.Fraction).  Both norms must lie within
    (2 n + 6) 2^-53 of it, relative, n the number of taps: every computed weight carries one rounding (1); their sum
    carries n - 1; the reciprocal and the scaling of a weight by it carry at most three (1 / S, the product -- or the one
    division of the other norm --, and one to spare); the product with the sample carries one; the second sum n - 1.  All
    terms are non-negative, so the roundings compound without cancellation: 1 + (n - 1) + 3 + 1 + (n - 1) = 2 n + 3
    first-order terms of at most 2^-53 each, and the remaining 3 of 2 n + 6 cover the second-order terms for n <= 3 969
    ((1 + 2^-53)^(2 n + 3) - 1 < (2 n + 4) 2^-53).  The restatement, measured, reaches at most 0.11 of the bound."""
    img = B.image(kind, H, W, ch)
    space, color = B.tables(wsize, ss, sc)
    scale = 1 << 1100
    ci = [int(Fraction(float(c)) * scale) for c in color]
    si = [[int(Fraction(float(s)) * scale) for s in row] for row in space]
    assert all(Fraction(c, scale) == Fraction(float(color[k])) for k, c in enumerate(ci))
    a = img.reshape(H, W, -1).astype(int)
    hh, ww = (wsize[0] - 1) // 2, (wsize[1] - 1) // 2
    n = (2 * hh + 1) * (2 * ww + 1)
    bound = Fraction(2 * n + 6, 1 << 53)
    accs = [B.restate(kind, H, W, ch, wsize, ss, sc, norm)[1].reshape(H, W, -1) for norm in B.NORMS]
    worst = Fraction(0)
    for y in range(H):
        for x in range(W):
            for k in range(a.shape[2]):
                centre, num, den = int(a[y, x, k]), 0, 0
                for r in range(-hh, hh + 1):
                    yy = min(max(y + r, 0), H - 1)
                    for c in range(-ww, ww + 1):
                        q = int(a[yy, min(max(x + c, 0), W - 1), k])
                        wt = ci[abs(q - centre)] * si[r + hh][c + ww]
                        num += q * wt
                        den += wt
                exact = Fraction(num, den)
                for norm, acc in zip(B.NORMS, accs):
                    err = abs(Fraction(float(acc[y, x, k])) - exact)
                    assert err <= bound * exact, (y, x, k, norm, float(err / exact) if exact else None, float(bound))
                    if exact:
                        worst = max(worst, err / exact / bound)
    print(f"worst error / bound at {wsize[0]} x {wsize[1]}: {float(worst):.3f}")
    assert worst <= 1


def test_argument_errors(L):
    l = L.lib()
    img = np.zeros((2, 4, 5, 3), np.uint8)
    dst, acc = np.zeros_like(img), np.zeros(img.shape, np.float64)
    space, color = (np.ascontiguousarray(t) for t in B.tables((5, 5), 10, 30))
    s, d, a, sp, cm = vp(img), vp(dst), vp(acc), vp(space), vp(color)
    bad = [dict(ch=2), dict(ch=0), dict(ch=4), dict(H=0), dict(W=0), dict(H=-3), dict(images=-1), dict(wh=0), dict(ww=0), dict(wh=65),
           dict(ww=65), dict(wh=-5), dict(norm=2), dict(norm=-1), dict(src=None), dict(dst=None), dict(space=None), dict(color=None),
           dict(dst=s)]
    for kw in bad:
        p = dict(src=s, images=2, H=4, W=5, ch=3, wh=5, ww=5, space=sp, color=cm, norm=0, dst=d, acc=a)
        p.update(kw)
        args = (p["src"], p["images"], p["H"], p["W"], p["ch"], p["wh"], p["ww"], p["space"], p["color"], p["norm"], p["dst"], p["acc"])
        assert l.smt_bilateral_filter_host(*args) == SMT_ERR_ARG, kw
        assert l.smt_bilateral_filter_batch(*args, None) == SMT_ERR_ARG, kw        # rejected before any HIP call
    assert l.smt_bilateral_filter_host(s, 2, 4, 5, 3, 5, 5, sp, cm, 0, d, None) == 0
    assert l.smt_bilateral_filter_host(s, 0, 4, 5, 3, 5, 5, sp, cm, 0, d, a) == 0     # no images: nothing to do
    for impl in (3, -1, 7):
        assert l.smt_bilateral_set_impl(impl) == SMT_ERR_ARG, impl
    for impl in (1, 2, 0):
        assert l.smt_bilateral_set_impl(impl) == 0, impl


def test_several_images_and_guards_on_the_host(L):
    """three different images in one call equal three single calls; outputs between guards under both prefills, the
    inputs untouched"""
    imgs = np.stack([B.image("noise", 9, 33, 3), B.image("stairs", 9, 33, 3), B.image("noise", 9, 33, 3)[::-1].copy()])
    wsize = (7, 3)
    space, color = B.tables(wsize, 10, 30)
    for norm in B.NORMS:
        def make(A):
            A.inp("src", imgs); A.inp("space", space); A.inp("color", color)
            A.out("dst", imgs.shape, np.uint8); A.out("acc", imgs.shape, np.float64)
            return lambda A: L.lib().smt_bilateral_filter_host(A.ptr("src"), 3, 9, 33, 3, wsize[0], wsize[1], A.ptr("space"), A.ptr("color"),
                                                               norm, A.ptr("dst"), A.ptr("acc"))
        out, _ = arena.run_two_seeds(make)
        for k in range(3):
            rdst, racc = B.restate_with(imgs[k], wsize, space, color, norm)
            assert np.array_equal(out["dst"][k], rdst) and np.array_equal(B.bits(out["acc"][k]), B.bits(racc)), (norm, k)


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
    assert not any(n in smt_h for n in NEW)
    src = tmp_path / "c99.c"
    src.write_text('#include "smt_bilateral.h"\nint main(void) { return smt_bilateral_filter_host(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == SMT_ERR_ARG'
                   ' && SMT_BILATERAL_NORM_DIVIDE == 1 ? 0 : 1; }\n')
    lib_dir = os.path.join(ROOT, "stereo_match_traditional_amd", "lib")
    exe = tmp_path / "c99"
    r = subprocess.run([os.environ.get("CC", "gcc"), "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L" + lib_dir, "-lsmt_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_python_names():
    from stereo_match_traditional_amd import _lib, api, shard
    for n in ("bilateralfiter", "bilateral_masks", "bilateral_set_impl", "bilateral_last_form"):
        assert callable(getattr(api, n)) and n in api.__all__, n
    for n in ("BILATERAL_NORM_RECIPROCAL", "BILATERAL_NORM_DIVIDE", "BILATERAL_FORM_DIRECT", "BILATERAL_FORM_STAGED"):
        assert n in api.__all__ and getattr(api, n) == getattr(_lib, n), n
    assert (_lib.BILATERAL_NORM_RECIPROCAL, _lib.BILATERAL_NORM_DIVIDE) == (B.RECIPROCAL, B.DIVIDE)
    assert (_lib.BILATERAL_FORM_DIRECT, _lib.BILATERAL_FORM_STAGED) == (B.DIRECT, B.STAGED)
    assert callable(shard.bilateral_batch) and "not sharded" in shard.bilateral_batch.__doc__
    assert os.path.exists(os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "bilateral_main"))
    assert _lib.lib().smt_bilateral_filter_batch.argtypes is not None and len(_lib.lib().smt_bilateral_filter_batch.argtypes) == 13


def test_cpp_mirror_against_the_contract_stub_under_asan(tmp_path):
    """host/smt_bilateral.hpp and a main of its own against a host-only stub of the entries it calls, with exact-size
    heap buffers, as its own process"""
    cxx = os.environ.get("CXX", "g++")
    exe = tmp_path / "bilateral_mirror"
    cmd = [cxx] + FLAGS + [os.path.join(MIRROR, "bilateral_stub.cpp"), os.path.join(MIRROR, "bilateral_mirror_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr         # -Wall -Wextra -Werror clean
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bilateral: contract held" in r.stdout
