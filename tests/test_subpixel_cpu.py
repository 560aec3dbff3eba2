"""Sub-pixel disparities where there is no device: the host twin smt_wta_subpixel_host (the same rule header the kernels
include) against the NumPy restatement on the whole case table, bit for bit; properties of the rule; argument errors;
exports.  tests/subpixel_cases.py holds the restatement and the table."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import subpixel_cases as SP  # noqa: E402
import bounds_cases as BC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMT_ERR_ARG = -1
NEW = ("smt_subpixel_default_params", "smt_wta_subpixel", "smt_wta_subpixel_host", "smt_scanline_set_subpixel",
       "smt_crossarm_set_subpixel", "smt_pipeline_set_subpixel")


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd import _lib
    _lib.lib()
    return _lib


def host(L, vol, min_den=None):
    vol = np.ascontiguousarray(vol, np.float32)
    H, W, D = vol.shape
    disp = np.full((H, W), np.nan, np.float32)
    p = None if min_den is None else C.byref(L.SubpixelParams(min_den))
    rc = L.lib().smt_wta_subpixel_host(vol.ctypes.data_as(C.c_void_p), H, W, D, p, disp.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return disp


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("D,min_den,shape", SP.TABLE, ids=[f"D{d}-m{m:g}-{s[0]}x{s[1]}" for d, m, s in SP.TABLE])
def test_host_twin_equals_the_restatement(L, O, D, min_den, shape):
    vol = SP.volume(D, shape)
    got, ref = host(L, vol, min_den), SP.restate(O, vol, min_den)
    assert np.array_equal(bits(got), bits(ref)), np.argwhere(bits(got) != bits(ref))[:4]


def test_null_params_are_the_defaults(L, O):
    p = L.SubpixelParams(0.0)
    L.lib().smt_subpixel_default_params(C.byref(p))
    assert p.min_den == 1.0                                           # Sad.h:80
    vol = SP.volume(65, (5, 7))
    assert np.array_equal(bits(host(L, vol, None)), bits(SP.restate(O, vol, 1.0)))


def test_the_table_holds_what_it_says(O):
    """every construction is present at every D, the planted winners win, and the maps hold fractions"""
    for D in SP.DS:
        names = [n for n, _ in SP.special_rows(D)]
        assert len(set(names)) == len(names) and {"tie-next", "all-nan", "inf-both", "negzero-then-zero", "sad-scale"} <= set(names)
        vol = SP.volume(D, SP.SHAPES[-1])
        w = O.wta(vol).reshape(-1)
        for k, (name, _) in enumerate(SP.special_rows(D)):
            if name.startswith("planted-") and name != "planted-mid":
                assert w[k] == int(name.split("-")[1]), (D, name, w[k])
        if D >= 3:
            for m in SP.MIN_DENS:
                r = SP.restate(O, vol, m)
                assert (r != np.floor(r)).sum() > 100, (D, m)


@pytest.mark.parametrize("min_den", SP.MIN_DENS)
def test_the_result_stays_within_half_a_step_of_the_winner(L, O, min_den):
    """On the NaN-free rows |result - w| <= 0.5 + 2^-22: c[w-1] > c[w] <= c[w+1], so |c1 - c2| <= s in exact arithmetic;
    the table's rows keep s >= 1/4 of the magnitude of c1 + c2 wherever den = s is not clamped away (planted minima of
    0.25 under costs >= 0.5, integer-valued costs), so the three roundings move the quotient by less than 2^-22.  And
    the offset never has the sign opposite to c1 - c2."""
    for D in SP.DS:
        vol = SP.volume(D, SP.SHAPES[-1])
        ok = SP.nan_free(vol)
        w = O.wta(vol)
        r = host(L, vol, min_den)
        assert (np.abs(r.astype(np.float64) - w)[ok] <= 0.5 + 2.0 ** -22).all(), D
        if D >= 3:
            inner = ok & (w > 0) & (w < D - 1)
            wi = np.clip(w.astype(np.int64), 1, D - 2)
            c1 = np.take_along_axis(vol, (wi - 1)[..., None], 2)[..., 0].astype(np.float64)
            c2 = np.take_along_axis(vol, (wi + 1)[..., None], 2)[..., 0].astype(np.float64)
            with np.errstate(invalid="ignore"):
                sgn = np.sign(c1 - c2)
            d = np.sign(r.astype(np.float64) - w)
            assert ((d == 0) | (d == sgn))[inner].all(), D
            big = inner & np.isfinite(c1) & np.isfinite(c2) & (np.abs(r - w) >= 2.0 ** -10)
            assert big.sum() > 50 and (d == sgn)[big].all(), D


def test_an_exact_parabola_gives_its_vertex(L):
    """c[d] = a (d - x0)^2 + b on dyadic a, x0, b: every step of the rule is exact, den = 2 a is above min_den = 2^-20,
    and the result is x0"""
    rows, want = [], []
    for D in (3, 60, 65, 257):
        for a in (0.25, 1.0, 8.0):
            for b in (0.0, -16.0, 5.5):
                for w in sorted({1, D // 2, D - 2}):
                    for f in (-0.375, -0.125, 0.0, 0.25, 0.4375):
                        x0 = w + f
                        c = a * (np.arange(D, dtype=np.float64) - x0) ** 2 + b
                        assert np.array_equal(c, c.astype(np.float32).astype(np.float64))
                        rows.append((D, c.astype(np.float32))); want.append(x0)
    for (D, c), x0 in zip(rows, want):
        got = host(L, c.reshape(1, 1, D), 2.0 ** -20)
        assert float(got[0, 0]) == x0, (D, x0, float(got[0, 0]))


def test_argument_errors(L):
    l = L.lib()
    v = np.zeros(4 * 4 * 8, np.float32)
    d = np.zeros(16, np.float32)
    vp, dp = v.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    ok = L.SubpixelParams(1.0)
    for fn, tail in ((l.smt_wta_subpixel_host, ()), (l.smt_wta_subpixel, (None,))):       # both reject before any HIP call
        for H, W, D in ((0, 4, 8), (4, 0, 8), (4, 4, 0), (-1, 4, 8), (4, -3, 8), (4, 4, -8), (1, 1, 513)):
            assert fn(vp, H, W, D, C.byref(ok), dp, *tail) == SMT_ERR_ARG, (H, W, D)
        assert fn(None, 4, 4, 8, C.byref(ok), dp, *tail) == SMT_ERR_ARG
        assert fn(vp, 4, 4, 8, C.byref(ok), None, *tail) == SMT_ERR_ARG
        for m in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert fn(vp, 4, 4, 8, C.byref(L.SubpixelParams(m)), dp, *tail) == SMT_ERR_ARG, m
    assert l.smt_wta_subpixel_host(vp, 4, 4, 8, C.byref(ok), dp) == 0
    for setter in (l.smt_scanline_set_subpixel, l.smt_crossarm_set_subpixel, l.smt_pipeline_set_subpixel):
        assert setter(None, C.byref(ok)) == SMT_ERR_ARG and setter(None, None) == SMT_ERR_ARG


def test_new_symbols_are_declared_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    assert 'extern "C"' in hdr or "__cplusplus" in hdr
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, plain), name
        assert hasattr(L.lib(), name), name
    assert re.search(r"typedef struct smt_subpixel_params \{ float min_den; \} smt_subpixel_params;", plain)
    assert "//" not in plain.replace("://", ""), "the header stays plain C: no // comments"


def test_the_new_declarations_have_their_decisions():
    """registered on import of tests/subpixel_cases.py: a reason for every new declaration, none of them in the table"""
    assert set(NEW) <= set(BC.NOT_CALLER_BUFFER) and not set(NEW) & set(BC.ENTRIES)


@pytest.mark.parametrize("params", SP.BOUNDS, ids=BC.case_id)
def test_host_twin_in_the_arena(O, params):
    """guards, both prefill seeds, inputs untouched, the restatement: the bounds suite's rules on host memory"""
    SP.run_case(BC.Ctx(O, None), True, params)
