"""MedianFilter with in == out (CBLSM.cpp:162) and the CBLSM.cpp tail: what can be checked without a GPU -- the host twin
of the kernels' schedule (csrc/median_schedule.h) against the oracle in place, the band seams, the discrimination
condition, the defaults and the argument checks (they return before any device work)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import median_inplace_cases as MC  # noqa: E402

SMT_OK, SMT_ERR_ARG = 0, -1
HS = (1, 2, 3, 5, 9, 33)
WS = (1, 2, 3, 4, 5, 17, 40, 130)
WNDS = (1, 3, 5, 7, 2, 4, 6)


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd import build
    L = C.CDLL(build.build())
    L.smt_median_filter_inplace_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int]
    L.smt_median_filter_inplace_host_ex.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_int, C.c_int]
    L.smt_median_filter_inplace_batch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smt_median_filter_inplace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smt_median_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.smt_cblsm_tail_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def host(lib, m, wnd, impl=None, band=0, reverse=0, stride=0):
    """the host twin on a copy of [H][W] or of a flat buffer holding `pairs` maps `stride` apart"""
    a = np.ascontiguousarray(m, np.float32).copy()
    H, W = a.shape[-2:]
    pairs = 1 if a.ndim == 2 else a.shape[0]
    p = a.ctypes.data_as(C.c_void_p)
    if impl is None:
        rc = lib.smt_median_filter_inplace_host(p, pairs, stride, W, H, wnd)
    else:
        rc = lib.smt_median_filter_inplace_host_ex(p, pairs, stride, W, H, wnd, impl, band, reverse)
    assert rc == SMT_OK, rc
    return a


@pytest.mark.parametrize("wnd", WNDS)
def test_host_twin_equals_the_oracle_in_place(lib, wnd):
    """Test 1 and 3 of the issue: every H x W of the grid, both formulations and both thread orders of the ring form;
    where the discrimination condition applies it is asserted on the oracle's result."""
    for H in HS:
        for W in WS:
            m = MC.rand_map(H, W, 1000 * H + W)
            want = MC.oracle_inplace(m, wnd)
            if wnd == 1:
                assert MC.same_bits(want, m)
            for impl, rev in ((0, 0), (0, 1), (1, 0)):
                got = host(lib, m, wnd, impl, 0, rev)
                assert MC.same_bits(got, want), (H, W, wnd, impl, rev)
            assert MC.same_bits(host(lib, m, wnd), want)
            if MC.discriminates(m, wnd):
                MC.check_discrimination(m, wnd, want)


@pytest.mark.parametrize("wnd", (3, 5, 7, 4))
def test_host_twin_on_constant_and_all_inf_maps(lib, wnd):
    for H, W in ((5, 5), (9, 17), (33, 40), (1, 4), (3, 1)):
        for m in (np.full((H, W), np.inf, np.float32), np.full((H, W), 7.0, np.float32)):
            want = MC.oracle_inplace(m, wnd)
            for impl in (0, 1):
                assert MC.same_bits(host(lib, m, wnd, impl), want), (H, W, wnd, impl)


@pytest.mark.parametrize("pairs", (1, 3))
def test_host_twin_batches_and_leaves_the_stride_gap_untouched(lib, pairs):
    H, W, gap = 9, 17, 11
    stride = H * W + gap
    for wnd in (3, 5, 6):
        maps = MC.rand_map(H, W, 77 + wnd, pairs)
        for impl in (0, 1):
            buf = np.full(pairs * stride, -123.0, np.float32)
            for b in range(pairs):
                buf[b * stride:b * stride + H * W] = maps[b].ravel()
            rc = lib.smt_median_filter_inplace_host_ex(buf.ctypes.data_as(C.c_void_p), pairs, stride, W, H, wnd, impl, 0, 0)
            assert rc == SMT_OK
            for b in range(pairs):
                got = buf[b * stride:b * stride + H * W].reshape(H, W)
                assert MC.same_bits(got, MC.oracle_inplace(maps[b], wnd)), (pairs, wnd, impl, b)
                assert np.all(buf[b * stride + H * W:(b + 1) * stride] == -123.0)


@pytest.mark.parametrize("shape", ((13, 17), (33, 40)))
def test_band_seams(lib, shape):
    """Test 2: band heights 1, 2, r, r + 1, 5 and H; the rows above a band come from global memory (final), the rows
    below it too (untouched)."""
    H, W = shape
    m = MC.rand_map(H, W, 5)
    for wnd in (3, 5, 7):
        r = wnd // 2
        want = MC.oracle_inplace(m, wnd)
        for band in sorted({1, 2, r, r + 1, 5, H}):
            for impl, rev in ((0, 0), (0, 1), (1, 0)):
                assert MC.same_bits(host(lib, m, wnd, impl, band, rev), want), (shape, wnd, band, impl, rev)


def test_band_seam_at_the_real_band_height(lib):
    """H = 1025: the plain form runs 1024 + 1 rows, the ring form 1022 + 3 (506 + 506 + 13 at window 7)."""
    m = MC.rand_map(1025, 5, 9)
    for wnd in (3, 7):
        want = MC.oracle_inplace(m, wnd)
        for impl in (0, 1):
            assert MC.same_bits(host(lib, m, wnd, impl), want), (wnd, impl)
    assert lib.smt_median_filter_inplace_host_ex(C.c_void_p(4096), 1, 0, 5, 1025, 3, 0, 1023, 0) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace_host_ex(C.c_void_p(4096), 1, 0, 5, 1025, 3, 1, 1025, 0) == SMT_ERR_ARG


def test_cblsm_post_defaults_are_cblsm_cpp_155_161_162(lib):
    from stereo_match_traditional_amd._lib import CBLSMPostParams
    p = CBLSMPostParams(7, 7, 7, 7, 7)
    lib.smt_cblsm_post_default_params(C.byref(p))
    assert (p.gate, p.speckle_diff, p.speckle_min_area, p.speckle_invalid, p.median_wnd) == (5, 1, 50, -(2 ** 31), 3)
    lib.smt_cblsm_post_default_params(None)


def test_out_of_place_median_still_rejects_aliased_buffers(lib):
    a = C.c_void_p(4096)
    assert lib.smt_median_filter(a, a, 8, 8, 3, None) == SMT_ERR_ARG


def test_inplace_entries_reject_arguments_without_a_gpu(lib):
    a = C.c_void_p(4096)                                    # never dereferenced: the checks come first
    for f in (lambda d, P, s, W, H, w: lib.smt_median_filter_inplace_batch(d, P, s, W, H, w, None),
              lambda d, P, s, W, H, w: lib.smt_median_filter_inplace_host(d, P, s, W, H, w),
              lambda d, P, s, W, H, w: lib.smt_median_filter_inplace_host_ex(d, P, s, W, H, w, 0, 0, 0)):
        assert f(None, 1, 0, 8, 8, 3) == SMT_ERR_ARG
        for pairs in (0, -1):
            assert f(a, pairs, 0, 8, 8, 3) == SMT_ERR_ARG
        for W, H in ((0, 8), (8, 0), (-1, 8), (8, -2)):
            assert f(a, 1, 0, W, H, 3) == SMT_ERR_ARG
        assert f(a, 1, 0, 32768, 65536, 3) == SMT_ERR_ARG   # H*W = 2^31
        for wnd in (0, 8, -1):
            assert f(a, 1, 0, 8, 8, wnd) == SMT_ERR_ARG
        for stride in (1, 63):
            assert f(a, 2, stride, 8, 8, 3) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace(None, 8, 8, 3, None) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace(a, 0, 8, 3, None) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace(a, 8, 8, 9, None) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace_host_ex(a, 1, 0, 8, 8, 3, 2, 0, 0) == SMT_ERR_ARG
    assert lib.smt_median_filter_inplace_host_ex(a, 1, 0, 8, 8, 3, 0, -1, 0) == SMT_ERR_ARG
    assert lib.smt_median_inplace_set_impl(2) == SMT_ERR_ARG and lib.smt_median_inplace_set_impl(-1) == SMT_ERR_ARG
    assert lib.smt_median_inplace_set_impl(0) == SMT_OK


def test_tail_and_post_entries_reject_arguments_without_a_gpu(lib):
    from stereo_match_traditional_amd._lib import CBLSMPostParams
    a, b, c = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    f = lib.smt_cblsm_tail_batch
    ok = dict(dL=a, dR=b, pairs=2, stride=0, H=8, W=8, post=None, cls=c)

    def call(**kw):
        k = dict(ok, **kw)
        return f(k["dL"], k["dR"], k["pairs"], k["stride"], k["H"], k["W"], k["post"], k["cls"], None, None, None)

    assert call(dL=None) == SMT_ERR_ARG and call(dR=None) == SMT_ERR_ARG and call(cls=None) == SMT_ERR_ARG
    assert call(pairs=-1) == SMT_ERR_ARG
    assert call(pairs=0) == SMT_OK                          # a no-op, as in the flows
    for H, W in ((0, 8), (8, 0), (-1, 8)):
        assert call(H=H, W=W) == SMT_ERR_ARG
    assert call(H=65536, W=32768) == SMT_ERR_ARG
    assert call(stride=63) == SMT_ERR_ARG
    for wnd in (0, 8):
        p = CBLSMPostParams()
        lib.smt_cblsm_post_default_params(C.byref(p))
        p.median_wnd = wnd
        assert call(post=C.addressof(p)) == SMT_ERR_ARG
    g = lib.smt_cblsm_flow_run_batch_post
    g.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5
    assert g(None, a, a, 1, a, b, c, None, None) == SMT_ERR_ARG
    h = lib.smt_crossagg_flow_run_batch_post
    h.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    assert h(None, a, a, None, None, 1, a, b, c, None, None) == SMT_ERR_ARG
    assert lib.smt_crossagg_flow_status(None) == SMT_ERR_ARG
