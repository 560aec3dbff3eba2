"""Batched post-filters (smt_remove_speckles_batch, smt_median_filter_batch, smt_pipeline_run_batch_post): what can be
checked without a GPU -- the main.cpp:93-94 defaults, the argument checks (they return before any device work) and the
host-side check of the border-merge kernel's thread mapping."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SMT_OK, SMT_ERR_ARG, SMT_ERR_STATE = 0, -1, -6


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd import build
    L = C.CDLL(build.build())
    L.smt_remove_speckles_batch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int,
                                            C.c_void_p, C.c_void_p]
    L.smt_median_filter_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p]
    return L


def test_post_default_params_are_main_cpp_93_94(lib):
    from stereo_match_traditional_amd._lib import PostParams
    p = PostParams(7, 7, 7, 7)
    lib.smt_post_default_params(C.byref(p))
    assert (p.speckle_diff, p.speckle_min_area, p.speckle_invalid, p.median_wnd) == (1, 30, -(2 ** 31), 3)
    lib.smt_post_default_params(None)                      # tolerated, like smt_pipeline_default_params


def test_remove_speckles_batch_rejects_arguments_without_a_gpu(lib):
    f = lib.smt_remove_speckles_batch
    fake = C.c_void_p(4096)                                # never dereferenced: the checks come first
    ok = dict(disp=fake, pairs=2, stride=0, W=64, H=48)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["disp"], a["pairs"], a["stride"], a["W"], a["H"], 1, 30, -(2 ** 31), None, None)

    assert call(disp=None) == SMT_ERR_ARG
    for pairs in (0, -1):
        assert call(pairs=pairs) == SMT_ERR_ARG
    for W, H in ((0, 48), (64, 0), (-3, 48), (64, -1)):
        assert call(W=W, H=H) == SMT_ERR_ARG
    assert call(W=32768, H=65536) == SMT_ERR_ARG           # H*W = 2^31
    assert call(W=65536, H=65536) == SMT_ERR_ARG
    for stride in (1, 64 * 48 - 1):
        assert call(stride=stride) == SMT_ERR_ARG


def test_median_filter_batch_rejects_arguments_without_a_gpu(lib):
    f = lib.smt_median_filter_batch
    a, b = C.c_void_p(4096), C.c_void_p(1 << 20)
    assert f(None, b, 1, 0, 8, 8, 3, None) == SMT_ERR_ARG
    assert f(a, None, 1, 0, 8, 8, 3, None) == SMT_ERR_ARG
    assert f(a, a, 1, 0, 8, 8, 3, None) == SMT_ERR_ARG
    assert f(a, b, 0, 0, 8, 8, 3, None) == SMT_ERR_ARG
    assert f(a, b, 1, 0, 0, 8, 3, None) == SMT_ERR_ARG
    assert f(a, b, 1, 0, 8, 0, 3, None) == SMT_ERR_ARG
    for wnd in (0, 8, -1):
        assert f(a, b, 1, 0, 8, 8, wnd, None) == SMT_ERR_ARG
    assert f(a, b, 2, 63, 8, 8, 3, None) == SMT_ERR_ARG
    assert f(a, b, 1, 0, 32768, 65536, 3, None) == SMT_ERR_ARG


def test_pipeline_run_batch_post_rejects_a_null_handle(lib):
    from stereo_match_traditional_amd._lib import PostParams
    p = PostParams()
    lib.smt_post_default_params(C.byref(p))
    f = lib.smt_pipeline_run_batch_post
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p]
    x = C.c_void_p(4096)
    assert f(None, x, x, 1, x, x, x, None, C.addressof(p), None) == SMT_ERR_ARG


def test_speckle_border_merge_examines_every_cross_tile_pair_once(lib):
    """smt_speckle_selftest_tiles: over tile multiples, partial tiles, one-pixel rows / columns and the 1080p map,
    every 8-adjacent pair whose pixels lie in two tiles (diagonal pairs across a tile corner included) is examined by
    exactly one border-merge thread and no thread examines a pair inside one tile."""
    f = lib.smt_speckle_selftest_tiles
    shapes = [(1, 1), (1, 1000), (1000, 1), (7, 1000), (32, 32), (33, 33), (31, 65), (64, 64), (65, 97), (2, 33),
              (33, 2), (1080, 1920), (540, 960), (100, 1), (1, 33)]
    for H, W in shapes:
        assert f(H, W) == SMT_OK, (H, W)
    for H in range(1, 70, 3):
        for W in (1, 2, 31, 32, 33, 63, 64, 65, 95):
            assert f(H, W) == SMT_OK, (H, W)
    assert f(0, 5) == SMT_ERR_ARG and f(5, 0) == SMT_ERR_ARG and f(1 << 14, 1 << 14) == SMT_ERR_ARG
