"""Host-side checks of the maps-only batch kernel (adcensus_kernels.h, adcensus_rules.h; no GPU): the rank table that replaces the float costs
in its WTA, and the workgroup arithmetic of its launch (K chunks per workgroup, table workgroups fused in)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd import build
    lib = ctypes.CDLL(build.build())
    lib.smt_adcensus_selftest_cost_rank.argtypes = [ctypes.c_float, ctypes.c_float]
    lib.smt_adcensus_selftest_maps_grid.argtypes = [ctypes.c_int] * 4
    return lib


@pytest.mark.parametrize("sc,ss", [(10.0, 30.0), (7.5, 12.25), (1e-3, 1e6), (1e6, 1e-3), (1e-3, 1e-3), (1e6, 1e6)])
def test_rank_table_preserves_cost_order(lib, sc, ss):
    """rank[64*ad + hd] orders the f32 sums lut[ad] + lut[256 + hd] exactly: equal ranks iff equal bits."""
    assert lib.smt_adcensus_selftest_cost_rank(sc, ss) == 0


def test_rank_table_rejects_bad_sigmas(lib):
    assert lib.smt_adcensus_selftest_cost_rank(0.0, 30.0) != 0
    assert lib.smt_adcensus_selftest_cost_rank(10.0, -1.0) != 0


def test_maps_grid_is_a_bijection(lib):
    """Every 64-pixel chunk of both views once, on its XCD, for the benchmark shapes, tiny and random grids and chunk
    counts per workgroup; with the next pair's table workgroups fused in, every workgroup once."""
    f = lib.smt_adcensus_selftest_maps_grid
    shapes = [(1080, 1920), (720, 1280), (375, 1242), (1, 1), (2, 70), (33, 64), (700, 3), (20, 130)]
    for H, W in shapes:
        nbx = (W + 63) // 64
        ptx, pty, eb = (W + 63) // 64, (H + 31) // 32, (H + 15) // 16
        nprep = ptx * (pty + (eb + ptx - 1) // ptx)
        for K in (1, 2, 3, 4, 7, 8, 16, 64):
            assert f(nbx, H, K, nprep) == 0, (H, W, K)
            assert f(nbx, H, K, 0) == 0, (H, W, K)
    rng = np.random.default_rng(5)
    for _ in range(300):
        nbx, H, K, nprep = int(rng.integers(1, 40)), int(rng.integers(1, 300)), int(rng.integers(1, 65)), int(rng.integers(0, 900))
        assert f(nbx, H, K, nprep) == 0, (nbx, H, K, nprep)
    assert f(0, 10, 8, 1) != 0 and f(4, 10, 0, 1) != 0
