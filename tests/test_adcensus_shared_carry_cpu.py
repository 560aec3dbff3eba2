"""The auxiliary work items of a shared AD-Census launch (adcensus_kernels.h, k_cost_maps_shared) without a GPU: the edge
items of the launch's own pair, the conversion items of the pair before it and the table tiles of the pair after it ride
in the fused grid's table class.  The host selftests run the kernel's own index functions: every cost workgroup and every
item decoded exactly once (smt_adcensus_selftest_shared_aux_grid), the items' pixel arithmetic covering its column set
exactly once and no edge range empty (smt_adcensus_selftest_shared_aux), and the split finish -- edge merges in either
order against the publishes, then the conversion -- equal to the single pass (smt_adcensus_selftest_shared_keys)."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dll():
    from stereo_match_traditional_amd import build
    d = C.CDLL(build.build())
    d.smt_adcensus_selftest_shared_aux_grid.argtypes = [C.c_int] * 4
    d.smt_adcensus_selftest_shared_aux.argtypes = [C.c_int] * 6
    d.smt_adcensus_selftest_shared_keys.argtypes = [C.c_int] * 4 + [C.c_uint]
    d.smt_adcensus_selftest_fused_grid.argtypes = [C.c_int] * 2
    return d


# ncost, nprep, nedge, nconv: each of the last three zero in turn, all zero, one cost group, fewer and more auxiliary
# groups than cost groups, the headline's counts (1080p x 192, K = 4) with and without each part
GRIDS = [(8, 5, 3, 2), (8, 0, 3, 2), (8, 5, 0, 2), (8, 5, 3, 0), (8, 0, 0, 0), (8, 0, 1, 0), (8, 40, 30, 20),
         (16, 1, 1, 1), (64, 7, 9, 8), (72, 9, 0, 100), (8104, 1110, 256, 507), (8104, 0, 256, 507), (8104, 1110, 256, 0),
         (8104, 0, 256, 0), (24, 3, 200, 0), (1000, 17, 5, 333)]


@pytest.mark.parametrize("ncost,nprep,nedge,nconv", GRIDS)
def test_every_workgroup_and_item_decoded_once(dll, ncost, nprep, nedge, nconv):
    assert dll.smt_adcensus_selftest_shared_aux_grid(ncost, nprep, nedge, nconv) == 0
    if nprep > 0:                                          # the table-only grid keeps its meaning
        assert dll.smt_adcensus_selftest_fused_grid(ncost, nprep) == 0


def test_grid_arguments(dll):
    for bad in [(0, 1, 1, 1), (12, 1, 1, 1), (8, -1, 1, 1), (8, 1, -1, 1), (8, 1, 1, -1)]:
        assert dll.smt_adcensus_selftest_shared_aux_grid(*bad) == -1, bad


# H, W, D.  H = 1; idhi == 3 (W == D + 6); W - 3 - D == 66; item sizes that divide their set exactly ((32, 128, 64): 4096
# keys, one conversion item; (16, 128, 62): 16 x 64 edge pixels, one edge item) and that do not; more than one item of
# every kind; 3 H a multiple of 64 and not; every C and ragged D; the GPU tests' shapes
SHAPES = [(1, 70, 64), (1, 500, 192), (3, 70, 64), (5, 198, 192), (4, 262, 256), (7, 133, 64), (6, 261, 192),
          (32, 128, 64), (16, 128, 62), (64, 140, 100), (65, 330, 192), (6, 259, 192), (6, 330, 192), (5, 140, 100),
          (7, 129, 33), (12, 330, 192), (10, 140, 100), (40, 700, 192), (128, 96, 20), (3, 1030, 192)]


@pytest.mark.parametrize("K", [1, 4, 64])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_items_cover_their_pixels_once(dll, H, W, D, K):
    for first in (0, 1):
        for last in (0, 1):
            assert dll.smt_adcensus_selftest_shared_aux(H, W, D, K, first, last) == 0, (first, last)


def test_aux_arguments(dll):
    # an empty identity set is the two-view kernel's shape
    for bad in [(0, 100, 64, 4), (4, 0, 64, 4), (4, 100, 0, 4), (4, 100, 257, 4), (4, 100, 64, 0), (4, 100, 64, 65),
                (4, 69, 64, 4)]:
        assert dll.smt_adcensus_selftest_shared_aux(*bad, 0, 0) == -1, bad


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_split_finish_equals_the_single_pass(dll, H, W, D):
    """seed & 4 merges the edge keys in front of the publishes instead of behind them"""
    for seed in (0, 1, 2, 4, 5, 6):
        assert dll.smt_adcensus_selftest_shared_keys(H, W, D, 4, seed) == 0, seed


def test_header_documents_both_forms_and_the_selftests():
    text = open(os.path.join(ROOT, "include", "smt.h")).read()
    for word in ("SMT_SHARED_FINISH", "apart", "smt_adcensus_selftest_shared_aux", "smt_adcensus_selftest_shared_aux_grid"):
        assert word in text, word
