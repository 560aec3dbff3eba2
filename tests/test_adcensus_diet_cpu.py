"""The index rules of the shared AD-Census launch (adcensus_kernels.h, k_cost_maps_shared) without a GPU, over the shapes of
test_adcensus_diet_gpu.py.  The D = 192 kernel computes a ring base once per group of 3 pixels of a wave's walk and
reaches the group's slots at constant offsets (shared_ring_slot), up to 4 slots past the ring's end; the host model in
smt_adcensus_selftest_shared_keys publishes by the same rule -- wave by wave, group by group -- and fails if two live
columns meet in a slot, if a slot is not free after a flush, or if a right pixel does not get its first minimum."""
import ctypes as C

import pytest

# H, W, D of the GPU tests (tables, walk tails and ring, ties, domain) and further ring cases at D = 192: columns of every
# residue mod 512 at the ring's end in a run's first, middle and last group
SHAPES = [(1, 70, 64), (4, 64, 64), (5, 67, 64), (9, 131, 128), (33, 200, 130), (41, 257, 192),
          (3, 257, 192), (3, 258, 192), (3, 259, 192), (3, 304, 192), (6, 700, 192), (4, 1030, 192), (6, 530, 128),
          (6, 330, 192), (40, 330, 192), (2, 1920, 192), (3, 777, 192), (2, 1536, 192), (3, 1537, 191), (2, 600, 256)]


@pytest.fixture(scope="module")
def dll():
    from stereo_match_traditional_amd import build
    d = C.CDLL(build.build())
    d.smt_adcensus_selftest_shared_aux_grid.argtypes = [C.c_int] * 4
    d.smt_adcensus_selftest_shared_aux.argtypes = [C.c_int] * 6
    d.smt_adcensus_selftest_shared_keys.argtypes = [C.c_int] * 4 + [C.c_uint]
    d.smt_adcensus_selftest_fused_grid.argtypes = [C.c_int] * 2
    d.smt_adcensus_selftest_maps_grid.argtypes = [C.c_int] * 4
    return d


@pytest.mark.parametrize("K", [1, 3, 4, 64])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_ring_slots_and_first_minima(dll, H, W, D, K):
    """K = 1: 16-pixel walks (5 groups + 1 pixel); 3, 4: runs of 1 to 4 chunks; 64: many runs on one ring"""
    for seed in range(8):
        assert dll.smt_adcensus_selftest_shared_keys(H, W, D, K, seed) == 0, seed


@pytest.mark.parametrize("K", [1, 4, 64])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_aux_items_and_grids(dll, H, W, D, K):
    nbx = (W + 63) // 64
    nprep = ((W + 63) // 64) * ((H + 31) // 32 + 1)
    assert dll.smt_adcensus_selftest_maps_grid(nbx, H, K, nprep) == 0
    ncost = 8 * ((nbx * H + 8 * K - 1) // (8 * K))
    assert dll.smt_adcensus_selftest_fused_grid(ncost, nprep) == 0
    served = W - 3 - D >= 3                                 # the shared form's shapes; the others take the two-view kernels
    for first in (0, 1):
        for last in (0, 1):
            assert dll.smt_adcensus_selftest_shared_aux(H, W, D, K, first, last) == (0 if served else -1), (first, last)

