"""The shared maps-only form with the edges finished apart (adcensus_kernels.h, k_cost_maps_shared + k_shared_finish) without
a GPU.  Every left hypothesis (j, d) with j <= W-4 and j - d >= 3 publishes to right column j - d; a right column
j' > W-3-D lacks only its edge hypotheses W-3 <= j' + d <= W+3, because the right view's cost is constant in d from
W+3-j' on (the staging clamps the census index to W+3 and the value index to W-1); the columns 0..2 share nothing.
Checked on the oracle's volumes, and on the host walk of the form's rules (smt_adcensus_selftest_shared_keys)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def selftest():
    from stereo_match_traditional_amd import build
    f = C.CDLL(build.build()).smt_adcensus_selftest_shared_keys
    f.argtypes = [C.c_int] * 4 + [C.c_uint]
    f.restype = C.c_int
    return f


ORACLE_SHAPES = [(6, 230, 192), (5, 90, 64), (4, 140, 100), (3, 70, 64), (5, 200, 192), (4, 262, 256), (3, 134, 128)]


@pytest.fixture(scope="module")
def volumes(O):
    """both views' oracle volumes as bit patterns, once per shape"""
    out = {}
    for H, W, D in ORACLE_SHAPES:
        L, R = O.synth_pair(H, W, D, 4700 + W, noise=True)
        out[(H, W, D)] = (O.adcensus_view(L, R, D, 10.0, 30.0, 0).view(np.uint32),
                          O.adcensus_view(L, R, D, 10.0, 30.0, 1).view(np.uint32))
    return out


@pytest.mark.parametrize("H,W,D", ORACLE_SHAPES)
def test_right_cost_is_constant_past_the_clamps(volumes, H, W, D):
    _, volR = volumes[(H, W, D)]
    n = 0
    for c in range(W):
        d0 = W + 3 - c
        if d0 < D - 1:
            assert (volR[:, c, d0:] == volR[:, c, d0:d0 + 1]).all(), c
            n += 1
    assert n == min(W, D - 5)                              # the columns c > W+4-D


@pytest.mark.parametrize("H,W,D", ORACLE_SHAPES)
def test_right_map_from_shared_and_edge_hypotheses(O, volumes, H, W, D):
    """first minimum over the keys cost bits << 32 | d of the left volume's shareable costs and the right volume's edge
    hypotheses, column by column, is the right volume's WTA"""
    volL, volR = volumes[(H, W, D)]
    want = O.wta(volR.view(np.float32))
    nokey = np.uint64(0xFFFFFFFFFFFFFFFF)
    got = np.empty((H, W), np.float32)
    nshared = nedge = 0
    for c in range(W):
        key = np.full(H, nokey, np.uint64)
        for d in range(D):                                 # published by left pixel j = c + d
            if c >= 3 and c + d <= W - 4:
                key = np.minimum(key, (volL[:, c + d, d].astype(np.uint64) << np.uint64(32)) | np.uint64(d))
                nshared += 1
        lo = max(0, W - 3 - c) if c >= 3 else 0
        hi = min(D - 1, W + 3 - c)
        assert hi - lo <= 6 or c < 3
        for d in range(lo, hi + 1):                        # edge hypotheses, right-view arithmetic
            key = np.minimum(key, (volR[:, c, d].astype(np.uint64) << np.uint64(32)) | np.uint64(d))
            nedge += 1
        assert (key != nokey).all()
        got[:, c] = (key & np.uint64(0xFFFFFFFF)).astype(np.float32)
    assert np.array_equal(got, want)
    assert nshared > 0 and nedge <= 3 * D + 7 * (D + 2)


# W-3-D == 3; (W-2-D) % 64 in {0, 1, 63}; W % 64 in {0, 1, 3, 4, 63}; every D / 64, a D that is no multiple of 64, rows
# shorter and longer than a run
WALK_SHAPES = [(3, 70, 64), (2, 198, 192), (2, 262, 256),                      # W-3-D == 3
               (3, 130, 64), (3, 131, 64), (3, 193, 64),                       # (W-2-D) % 64 = 0, 1, 63 (W % 64 = 2, 3, 1)
               (2, 258, 192), (2, 259, 192), (2, 321, 192), (2, 230, 100),     # the same at C = 3 and C = 2
               (3, 128, 64), (3, 129, 64), (3, 132, 64), (3, 191, 64),         # W % 64 = 0, 1, 4, 63
               (2, 256, 192), (2, 257, 192), (2, 260, 192), (2, 319, 192), (2, 323, 192),
               (2, 320, 256), (2, 323, 256), (2, 383, 256), (1, 640, 192), (5, 211, 33)]


def test_walk_shapes_reach_the_rules():
    assert {W - 3 - D for _, W, D in WALK_SHAPES} >= {3}
    assert {(W - 2 - D) % 64 for _, W, D in WALK_SHAPES} >= {0, 1, 63}
    assert {W % 64 for _, W, D in WALK_SHAPES} >= {0, 1, 3, 4, 63}


@pytest.mark.parametrize("K", [1, 3, 4, 64])
@pytest.mark.parametrize("H,W,D", WALK_SHAPES)
def test_shared_keys_walk_with_edges(selftest, H, W, D, K):
    for seed in (0, 1, 2, 7):
        assert selftest(H, W, D, K, seed) == 0, seed
