"""The shared maps-only form of the AD-Census batch (adcensus_kernels.h, k_cost_maps_shared) without a GPU: the host walk of
its run / ring / flush / merge arithmetic (smt_adcensus_selftest_shared_keys), and the identity it rests on, checked on
the oracle's volumes: for 3 <= j' and j' + d <= W-4 the right view's cost(i, j', d) has the bits of the left view's
cost(i, j' + d, d), so the right WTA map of the columns 3 <= j' <= W-3-D is the first minimum along a diagonal of the
left volume."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def selftest():
    from stereo_match_traditional_amd import build
    f = C.CDLL(build.build()).smt_adcensus_selftest_shared_keys
    f.argtypes = [C.c_int] * 4 + [C.c_uint]
    f.restype = C.c_int
    return f


# H, W, D: W < D+6 (empty set), W == D+6 (one shared column), W no multiple of 64, H = 1, rows shorter and longer than a
# run, every D / 64 and a D that is no multiple of 64
SHAPES = [(3, 69, 64), (9, 70, 256), (4, 261, 256), (3, 70, 64), (8, 198, 192), (2, 262, 256), (5, 106, 100),
          (12, 230, 192), (11, 90, 64), (20, 140, 100), (9, 300, 256), (1, 500, 192), (1, 64, 20), (18, 330, 192),
          (5, 450, 256), (24, 200, 64), (3, 1030, 192), (2, 640, 128), (7, 129, 33)]


@pytest.mark.parametrize("K", [1, 3, 4, 64])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_shared_keys_walk(selftest, H, W, D, K):
    for seed in (0, 1, 2, 7):                              # palette with ties, every cost equal, mostly distinct, palette
        assert selftest(H, W, D, K, seed) == 0, seed


def test_shared_keys_walk_arguments(selftest):
    for bad in [(0, 100, 64, 4), (4, 0, 64, 4), (4, 100, 0, 4), (4, 100, 257, 4), (4, 100, 64, 0), (4, 100, 64, 65)]:
        assert selftest(*bad, 0) == -1, bad


@pytest.mark.parametrize("H,W,D", [(12, 230, 192), (11, 90, 64), (20, 140, 100), (9, 300, 256), (8, 198, 192)])
def test_identity_on_oracle_volumes(O, H, W, D):
    L, R = O.synth_pair(H, W, D, 4100 + W, noise=True)
    volL = O.adcensus_view(L, R, D, 10.0, 30.0, 0).view(np.uint32)
    volR = O.adcensus_view(L, R, D, 10.0, 30.0, 1).view(np.uint32)
    n = 0
    for d in range(D):
        jr = np.arange(3, W - 3 - d)                       # j' >= 3 and j' + d <= W-4
        if jr.size == 0:
            continue
        assert np.array_equal(volR[:, jr, d], volL[:, jr + d, d]), d
        n += H * jr.size
    assert n > 0
    # hence the right map of the identity set is the first minimum along the left volume's diagonal
    hi = W - 3 - D
    if hi >= 3:
        want = O.wta(volR.view(np.float32))
        cols = np.arange(3, hi + 1)
        diag = volL.view(np.float32)[:, cols[:, None] + np.arange(D)[None, :], np.arange(D)[None, :]]   # [H][cols][D]
        assert np.array_equal(np.argmin(diag, axis=2).astype(np.float32), want[:, cols])


def test_header_documents_the_hook_and_the_selftest():
    text = open(os.path.join(ROOT, "include", "smt.h")).read()
    assert "SMT_MAPS_SHARED" in text and "smt_adcensus_selftest_shared_keys" in text
