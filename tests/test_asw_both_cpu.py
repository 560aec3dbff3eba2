"""smt_asw_both takes the right view's ASW costs from the left view's: costR(i, x', d) = costL(i, x' + d, d) wherever
ASW.h:401 accepts d, because the tap weight is one factor per image and the truncated error is symmetric.  Without a
GPU: the new entry points exist, the rank-key encoding passes the library's host-side check, and the identity itself
holds on the oracle bit for bit (the premise, pinned for whoever changes the oracle next)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("smt_asw_both", "smt_asw_both_set_impl", "smt_asw_default_params", "smt_asw_flow_create_on",
         "smt_asw_flow_destroy", "smt_asw_flow_set_stream", "smt_asw_flow_run_batch", "smt_asw_selftest_right_keys")


def _lib():
    from stereo_match_traditional_amd import build
    return ctypes.CDLL(build.build())


def right_from_left(cl, wins):
    """The right view's cost volume and map rebuilt from a left volume [H][W][D]: diagonal gather where x' + d <=
    W - wins - 2, then the chain cv[d] = cv[d-1] (ASW.h:422-425), NaN where even d = 0 is rejected; WinTakeAll
    (:193-208): first strict minimum, a NaN never satisfies `min > value`."""
    H, W, D = cl.shape
    xlim = W - wins - 2
    cr = np.full((H, W, D), np.nan, np.float32)
    dr = np.zeros((H, W), np.float32)
    for x in range(W):
        if x > xlim:
            continue
        for d in range(D):
            cr[:, x, d] = cl[:, x + d, d] if x + d <= xlim else cr[:, x, d - 1]
        mn = cr[:, x, 0].copy()
        for d in range(1, D):
            with np.errstate(invalid="ignore"):
                better = mn > cr[:, x, d]
            mn[better] = cr[better, x, d]
            dr[better, x] = d
    return cr, dr


def test_asw_both_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_lib(), name), name


def test_asw_default_params_are_asweight_cpp_values():
    from stereo_match_traditional_amd import _lib as L
    p = L.ASWParams()
    _lib().smt_asw_default_params(ctypes.byref(p))
    assert (p.winSize, p.T, p.sigma_space, p.sigma_color) == (11, 40, 50.0, 30.0)


def test_both_set_impl_accepts_1_and_2_only():
    f = _lib().smt_asw_both_set_impl
    assert f(1) == 0 and f(2) == 0
    for bad in (0, 3, -1):
        assert f(bad) == -1


def test_rank_key_minimum_is_wintakeall_of_the_chained_right_row():
    f = _lib().smt_asw_selftest_right_keys
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    for k, (W, D, wins) in enumerate([(40, 16, 3), (96, 48, 6), (300, 300, 3), (64, 512, 2), (200, 128, 17), (24, 1, 3),
                                      (20, 130, 4), (7, 5, 9), (960, 128, 17)]):
        for seed in (1, 2, 3):
            assert f(W, D, wins, 100 * k + seed) == 0, (W, D, wins, seed)
    assert f(0, 4, 1, 0) == -1 and f(4, 0, 1, 0) == -1 and f(4, 513, 1, 0) == -1 and f(4, 4, -1, 0) == -1


@pytest.mark.parametrize("H,W,D,winSize,seed,noise", [(14, 40, 16, 2, 1, False), (10, 36, 64, 4, 2, True),
                                                     (8, 30, 70, 1, 3, False), (6, 24, 1, 2, 4, False),
                                                     (5, 20, 130, 3, 5, True), (9, 300, 300, 2, 7, False),
                                                     (12, 200, 128, 16, 9, False), (24, 96, 48, 5, 11, True)])
def test_oracle_right_view_is_the_left_views_diagonal(O, H, W, D, winSize, seed, noise):
    """Passes before the feature exists, on purpose: it pins the identity on the oracle alone."""
    L, R = O.synth_pair(H, W, 32, seed, noise)
    pad = winSize + 1
    Lp, Rp = O.pad_replicate(L, pad), O.pad_replicate(R, pad)
    sp, cm = O.asw_masks(winSize, 50.0, 30.0)
    dl, cl = O.asw(Lp, Rp, D, winSize, sp, cm, 40, 0, want_cost=True)
    dr, cr = O.asw(Lp, Rp, D, winSize, sp, cm, 40, 1, want_cost=True)
    cr2, dr2 = right_from_left(cl, pad)
    assert np.array_equal(np.isnan(cr2), np.isnan(cr))
    assert np.array_equal(cr2.view(np.uint32)[~np.isnan(cr)], cr.view(np.uint32)[~np.isnan(cr)])
    assert np.array_equal(dr2, dr)
