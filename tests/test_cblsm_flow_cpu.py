"""The summed-area first pass of smt_cblsm_flow_run_batch rests on box arithmetic that the library checks on the host
(smt_cblsm_selftest_box): rectangle corners in a uint32 table against direct sums, the clipping of arms that leave the
plane, and the exactness argument -- (float)S / (float)n equals costAggregationV5's sequential float sum while S < 2^24,
up to arm length 127 with every entry 255."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from stereo_match_traditional_amd import build
    return ctypes.CDLL(build.build())


def test_box_arithmetic_matches_direct_sums():
    f = _lib().smt_cblsm_selftest_box
    cases = [(1, 1, 1, 0, 0), (1, 1, 1, 5, 1), (1, 37, 3, 34, 0), (29, 1, 3, 34, 1), (17, 33, 5, 34, 0), (40, 70, 3, 34, 1),
             (5, 9, 300, 3, 0), (60, 300, 2, 127, 0), (300, 40, 2, 127, 1)]
    for k, (H, W, D, m, fill) in enumerate(cases):
        assert f(H, W, D, m, fill, 11 + k) == 0, (H, W, D, m, fill)


def test_box_arithmetic_at_the_exactness_bound():
    """All-255 volume, the centre pixel's rectangle 255 x 255: S = 255^3 = 16 581 375, the largest sum the flow's
    summed-area path ever divides; just past it (arm 128) the box sums still match (only the float claim stops)."""
    f = _lib().smt_cblsm_selftest_box
    assert f(255, 255, 1, 127, 1, 5) == 0
    assert f(257, 257, 1, 128, 1, 6) == 0


def test_box_selftest_rejects_bad_sizes():
    f = _lib().smt_cblsm_selftest_box
    assert f(0, 4, 1, 1, 0, 0) == -1
    assert f(4, 4, 0, 1, 0, 0) == -1
    assert f(4, 4, 1, -1, 0, 0) == -1
    assert f(1 << 14, 1 << 13, 1, 1, 0, 0) == -1


def test_cblsm_flow_is_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    for name in ("smt_cblsm_default_params", "smt_cblsm_flow_create_on", "smt_cblsm_flow_destroy",
                 "smt_cblsm_flow_set_stream", "smt_cblsm_flow_run_batch", "smt_cblsm_flow_volumes",
                 "smt_cblsm_flow_status", "smt_cblsm_selftest_box"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_lib(), name), name


def test_cblsm_default_params_are_cblsm_cpp_values():
    from stereo_match_traditional_amd import _lib as L
    p = L.CBLSMParams()
    _lib().smt_cblsm_default_params(ctypes.byref(p))
    assert (p.tau, p.sec_length, p.max_length) == (25, 17, 34)
