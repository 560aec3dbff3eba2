"""Tapered tail of the maps-only launches (adcensus_rules.h: maps_span, maps_span_groups) without a GPU.  The library's own
check of the span rule (smt_adcensus_selftest_spans: every chunk in exactly one group, no group across its slice or
longer than K, the group count the companion's, n2 = n1 = 0 the plain rule) over short launches, launches around the
size of a few rounds of workgroups and the headline's 32 400 chunks, with tails from none to longer than the slice; then
the host walk of the shared form (smt_adcensus_selftest_shared_keys, which takes the taper where the launch does) under
forced tapers over the shapes and chunk counts of adcensus_shared_runs_cases.py."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adcensus_shared_runs_cases import CHUNKS, SHAPES  # noqa: E402

NBS = list(range(1, 81)) + [2000, 2047, 2048, 2049, 32400]
KS = [1, 2, 3, 4, 5, 8, 64]
TAILS = [(0, 0), (0, 1), (1, 0), (1, 2), (3, 3), (7, 50), (1000, 1000)]      # the last: longer than the slice
FORCED = ["0,2", "1,2", "3,1"]


@pytest.fixture(scope="module")
def dll():
    from stereo_match_traditional_amd import build
    d = C.CDLL(build.build())
    d.smt_adcensus_selftest_spans.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int]
    d.smt_adcensus_selftest_spans.restype = C.c_int
    d.smt_adcensus_selftest_shared_keys.argtypes = [C.c_int] * 4 + [C.c_uint]
    d.smt_adcensus_selftest_shared_keys.restype = C.c_int
    return d


@pytest.mark.parametrize("K", KS)
def test_span_rule(dll, K):
    for nb in NBS:
        for n2, n1 in TAILS:
            assert dll.smt_adcensus_selftest_spans(nb, K, n2, n1) == 0, (nb, n2, n1)


def test_span_rule_rejects_bad_arguments(dll):
    for args in ((0, 4, 0, 0), (10, 0, 0, 0), (10, 65, 0, 0), (10, 4, -1, 0), (10, 4, 0, -1)):
        assert dll.smt_adcensus_selftest_spans(*args) != 0, args


@pytest.mark.parametrize("taper", FORCED)
def test_shared_keys_walk_under_forced_tapers(dll, taper, monkeypatch):
    monkeypatch.setenv("SMT_MAPS_TAPER", taper)          # read at every call; restored by monkeypatch
    for H, W, D, _ in SHAPES:
        for K in [int(k) if k else 4 for k in CHUNKS]:
            assert dll.smt_adcensus_selftest_shared_keys(H, W, D, K, 0) == 0, (H, W, D, K)
