"""The shared maps-only form with runs walked in one pass (adcensus_kernels.h, k_cost_maps_shared) without a GPU: the host walk
of the form's rules (smt_adcensus_selftest_shared_keys) over the shapes and chunk counts of
test_adcensus_shared_runs_gpu.py.  A workgroup's consecutive chunks of one row form a run, cut into sub-runs of SH_RUN = 4
chunks; a run is published as a whole and flushed once.  Every right pixel must be written exactly once with its first
minimum, no two live columns may meet in a ring slot, rings end empty and the key map is reset.  That the shapes reach a
4-chunk run, a sub-run, a row change inside a workgroup, a walk cut by W and the ring's bound of 511 live columns is
asserted on a Python recomputation of the run structure (adcensus_shared_runs_cases.py)."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adcensus_shared_runs_cases import CHUNKS, SHAPES, features, workgroup_runs  # noqa: E402

KS = [int(k) if k else 4 for k in CHUNKS]


@pytest.fixture(scope="module")
def selftest():
    from stereo_match_traditional_amd import build
    f = C.CDLL(build.build()).smt_adcensus_selftest_shared_keys
    f.argtypes = [C.c_int] * 4 + [C.c_uint]
    f.restype = C.c_int
    return f


def test_every_chunk_is_in_exactly_one_run():
    for H, W, D, _ in SHAPES:
        for K in KS:
            seen = [(i, bx + u) for runs in workgroup_runs(H, W, K) for i, bx, n in runs for u in range(n)]
            assert sorted(seen) == [(i, bx) for i in range(H) for bx in range((W + 63) // 64)], (H, W, K)


@pytest.mark.parametrize("H,W,D,K,want", [
    (6, 330, 192, 4, {"run4": True, "row_change": True}),                      # the benchmark's K: 64 pixels per wave
    (6, 330, 192, 5, {"run4": True, "subrun": True, "row_change": True}),
    (7, 259, 192, 5, {"run4": True, "subrun": True, "cut_by_W": True}),
    (6, 700, 192, 8, {"run4": True, "subrun": True, "row_change": True}),      # runs longer than SH_RUN
    (6, 700, 192, 64, {"run4": True, "subrun": True, "row_change": True}),
    (6, 390, 64, 4, {"run4": True, "row_change": True}),
    (5, 460, 100, 8, {"run4": True, "subrun": True, "row_change": True}),
    (8, 700, 256, 5, {"run4": True, "subrun": True, "live": 511}),             # the ring (512) at its bound
    (8, 700, 256, 4, {"run4": True, "live": 509}),
    (2, 259, 192, 4, {"cut_by_W": True, "run4": False})])
def test_the_shapes_reach_what_they_are_there_for(H, W, D, K, want):
    assert (H, W, D) in [s[:3] for s in SHAPES] and K in KS
    f = features(H, W, D, K)
    assert {k: f[k] for k in want} == want


def test_no_run_has_more_live_columns_than_the_ring():
    assert max(features(H, W, D, K)["live"] for H, W, D, _ in SHAPES for K in KS) == 511


# the ids the cases had while a second parameter chose between two walks: they keep their names
@pytest.mark.parametrize("H,W,D,form", SHAPES, ids=["%d-%d-%d-%s-None" % s for s in SHAPES])
def test_shared_keys_walk(selftest, H, W, D, form):
    for K in KS:
        for seed in (0, 1, 2):
            assert selftest(H, W, D, K, seed) == 0, (K, seed)
