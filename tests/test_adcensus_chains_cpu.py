"""The chained batch schedule of smt_adcensus_compute_batch (adcensus_rules.h, chain_plan) without a GPU.  The host selftest
writes down the plan that the call itself issues -- which chain, stream, table sets and key maps every launch uses, and
the fork and join events -- and computes happens-before over it: every table set is built before it is read and not
rebuilt under a reader, every key map is merged, converted once and merged again in a total order, every right map is
complete and every internal stream joined before the call ends on the caller's stream
(smt_adcensus_selftest_chains, include/smt.h)."""
import ctypes as C
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {"default": 0, "pairs": 1, "ab": 2, "ba": 3}
SHARED, LAST_VOLUMES, FORK_START, FINISH_APART = 1, 2, 4, 8


@pytest.fixture(scope="module")
def dll():
    from stereo_match_traditional_amd import build
    d = C.CDLL(build.build())
    d.smt_adcensus_selftest_chains.argtypes = [C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_int, C.c_uint]
    return d


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("chains", [1, 2, 3])
@pytest.mark.parametrize("pairs", range(2, 10))
def test_plan_is_ordered(dll, pairs, chains, order):
    """every parity of the chains' starting counters (earlier calls of odd size, single pairs in between), the shared
    form and the two-view one, a last pair that writes volumes, either fork, either finish"""
    for parity in itertools.product((0, 1), repeat=3):
        counts = [7 + 2 * c + parity[c] for c in range(3)]
        for flags in range(16):
            assert dll.smt_adcensus_selftest_chains(pairs, chains, *counts, ORDERS[order], flags) == 0, (parity, flags)


def test_one_pair_and_long_batches(dll):
    for pairs in (1, 10, 11, 64, 65):
        for chains in (1, 2, 3):
            for order in ORDERS.values():
                assert dll.smt_adcensus_selftest_chains(pairs, chains, 0, 1, 0, order, SHARED) == 0, (pairs, chains, order)


def test_bad_arguments_refused(dll):
    for bad in [(0, 2, 0, 0, 0, 0, 0), (-1, 2, 0, 0, 0, 0, 0), (513, 2, 0, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0),
                (4, 4, 0, 0, 0, 0, 0), (4, 2, -1, 0, 0, 0, 0), (4, 2, 0, -1, 0, 0, 0), (4, 2, 0, 0, -1, 0, 0),
                (4, 2, 0, 0, 0, -1, 0), (4, 2, 0, 0, 0, 4, 0), (4, 2, 0, 0, 0, 0, 16)]:
        assert dll.smt_adcensus_selftest_chains(*bad) == -1, bad


def test_header_documents_the_schedule_and_its_hooks():
    text = open(os.path.join(ROOT, "include", "smt.h")).read()
    for word in ("SMT_CHAINS", "SMT_CHAIN_FORK", "SMT_CHAIN_ORDER", "smt_adcensus_selftest_chains", "0 / 1 / 2 / 3"):
        assert word in text, word
