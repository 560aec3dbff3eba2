"""The C ABI's contract about the caller's memory (include/smt.h, "Caller buffers"), for every entry point that takes
device buffers: called through libsmt_hip.so with pointers into an arena (tests/arena.py) on torch's current stream,
every case of tests/bounds_cases.py asserts
  * the guards in front of and behind every tensor, and the gaps between the maps of a strided batch, come back
    untouched under both fill seeds (no store outside the documented extents);
  * the inputs come back untouched;
  * the outputs of the two seeds -- prefilled with patterns that differ in every byte, one of them all NaN words and
    high bytes -- are bit-identical (every output element is written, and no byte beside an input reaches a result);
  * the outputs equal the CPU oracle by the rule of the entry's own parity test.
Tensors start at their natural alignment and at nothing coarser (an odd multiple of the item size modulo 16): no entry
point needs more, see the header.  Optional outputs are exercised present and NULL.

Then scratch history: every user of the scratch arena (csrc/scratch.hip) runs once warm, once after
smt_scratch_poison(0xFF) and once after smt_scratch_poison(0x00); the three outputs are bit-identical, equal the oracle,
and the arena's reserved bytes do not change across the last two calls, so the poisoned blocks were the ones reused.

Out of reach: a load outside an input that neither faults nor reaches the result.  Nothing here can see it (that takes
a device-side address sanitizer, which this suite does not use); the random, never flat images only make sure that such
a load, where it does reach the result, moves it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402

pytestmark = pytest.mark.gpu

_ALL = [(n, p) for n in BC.ENTRIES if n not in BC.HOST_ENTRIES for p in BC.CASES[n]]


@pytest.fixture(scope="module")
def X(smt, O):
    return BC.Ctx(O, "cuda:0")


@pytest.mark.parametrize("name,params", _ALL, ids=[f"{n}-{BC.case_id(p)}" for n, p in _ALL])
def test_guards_prefill_inputs_and_oracle(X, name, params):
    BC.run_case(X, name, params)


def test_the_table_covers_every_caller_buffer_entry():
    assert not set(BC.REQUIRED) - {n for n, _ in _ALL}


# every user of the scratch arena, at a shape of its table
_SCRATCH = [("smt_ncc", dict(H=5, W=19, D=64, win=1, impl=2, cost=True)),
            ("smt_ncc", dict(H=7, W=37, D=65, win=2, impl=2, cost=False))]
_SCRATCH += [("smt_asw", dict(H=3, W=33, D=64, ws=1, view=v, impl=i, cost=True)) for i in (3, 4, 5, 6) for v in (BC.VL, BC.VR)]
_SCRATCH += [("smt_asw_both", dict(H=2, W=17, D=65, ws=2, impl=i, costs=c)) for i in (1, 2) for c in ("", "LR")]
_SCRATCH += [("smt_sad_both", dict(H=5, W=29, D=65, ws=2, dispatch=1, impl=i, cost=False)) for i in (2, 1)]
_SCRATCH += [("smt_sad_both", dict(H=7, W=33, D=64, ws=1, dispatch=1, impl=2, cost=True, band=3)),
             ("smt_remove_speckles_batch", dict(H=33, W=34, gap=1)), ("smt_fill_the_hole_batch", dict(row=9, col=33, D=8, P=3, gap=7))]


@pytest.mark.parametrize("name,params", _SCRATCH, ids=[f"{n}-{BC.case_id(p)}" for n, p in _SCRATCH])
def test_scratch_history_does_not_reach_the_result(X, smt, name, params):
    warm = BC.run_case(X, name, params)                       # two seeds, guards, oracle; leaves the arena grown
    outs, reserved = [], []
    for byte in (0xFF, 0x00):
        smt.scratch_poison(byte)
        o, verify = BC.run_once(X, name, params, arena.SEEDS[0])
        verify(o)
        outs.append(o)
        reserved.append(smt.scratch_info()[0])
    BC.assert_same(warm, outs[0], f"{name}: warm call against the call on scratch filled with 0xFF")
    BC.assert_same(warm, outs[1], f"{name}: warm call against the call on scratch filled with 0x00")
    assert reserved[0] == reserved[1] > 0, reserved           # the poisoned blocks were the ones handed out again


def test_scratch_poison_on_an_empty_arena(smt):
    """SMT_OK in arena mode, whatever the arena holds -- also when it holds nothing"""
    smt.scratch_trim(0)
    assert smt.scratch_info() == (0, 0)
    smt.scratch_poison(0xA5)
    assert smt.scratch_info() == (0, 0)
