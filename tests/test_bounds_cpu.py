"""The bounds suite where there is no device: (1) the arena helper itself against numpy stand-ins of an entry point that
each make one of the mistakes the suite exists for -- the evidence that tests/test_bounds_gpu.py can fail, obtained
without running a broken kernel anywhere; (2) the host twins smt_fill_the_hole_batch_host and
smt_median_filter_inplace_host / _host_ex through the arena with front and back guards and strided gaps, against the
oracle; (3) completeness: every function include/smt.h declares is a key of the bounds table or is listed in
NOT_CALLER_BUFFER with a reason."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, H, W = 3, 5, 7
STRIDE = H * W + 7


def _view(A, name, shape, dtype, before=0):
    """numpy view of a tensor of a host arena with `before` elements on either side of it (what a stray pointer sees)"""
    isz = np.dtype(dtype).itemsize
    off = A.addr(name) - A.base - before * isz
    n = int(np.prod(shape)) + 2 * before
    return A.buf[off:off + n * isz].view(dtype)


def _standin(mistake):
    """out[b] = 2 * in[b] + 1 on float32 [P][H][W] maps STRIDE elements apart, with one mistake"""
    src = np.arange(P * H * W, dtype=np.float32).reshape(P, H, W)

    def make(A):
        A.inp("in", src, stride=STRIDE)
        A.out("out", (P, H, W), np.float32, stride=STRIDE)

        def call(A):
            span = (P - 1) * STRIDE + H * W
            i = _view(A, "in", (span,), np.float32, before=1)
            o = _view(A, "out", (span,), np.float32, before=1)
            for b in range(P):
                lo = 1 + b * STRIDE
                o[lo:lo + H * W] = 2 * i[lo:lo + H * W] + 1
            if mistake == "past the end":
                o[1 + span] = 3.0
            elif mistake == "before the start":
                o[0] = 3.0
            elif mistake == "batch gap":
                o[1 + H * W + 2] = 3.0
            elif mistake == "unwritten element":
                o[1 + STRIDE + 4] = A.initial("out").reshape(-1)[H * W + 4]      # what the prefill put there
            elif mistake == "guard reaches the result":
                o[1] = 2 * i[1] + 1 + (0.0 if np.isnan(i[0]) else 1.0)           # reads the element before the input
            elif mistake == "input modified":
                i[1 + 3] += 1.0
            return 0
        return call
    return make, 2 * src + 1


def test_a_correct_standin_passes():
    make, want = _standin(None)
    outs, _ = arena.run_two_seeds(make)
    assert np.array_equal(outs["out"], want)


@pytest.mark.parametrize("mistake,says", [("past the end", "back guard of out"),
                                          ("before the start", "front guard of out"),
                                          ("batch gap", "batch gap of out"),
                                          ("unwritten element", "out depends on the prefill"),
                                          ("guard reaches the result", "out depends on the prefill or on the guards"),
                                          ("input modified", "input in, map 0, byte 1")])
def test_every_mistake_is_rejected(mistake, says):
    make, _ = _standin(mistake)
    with pytest.raises(AssertionError) as e:
        arena.run_two_seeds(make)
    assert says in str(e.value), str(e.value)


def test_layout_rules():
    """guards of a full row-block and at least 4 KiB on both sides, natural alignment and nothing coarser, patterns that
    differ in every byte, NaN words and high bytes under the odd seed"""
    for seed in arena.SEEDS:
        A = arena.Arena(seed)
        A.inp("u8", np.zeros((3, 5), np.uint8)); A.out("f32", (2, 70, 300), np.float32); A.out("f64", (3, 3), np.float64)
        A.inout("i32", np.zeros((4, 2, 2), np.int32), stride=9)
        A.build()
        ends = []
        for name, isz, guard in (("u8", 1, 4096), ("f32", 4, 70 * 300 * 4), ("f64", 8, 4096), ("i32", 4, 4096)):
            off = A.addr(name) - A.base
            assert off % isz == 0 and ((off % 16) // isz) % 2 == 1, (name, off)
            assert A._t[name].guard == guard
            assert not ends or off - ends[-1] >= guard + A._t[prev].guard
            ends.append(off + A._t[name].span)
            prev = name
        assert A.nbytes - ends[-1] >= 4096 and A.addr("u8") - A.base >= 4096
    a, b = arena.pattern(1 << 16, arena.SEEDS[0]), arena.pattern(1 << 16, arena.SEEDS[1])
    assert (a != b).all() and (a[1:] != a[:-1]).all() and (a < 0x80).all() and (b >= 0x80).all()
    assert np.isnan(b.view(np.float32)).all() and np.isnan(b.view(np.float64)).all() and (b.view(np.int32) < 0).all()


@pytest.fixture(scope="module")
def X(O):
    return BC.Ctx(O, None)


_HOST = [(name, p) for name in BC.HOST_ENTRIES for p in BC.CASES[name]]


@pytest.mark.parametrize("name,params", _HOST, ids=[f"{n}-{BC.case_id(p)}" for n, p in _HOST])
def test_host_twins_in_the_arena(X, name, params):
    BC.run_case(X, name, params)


def _declared():
    text = open(os.path.join(ROOT, "include", "smt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(smt_\w+)\s*\(", text))


def test_every_declared_function_has_a_decision():
    declared, table, other = _declared(), set(BC.ENTRIES), set(BC.NOT_CALLER_BUFFER)
    assert len(declared) > 100
    assert not table & other, sorted(table & other)
    assert not declared - table - other, f"no bounds case and no reason: {sorted(declared - table - other)}"
    assert not (table | other) - declared, f"not in the header: {sorted((table | other) - declared)}"
    assert not set(BC.REQUIRED) - table, f"caller-buffer entries without a case: {sorted(set(BC.REQUIRED) - table)}"
    assert all(isinstance(r, str) and r for r in BC.NOT_CALLER_BUFFER.values())
    assert all(BC.CASES[n] for n in BC.ENTRIES), "an entry without cases"
