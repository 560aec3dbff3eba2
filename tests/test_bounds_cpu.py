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
import stream_order_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, H, W = 3, 5, 7
STRIDE = H * W + 7


def _view(A, name, shape, dtype, before=0):
    """numpy view of a tensor of a host arena with `before` elements on either side of it (what a stray pointer sees)"""
    isz = np.dtype(dtype).itemsize
    off = A.addr(name) - A.base - before * isz
    n = int(np.prod(shape)) + 2 * before
    return A.buf[off:off + n * isz].view(dtype)


def _standin(mistake, deferred=False):
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

        def call_deferred(A):
            """the same on an arena whose inputs arrive late: in program order, what a launch that is not ordered behind
            the caller's stream sees (reads before arrive()) and what becomes of what it wrote (writes before arrive())"""
            span = (P - 1) * STRIDE + H * W
            i = _view(A, "in", (span,), np.float32)
            o = _view(A, "out", (span,), np.float32)

            def compute():
                return [2 * i[b * STRIDE:b * STRIDE + H * W] + 1 for b in range(P)]

            def store(vals):
                for b in range(P):
                    o[b * STRIDE:b * STRIDE + H * W] = vals[b]

            if mistake == "reads before the inputs arrive":
                vals = compute()
                A.arrive()
                store(vals)
            elif mistake == "writes before the inputs arrive":
                store([2 * src[b].reshape(-1) + 1 for b in range(P)])          # the right values, stored too early
                A.arrive()
            else:
                A.arrive()
                store(compute())
            return 0
        return call_deferred if deferred else call
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
                                          ("input modified", "input in, map 0, byte 1"),
                                          ("reads before the inputs arrive", "bytes differ from the oracle"),
                                          ("writes before the inputs arrive", "out depends on the prefill")])
def test_every_mistake_is_rejected(mistake, says):
    """the last two on an arena whose inputs arrive late: a stand-in that computes from the buffer before arrive() has
    read the decoys -- the same result under both seeds, and not the oracle's, which verify says --, one that stores
    before arrive() has its output overwritten by the prefill"""
    deferred = mistake.endswith("the inputs arrive")
    make, want = _standin(mistake, deferred)
    with pytest.raises(AssertionError) as e:
        outs, _ = arena.run_two_seeds(make, deferred=deferred)
        BC.bits_eq(outs["out"], want, "out")                        # verify, by the stand-in's own rule
    assert says in str(e.value) and "out" in str(e.value), str(e.value)


def test_a_correct_standin_passes_on_deferred_inputs():
    make, want = _standin(None, deferred=True)
    outs, _ = arena.run_two_seeds(make, deferred=True)
    BC.bits_eq(outs["out"], want, "out")


def test_deferred_layout():
    """the two images: the decoy image is the seed's pattern plus a decoy of every input inside its domain (uint8 / float
    reversed in flat order, int32 the tensor's minimum, strided maps and gaps as in the true image); arrive() makes the
    whole buffer the true image, which is what build() makes without `deferred`; check() and initial() mean the true one"""
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    f32 = rng.random((P, H, W), dtype=np.float32)
    i32 = rng.integers(2, 9, (4, 6)).astype(np.int32)
    f64 = rng.random((3, 3))
    for seed in arena.SEEDS:
        def declare(A):
            A.inp("u8", u8); A.inout("f32", f32, stride=STRIDE); A.inp("i32", i32); A.inp("f64", f64)
            A.inp("one", np.array([7], np.int32)); A.inp("flat", np.full((2, 3), 4, np.uint8)); A.out("out", (2, 2), np.float32)
            return A
        plain = declare(arena.Arena(seed)).build()
        A = declare(arena.Arena(seed)).build(deferred=True)
        assert sorted(A.decoyed()) == ["f32", "f64", "i32", "u8"] and plain.decoyed() == []
        assert np.array_equal(A._init, plain.buf) and A.nbytes == plain.nbytes
        pat = arena.pattern(A.nbytes, seed)
        inside = np.zeros(A.nbytes, bool)
        for t in A._t.values():
            for off, nb in A._maps(t):
                inside[off:off + nb] = t.data is not None
        assert np.array_equal(A.buf[~inside], pat[~inside]), "pattern outside the inputs, gaps and outputs included"
        assert np.array_equal(A._read("u8", A.buf), u8.reshape(-1)[::-1].reshape(u8.shape))
        assert np.array_equal(A._read("f32", A.buf), f32.reshape(-1)[::-1].reshape(f32.shape))
        assert np.array_equal(A._read("f64", A.buf), f64.reshape(-1)[::-1].reshape(f64.shape))
        assert (A._read("i32", A.buf) == i32.min()).all() and A._read("one", A.buf)[0] == 7
        assert np.array_equal(A.initial("u8"), u8) and np.array_equal(A.initial("i32"), i32)
        with pytest.raises(AssertionError, match="input u8"):
            A.check()                                               # the decoys are not what the inputs were
        A.arrive()
        assert np.array_equal(A.buf, plain.buf)
        A.check()
        snap = A.buf.copy()
        A.buf[A.addr("out") - A.base - 1] ^= 1
        A.check(snap)                                               # check reads the buffer it is given
        with pytest.raises(AssertionError, match="front guard of out"):
            A.check()
        K = declare(arena.Arena(seed)).build(deferred=True, keep=("i32",))
        assert sorted(K.decoyed()) == ["f32", "f64", "u8"] and np.array_equal(K._read("i32", K.buf), i32)


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


def _comment_before(text, name):
    """the last comment of include/smt.h in front of the declaration of `name` (a comment may serve several declarations)"""
    m = re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group()), text, flags=re.S))
    assert m, name
    start = text.rfind("\n/*", 0, m.start())                     # a comment of its own, not one behind a declaration
    return text[start:text.find("*/", start)]


def test_every_caller_buffer_entry_is_decided_synchronising_or_not():
    """SYNCHRONISING holds one decision per name of REQUIRED, and the header says the same: the comment of an entry
    decided SYNC ends with the sentence "Synchronising.", no comment of an entry decided ASYNC holds it"""
    text = open(os.path.join(ROOT, "include", "smt.h")).read()
    decided = {n for _, n, _, _ in SC.cases()}                     # every device entry of the bounds table
    assert set(SC.SYNCHRONISING) == decided >= set(BC.REQUIRED), sorted(set(SC.SYNCHRONISING) ^ decided)
    for name, decision in SC.SYNCHRONISING.items():
        assert decision in (SC.ASYNC, SC.SYNC, SC.ASYNC_WARM), (name, decision)
        comment = " ".join(_comment_before(text, name).replace("*", " ").split())
        says = comment.endswith(SC.SYNC)
        assert says == (decision == SC.SYNC), f"{name}: decided {decision!r}, the header's comment {'ends' if says else 'does not end'} with {SC.SYNC!r}"
        assert (SC.ASYNC_WARM in comment) == (decision == SC.ASYNC_WARM), f"{name}: decided {decision!r}"
    assert sorted(n for n, d in SC.SYNCHRONISING.items() if d == SC.SYNC) == [
        "smt_adcensus_option_aggregate", "smt_fill_the_hole", "smt_remove_speckles"]


def test_every_input_of_the_table_has_a_decoy_or_a_reason(X):
    """every case of the stream-order table, declared on a host arena: at least one input differs from its decoy; every
    entry with an int32 input that is decoyed is in INT32_DECOY with the reason its minimum is admissible; NO_DECOY names
    tensors that exist, with reasons"""
    cases = SC.cases()
    assert {n for _, n, _, _ in cases} == set(BC.ENTRIES) - set(BC.HOST_ENTRIES) >= set(BC.REQUIRED) | {"smt_ncc_flow_run_batch"}
    assert len({i for i, *_ in cases}) == len(cases)
    for want in ({"SMT_OVERLAP": v} for v in "012"):
        assert sum(e == want for _, n, _, e in cases if n == "smt_adcensus_compute_batch") == len(BC.CASES["smt_adcensus_compute_batch"])
    for n in ("smt_pipeline_run_batch", "smt_pipeline_run_batch_post"):
        for v in "012":
            ps = [p["P"] for _, m, p, e in cases if m == n and e == {"SMT_PIPE_SCHEDULE": v}]
            assert len(ps) == len(BC.CASES[n]) + (v == "2") and (5 in ps) == (v == "2"), (n, v, ps)
    with_int32 = set()
    for cid, name, params, _ in cases:
        A = arena.Arena(arena.SEEDS[1])
        BC.ENTRIES[name](A, X, **params)
        keep = SC.NO_DECOY.get(name, {})
        assert set(keep) <= {t.name for t in A._t.values() if t.data is not None}, cid
        A.build(deferred=True, keep=tuple(keep), decoys=SC.own_decoys(name, A))
        assert A.decoyed(), f"{cid}: no input differs from its decoy"
        if any(A._t[n].dtype == np.int32 for n in A.decoyed()):
            with_int32.add(name)
    assert with_int32 == set(SC.INT32_DECOY), sorted(with_int32 ^ set(SC.INT32_DECOY))
    assert all(isinstance(r, str) and r for r in SC.INT32_DECOY.values())
    assert all(isinstance(r, str) and r for d in SC.NO_DECOY.values() for r in d.values())
