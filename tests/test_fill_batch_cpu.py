"""smt_fill_the_hole_batch without a GPU: its host twin smt_fill_the_hole_batch_host runs the same rule text
(csrc/fill_rules.h: target derivation from cls, winner gather, angle-set choice, pick, pass-2 gating, flags) on host
memory and is held, bit for bit, to the oracle's FillTheHole fed with the lists of the same class map.  The oracle is
pinned to PostProcessing.h's own compiled code by tests/test_ref_pin_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fill_batch_cases as fc  # noqa: E402
from fill_batch_cases import bits  # noqa: E402

SMT_OK, SMT_ERR_ARG = 0, -1


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd import build
    L = C.CDLL(build.build())
    L.smt_fill_the_hole_batch_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                               C.c_int, C.c_int, C.c_void_p]
    L.smt_fill_the_hole_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p]
    return L


def host_batch(lib, maps, clss, D, pad_d=0, pad_c=0):
    """Runs the host twin on a batch laid out `pad` elements apart -> (maps afterwards, status [pairs][4])."""
    P, (row, col) = len(maps), maps[0].shape
    n = row * col
    dbuf = np.full((P, n + pad_d), 12345.0, np.float32)
    cbuf = np.full((P, n + pad_c), 1, np.uint8)                   # class 1 in the padding: must never be read as a target
    for b in range(P):
        dbuf[b, :n] = maps[b].reshape(-1)
        cbuf[b, :n] = clss[b].reshape(-1)
    status = np.full((P, 4), -77, np.int32)
    rc = lib.smt_fill_the_hole_batch_host(dbuf.ctypes.data, cbuf.ctypes.data, P, n + pad_d if pad_d else 0,
                                          n + pad_c if pad_c else 0, row, col, D, status.ctypes.data)
    assert rc == SMT_OK
    assert (dbuf[:, n:] == 12345.0).all(), "wrote into the padding between maps"
    return [dbuf[b, :n].reshape(row, col).copy() for b in range(P)], status


def check_pair(lib, O, d, cls, D, tag):
    ref, st, third = fc.expected(O, d, cls, D)
    (got,), status = host_batch(lib, [d], [cls], D)
    print(tag, "status", status[0].tolist(), "expected", st, "aliased", fc.aliased(cls), "mids", fc.mids(cls, third),
          "differing", int((bits(got) != bits(ref)).sum()))
    assert status[0].tolist() == st, tag
    assert np.array_equal(bits(got), bits(ref)), tag
    return st, third


@pytest.mark.parametrize("row,col,D", fc.SHAPES)
def test_single_pairs_match_the_oracle(lib, O, row, col, D):
    d, cls = fc.lr_case(O, row, col, row * 7 + col)
    st, third = check_pair(lib, O, d, cls, D, (row, col, D))
    if col > row > 1:                                                        # one row: every address has one candidate
        assert fc.aliased(cls) > 0, "a landscape LR map without aliased entries"


def test_the_shapes_stay_inside_defined_behaviour_and_cover_the_angle_rule(O):
    """On every shape the oracle does not raise and the third pass's hole count stays below the mismatch count; over
    the set (the three constructed middle-row cases included) the rows-alone cases of the angle rule all occur."""
    seen = set()
    cases = [fc.lr_case(O, r, c, r * 7 + c) + (D,) for r, c, D in fc.SHAPES] + [fc.mid_case(O, w) for w in (0, 1, 2)]
    for d, cls, D in cases:
        row, col = cls.shape
        _, st, third = fc.expected(O, d, cls, D)
        assert st[2] <= st[1]
        m0, m1, m2 = fc.mids(cls, third)
        if col // 2 >= row:
            seen.add("no middle row")
        if m0:
            seen.add("switch in pass 0 persists")
        if not m0 and m1:
            seen.add("switch in pass 1")
        if not m0 and not m1 and m2:
            seen.add("switch in pass 2 only")
    assert seen == {"no middle row", "switch in pass 0 persists", "switch in pass 1", "switch in pass 2 only"}, seen


@pytest.mark.parametrize("which", [0, 1, 2])
def test_middle_row_in_one_list_only(lib, O, which):
    d, cls, D = fc.mid_case(O, which)
    st, third = check_pair(lib, O, d, cls, D, ("mid", which))
    m0, m1, m2 = fc.mids(cls, third)
    assert (m0, m1) == [(True, False), (False, True), (False, False)][which]
    if which == 2:
        assert m2


@pytest.mark.parametrize("row,col,D", [(37, 61, 32), (50, 70, 24)])
def test_batches_with_strides(lib, O, row, col, D):
    maps, clss = fc.batch_of_five(O, row, col, 300 + row)
    got, status = host_batch(lib, maps, clss, D, pad_d=37, pad_c=5)
    for b in range(5):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        (single,), s1 = host_batch(lib, [maps[b]], [clss[b]], D)
        assert status[b].tolist() == st == s1[0].tolist(), b
        assert np.array_equal(bits(got[b]), bits(ref)) and np.array_equal(bits(single), bits(ref)), b
    assert np.array_equal(bits(got[3]), bits(maps[3])) and status[3].tolist() == [0, 0, -1, 0]
    assert status[4, 1] == 0 and status[4, 2] == -1 and status[4, 0] > 0
    assert (got[4] == fc.HOLE).sum() > 0, "the holes of the pair without mismatches must survive"
    # the status pointer may be NULL
    P, n = 5, row * col
    dbuf = np.ascontiguousarray(np.stack(maps))
    cbuf = np.ascontiguousarray(np.stack(clss))
    assert lib.smt_fill_the_hole_batch_host(dbuf.ctypes.data, cbuf.ctypes.data, P, 0, 0, row, col, D, None) == SMT_OK
    assert np.array_equal(bits(dbuf), bits(np.stack(got)))


def test_list_entries_outside_the_buffer_flag_the_pair_and_leave_it_alone(lib, O):
    maps, clss, D = fc.portrait_batch(O)
    got, status = host_batch(lib, maps, clss, D, pad_d=11)
    occ, mis = fc.lists(clss[1])
    with pytest.raises(ValueError):
        O.fill_the_hole(maps[1], D, occ, mis)
    assert status[1].tolist() == [len(occ), len(mis), -1, fc.UB_LIST]
    assert np.array_equal(bits(got[1]), bits(maps[1])), "a flagged pair must not be modified"
    for b in (0, 2):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        assert status[b].tolist() == st and np.array_equal(bits(got[b]), bits(ref)), b


def test_more_holes_than_mismatches_applies_passes_0_and_1_only(lib, O):
    maps, clss, D = fc.third_overrun_batch(O)
    got, status = host_batch(lib, maps, clss, D)
    fc.check_third_overrun(O, maps[1], clss[1], D, got[1], status[1])
    for b in (0, 2):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        assert status[b].tolist() == st and np.array_equal(bits(got[b]), bits(ref)), b


def test_full_size_maps(lib, O):
    """1920 x 1080, D = 192: the oracle's LR check, one pair as it comes and one with a seeded 2 % of 65535."""
    row, col, D = fc.FULL
    for b in (0, 2):
        dL, dR, rng = fc.full_size_inputs(b)
        d, cls, _, _ = O.lrcheck(dL, dR, 2)
        if b >= 2:
            d[rng.random((row, col)) < 0.02] = fc.HOLE
        st, third = check_pair(lib, O, d, cls, D, ("full size", b))
        assert fc.aliased(cls) > 10000 and (st[2] > 0) == (b >= 2)


def test_other_class_values_are_not_targets(lib, O):
    d, cls = fc.lr_case(O, 37, 61, 77)
    noisy = cls.copy()
    noisy[(cls == 0) & (np.random.default_rng(5).random(cls.shape) < 0.2)] = 3
    noisy[0, 0] = 255 if cls[0, 0] == 0 else cls[0, 0]
    (a,), sa = host_batch(lib, [d], [cls], 32)
    (b,), sb = host_batch(lib, [d], [noisy], 32)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_argument_errors(lib, entry):
    fake_d, fake_c = C.c_void_p(4096), C.c_void_p(1 << 20)                    # never dereferenced: the checks come first
    ok = dict(disp=fake_d, cls=fake_c, pairs=2, ds=0, cs=0, row=48, col=64, D=16)

    def call(**kw):
        a = dict(ok, **kw)
        args = (a["disp"], a["cls"], a["pairs"], a["ds"], a["cs"], a["row"], a["col"], a["D"], None)
        if entry == "device":
            return lib.smt_fill_the_hole_batch(*args, None)
        return lib.smt_fill_the_hole_batch_host(*args)

    assert call(disp=None) == SMT_ERR_ARG and call(cls=None) == SMT_ERR_ARG
    assert call(pairs=-1) == SMT_ERR_ARG
    for row, col in ((0, 64), (48, 0), (-1, 64), (48, -5)):
        assert call(row=row, col=col) == SMT_ERR_ARG
    assert call(D=-1) == SMT_ERR_ARG
    assert call(row=32768, col=65536) == SMT_ERR_ARG                          # row*col = 2^31
    assert call(row=65536, col=65536) == SMT_ERR_ARG
    for s in (1, 48 * 64 - 1):
        assert call(ds=s) == SMT_ERR_ARG and call(cs=s) == SMT_ERR_ARG
    assert call(pairs=0) == SMT_OK                                            # a no-op: nothing is touched
    assert call(pairs=0, disp=None) == SMT_ERR_ARG


def test_is_declared_with_its_flags():
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    for name in ("smt_fill_the_hole_batch(", "smt_fill_the_hole_batch_host(", "#define SMT_FILL_UB_LIST 1",
                 "#define SMT_FILL_UB_THIRD 2"):
        assert name in hdr, name
