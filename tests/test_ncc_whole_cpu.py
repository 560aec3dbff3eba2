"""NCC.h's whole-image ncc() where there is no device: the fixture against the reference (regenerated when the reference
tree is present), the NumPy restatements of tests/ncc_whole_cases.py against the fixture and against each other, the exact
form against fractions.Fraction, the host selftest of the INT kernel's recurrences, the argument rules, and the winner rule
split into runs of offsets (how the kernels split them over workgroups) against the sequential rule on hostile rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import ncc_whole_cases as WC  # noqa: E402
import make_ncc_whole_golden as MG  # noqa: E402

SMT_ERR_ARG, SMT_ERR_REF_UB = -1, -5
K, O = 5, 79                                              # what the reference fixes (NCC.h:121-122)


@pytest.fixture(scope="module")
def FX():
    return dict(np.load(MG.OUT))


@pytest.fixture(scope="module")
def REFS():
    """{(name, view): (loops cost, loops offsets, int cost, int offsets, exact, flat)} of the six pairs, computed once"""
    out = {}
    for name, L, R in WC.fixture_pairs():
        for view in (WC.VL, WC.VR):
            out[name, view] = WC.ref_loops(L, R, K, O, view) + WC.ref_int(L, R, K, O, view) + WC.exact_ld(L, R, K, O, view)
    return out


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd._lib import lib
    return lib()


def test_fixture_holds_exactly_the_recorded_names(FX):
    names = {f"{n}_{m}" for n, _, _ in WC.fixture_pairs() for m in ("left", "right")} | {"grey"}
    assert set(FX) == names and len(names) == 13
    assert os.path.getsize(MG.OUT) < 64 * 1024


def test_fixture_regenerates_from_the_reference(FX):
    got = MG.record(MG.DEFAULT_REFERENCE)
    if got is None:
        pytest.skip("the reference tree is not on this machine")
    assert set(got) == set(FX)
    for name in FX:
        assert np.array_equal(got[name], FX[name]), name


@pytest.mark.parametrize("view,mode", [(WC.VL, "left"), (WC.VR, "right")])
def test_loop_restatement_equals_the_fixture(FX, REFS, view, mode):
    for name, L, R in WC.fixture_pairs():
        off = REFS[name, view][1]
        assert np.array_equal((3 * off).astype(np.uint8), FX[f"{name}_{mode}"]), name


@pytest.mark.parametrize("view,mode", [(WC.VL, "left"), (WC.VR, "right")])
def test_integer_form(FX, REFS, view, mode):
    """the three checks: the map equals the fixture (under the excuse rule, which the six pairs do not need), the costs lie
    within the derived bound of the exact rational function, and the NaN pattern is the loop nest's and {Ai Bi == 0}"""
    worst = 0.0
    for name, L, R in WC.fixture_pairs():
        lc, loff, ic, ioff, exact, flat = REFS[name, view]
        assert np.array_equal(np.isnan(ic), np.isnan(lc))
        worst = max(worst, WC.check_costs(ic, exact, flat, WC.INT, K))
        WC.check_costs(lc, exact, flat, WC.LOOP, K)
        need = WC.excused(ioff, loff, exact, WC.bound_of(WC.INT, exact, K), WC.bound_of(WC.LOOP, exact, K))
        assert need == 0, f"{name}: {need} pixels needed the excuse (none did when the fixture was made)"
        assert np.array_equal((3 * ioff).astype(np.uint8), FX[f"{name}_{mode}"]), name
        assert (ioff[flat.all(axis=2)] == 0).all() and flat.all(axis=2).sum() == (ioff == 0).sum()
    print(f"integer form, view {mode}: largest error {worst:.3f} bounds")
    assert 0 < worst <= 1


def test_patches_pairs_hold_what_they_promise(REFS):
    """all-NaN pixels, and constant windows that score the maximum 1 / n exactly"""
    for (name, view), (lc, loff, ic, ioff, exact, flat) in REFS.items():
        if "patches" not in name:
            continue
        H, W = ioff.shape
        h, w = WC.extents(H, W, K)
        assert flat.all(axis=2).sum() >= 50
        inv_n = (1.0 / ((h - 1) * (w - 1)))[:, :, None].repeat(O, 2)
        top = np.abs(exact - 1 / ((h - 1) * (w - 1)).astype(WC.LD)[:, :, None]) <= WC.bound_int(exact)
        assert (top & ~flat).sum() >= 50, "no window scores 1 / n"
        assert (np.abs(ic[~flat]) <= inv_n[~flat] * (1 + 2.0 ** -50)).all(), "|res| <= 1 / n"


def test_exact_form_against_fractions(REFS):
    rng = np.random.default_rng(5)
    pairs = {n: (L, R) for n, L, R in WC.fixture_pairs()}
    checked = 0
    for (name, view), (_, _, _, _, exact, flat) in REFS.items():
        L, R = pairs[name]
        H, W = L.shape
        for _ in range(25):
            y, x, o = int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(1, O + 1))
            fr = WC.exact_fraction(L, R, K, O, view, y, x, o)
            assert (fr is None) == bool(flat[y, x, o - 1])
            if fr is None:
                continue
            import exact_matchers as XM
            assert XM.fraction_rel_err(exact[y, x, o - 1], fr) <= 2.0 ** -60
            checked += 1
    assert checked > 200


def test_symmetry_identity_of_the_integer_form(REFS):
    """left cost at (y, x, o) == right cost at (y, x - o, o), word for word, wherever x - k >= o and x + k <= W - 1"""
    words = 0
    for name, L, R in WC.fixture_pairs():
        cl, cr = REFS[name, WC.VL][2], REFS[name, WC.VR][2]
        W = L.shape[1]
        for o in range(1, O + 1):
            xs = np.arange(max(o + K, 0), W - K)
            if len(xs) == 0:
                continue
            a, b = cl[:, xs, o - 1], cr[:, xs - o, o - 1]
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), (name, o)
            words += a.size
    assert words > 40000


@pytest.mark.parametrize("H,W,k,o", WC.SHAPES + [(9, 83, 5, 79), (3, 80, 35, 3), (12, 300, 7, 9)])
def test_selftest_box(lib, H, W, k, o):
    for view in (WC.VL, WC.VR):
        assert lib.smt_whole_ncc_selftest_box(H, W, k, o, view, 7 + H + W) == 0, (H, W, k, o, view)


def test_argument_rules(lib):
    st = lib.smt_whole_ncc_selftest_box
    assert st(1, 10, 2, 3, WC.VL, 1) == SMT_ERR_ARG           # H < 2: a one-row window, n = 0
    assert st(4, 1, 2, 1, WC.VL, 1) == SMT_ERR_ARG            # W < 2
    assert st(4, 10, 0, 3, WC.VL, 1) == SMT_ERR_ARG           # kernel_size < 1
    assert st(4, 10, 2, 0, WC.VL, 1) == SMT_ERR_ARG           # max_offset < 1
    assert st(4, 10, 2, 3, 3, 1) == SMT_ERR_ARG               # a view that is neither left nor right
    assert st(4, 10, 2, 11, WC.VL, 1) == SMT_ERR_REF_UB       # max_offset > W: the shift loops leave tmp
    assert st(4, 10, 2, 10, WC.VR, 1) == 0                    # max_offset == W is defined
    assert st(3, 80, 36, 3, WC.VL, 1) == SMT_ERR_ARG          # beyond the integer limit there is no INT kernel
    assert st(2, 600, 2, 513, WC.VL, 1) == SMT_ERR_ARG        # SMT_MAX_DISPARITY
    from stereo_match_traditional_amd import _lib
    p = _lib.NCCWholeParams()
    lib.smt_whole_ncc_default_params(C.byref(p))
    assert (p.kernel_size, p.max_offset, p.add_constant) == (5, 79, 0)
    for impl in (-1, 3):
        assert lib.smt_whole_ncc_set_impl(impl) == SMT_ERR_ARG
    assert lib.smt_whole_ncc_set_impl(0) == 0
    assert lib.smt_whole_ncc_set_groups(-1) == SMT_ERR_ARG and lib.smt_whole_ncc_set_groups(0) == 0
    # the caller-buffer entries reject before anything is launched (no device here)
    buf = (C.c_uint8 * 64)()
    for H, W, k, o, view, want in ((1, 10, 2, 3, 1, SMT_ERR_ARG), (4, 10, 0, 3, 1, SMT_ERR_ARG), (4, 10, 2, 3, 0, SMT_ERR_ARG),
                                   (4, 10, 2, 11, 2, SMT_ERR_REF_UB), (4, 10, 2, 600, 1, SMT_ERR_ARG)):
        p.kernel_size, p.max_offset = k, o
        assert lib.smt_whole_ncc(buf, buf, H, W, C.byref(p), view, buf, None, None, None) == want, (H, W, k, o, view)
    p.kernel_size, p.max_offset = 2, 3
    assert lib.smt_whole_ncc(None, buf, 4, 10, C.byref(p), 1, buf, None, None, None) == SMT_ERR_ARG
    assert lib.smt_whole_ncc(buf, buf, 4, 10, C.byref(p), 1, None, None, None, None) == SMT_ERR_ARG
    assert lib.smt_bgr_to_grey_batch(buf, -1, 2, 2, buf, None) == SMT_ERR_ARG
    assert lib.smt_bgr_to_grey_batch(None, 0, 2, 2, None, None) == 0
    assert lib.smt_whole_ncc_flow_run_batch(None, buf, buf, 1, buf, None, None, None, None, None) == SMT_ERR_ARG


def _sequential(row):
    best, off = -2.0, 0
    for o, c in enumerate(row, 1):
        if c > best:
            best, off = c, o
    return off


def _in_runs(row, G):
    """the kernels' rule: G consecutive runs of ceil(O / G) offsets, each with the reference's statement from (-2.0, 0),
    then the runs' winners in their order under the same statement"""
    O_ = len(row)
    per = -(-O_ // G)
    best, off = -2.0, 0
    for g in range(G):
        b, f = -2.0, 0
        for o in range(1 + g * per, min(O_, (g + 1) * per) + 1):
            if row[o - 1] > b:
                b, f = row[o - 1], o
        if b > best:
            best, off = b, f
    return off


def test_winner_rule_in_runs_on_hostile_rows():
    """the rule as a statement of its own, beside the C helpers: smt_whole_ncc_selftest_box (test_selftest_box) holds the
    kernels' nw_group and nw_offer to the sequential loop for every G, and tests/test_ncc_whole_gpu.py runs the kernels
    over runs of several offsets.  Here: exact ties (the first stays), NaN first and later, all NaN, costs below the start value's reach (-2.0 is below every
    cost: |res| <= 1), and every split into runs"""
    nan = float("nan")
    rows = [[0.5, 0.5, 0.5], [nan, 0.25, 0.25, nan, 0.25], [0.25, nan, 0.5, 0.5, nan], [nan] * 7, [-1.0, -1.0, nan],
            [0.0, -0.0, 0.0], [nan, nan, -0.75], [1.0 / 3] * 9 + [np.nextafter(1.0 / 3, 1)] * 2 + [1.0 / 3]]
    rng = np.random.default_rng(3)
    palette = np.array([nan, -1.0, -0.5, 0.0, 0.125, 0.125, 0.5, 0.5, 1.0])
    rows += [list(palette[rng.integers(0, len(palette), n)]) for n in (1, 2, 5, 17, 79, 86) for _ in range(20)]
    for row in rows:
        want = _sequential(row)
        assert want == int(WC.winner(np.array(row).reshape(1, 1, -1))[0, 0])
        for G in range(1, len(row) + 1):
            assert _in_runs(row, G) == want, (row, G)
    assert _sequential([nan] * 4) == 0 and _sequential([0.5, nan, 0.5]) == 1


def test_bgr_to_grey_restatement_equals_the_fixture(FX):
    assert np.array_equal(WC.bgr_to_grey(WC.fixture_bgr()), FX["grey"])
    v = np.arange(256, dtype=np.uint8)
    full = WC.bgr_to_grey(np.stack([v, v, v], axis=-1)[None])
    assert full.max() == 3 * 84 and full[0, 255] == 252        # the three truncated thirds cannot wrap
