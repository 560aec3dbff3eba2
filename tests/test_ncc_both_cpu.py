"""Both-view NCC (smt_lrncc, smt_lrncc_flow_run_batch) without a GPU: the exports are declared as the header states and
exported, the Python names exist, the rank key reproduces WinTakeAll's sequential rule on hostile rows
(smt_lrncc_selftest_keys), a NumPy restatement of the right view's definition equals the mirrored oracle call, and the
inputs whose right maps the GPU tests hold to the oracle have no near-ties.

Near-ties.  The oracle sums in float64 (loop nest), the integer kernels round four times: two evaluations differ by at
most b = exact_matchers.ncc_forms_bound(win) per cost.  If at a pixel the best cost exceeds every other by more than
g = 2 b + 2^-23 (two float32 half-ulps of values up to 1 on top of the two evaluation errors), WinTakeAll's outcome is that
hypothesis under both: it beats the narrowed maximum of everything before it, and nothing after it beats its narrowed
value.  Pixels with sentinel hypotheses (the first sentinel wins whatever the costs) and pixels whose d = 0 cost is NaN
(the map is 0; the NaN pattern is an integer statement) do not depend on the costs at all."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds_cases as BC  # noqa: E402
import exact_matchers as XM  # noqa: E402
import ncc_both_cases as LC  # noqa: E402  (registers the bounds and stream-order rows of the new exports)
import stream_order_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "smt_lrncc": "const uint8_t *L, const uint8_t *R, int H, int W, int D, int winSize, int32_t *dispL, int32_t *dispR, "
                 "double *costL, double *costR, void *stream",
    "smt_lrncc_flow_run_batch": "smt_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *dispL, "
                                "int32_t *dispR, int32_t *lastdisp, uint8_t *cls",
    "smt_lrncc_set_impl": "int impl",
    "smt_lrncc_last_form": "void",
    "smt_lrncc_selftest_keys": "int W, int D, int winSize, unsigned seed",
}


def _lib():
    from stereo_match_traditional_amd import build
    return ctypes.CDLL(build.build())


def test_new_symbols_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smt.h")).read(), flags=re.S)
    lib = _lib()
    assert set(re.findall(r"\b(smt_lrncc\w*)\s*\(", hdr)) == set(DECLARED)
    for name, params in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        assert " ".join(m.group(1).split()) == params, name
        assert hasattr(lib, name), name
        assert (name in BC.ENTRIES) != (name in BC.NOT_CALLER_BUFFER), name
    for k, v in (("SMT_LRNCC_FORM_COMPOSED", 1), ("SMT_LRNCC_FORM_KEYS", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (k, v), hdr), k
    assert SC.SYNCHRONISING["smt_lrncc"] == SC.ASYNC and SC.SYNCHRONISING["smt_lrncc_flow_run_batch"] == SC.ASYNC_WARM
    assert {n for _, n, _, _ in SC.cases()} >= {"smt_lrncc", "smt_lrncc_flow_run_batch"}


def test_the_cases_cover_every_kernel_and_form():
    kernels = {(p["impl"], (p["D"] + 63) // 64, p["lr"]) for p in LC.LRNCC_CASES if LC.expected_form(p["H"], p["W"], p["win"], p["impl"], p["lr"])}
    for impl in (2, 3):                                        # every box instantiation and dot4 slot counts 1, 2, 4, 5 under KEYS
        assert {k for i, k, m in kernels if i == impl and m == 2} >= {1, 2, 4, 5}
    assert any(i == 1 for i, _, _ in kernels) and any(m == 1 for _, _, m in kernels)
    assert any(LC.expected_form(p["H"], p["W"], p["win"], p["impl"], p["lr"]) is None for p in LC.LRNCC_CASES)
    assert any(p["W"] < p["D"] for p in LC.LRNCC_CASES) and any(p["win"] == 0 for p in LC.LRNCC_CASES)
    assert {p["form"] for p in LC.FLOW_CASES} == {0, LC.LOOP, LC.DOT4, LC.BOX}
    assert {p["outs"] for p in LC.FLOW_CASES} >= {LC.OUTS, ("dispR",), ("lastdisp",), ("cls",)}


def test_python_layer_has_the_new_names():
    from stereo_match_traditional_amd import _lib as L, api, shard
    assert (L.LRNCC_FORM_COMPOSED, L.LRNCC_FORM_KEYS) == (1, 2)
    for name in ("NCC_both", "lrncc_set_impl", "lrncc_last_form", "LRNCC_FORM_COMPOSED", "LRNCC_FORM_KEYS"):
        assert hasattr(api, name) and name in api.__all__, name
    assert callable(api.NCCFlow.run_both) and callable(shard.ncc_both_batch) and callable(shard.ncc_batch)
    lib = L.lib()
    assert len(lib.smt_lrncc.argtypes) == 11 and len(lib.smt_lrncc_flow_run_batch.argtypes) == 8


def test_hooks_and_rejections_without_a_device():
    lib = _lib()
    f = lib.smt_lrncc_set_impl
    try:
        assert f(1) == 0 and f(2) == 0 and f(0) == 0
        assert f(3) == -1 and f(-1) == -1
    finally:
        f(0)
    assert lib.smt_lrncc_flow_run_batch(None, None, None, 0, None, None, None, None) == -1
    one = ctypes.c_void_p(16)                                  # never dereferenced: the sizes are rejected first
    for H, W, D, win in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 513, 1), (4, 4, 4, -1)):
        assert lib.smt_lrncc(one, one, H, W, D, win, one, one, None, None, None) == -1
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert lib.smt_lrncc(args[0], args[1], 4, 4, 4, 1, args[2], args[3], None, None, None) == -1


# (W, D, winSize): one hypothesis, a wave, past a wave, D > 256, W < D, side 1, an interior of one column, none at all
KEY_ROWS = [(9, 1, 1), (40, 64, 1), (100, 65, 2), (30, 64, 3), (20, 300, 1), (300, 200, 0), (600, 512, 2), (9, 5, 4), (9, 5, 5),
            (12, 40, 0)]


@pytest.mark.parametrize("W,D,win", KEY_ROWS)
def test_rank_keys_reproduce_wintakeall_on_hostile_rows(W, D, win):
    """seed % 4 selects the palette: exact ties; pairs that round down / up to one float; NaN at d = 0 and d > 0; a mix"""
    f = _lib().smt_lrncc_selftest_keys
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    for seed in range(16):
        assert f(W, D, win, seed) == 0, seed


def test_key_selftest_rejects_bad_sizes():
    f = _lib().smt_lrncc_selftest_keys
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    for bad in ((0, 4, 1), (4, 0, 1), (4, 513, 1), (4, 4, -1), ((1 << 16) + 1, 4, 1)):
        assert f(*bad, 0) == -1, bad


def test_the_rank_key_rule_in_numpy():
    """The rule the key encodes, restated: with f = float32(c) and F = max f, the winner is the LAST d with c[d] > F if
    any, else the FIRST d with f[d] == F -- equal to the sequential loop on rows of ties and of doubles around floats."""
    rng = np.random.default_rng(11)
    F = np.float32(0.7310586)
    pal = np.array([float(F), float(F) + 2.0 ** -40, float(F) - 2.0 ** -41, float(F) + 2.0 ** -39, 0.5, 0.5 + 2.0 ** -40, 0.25, -1.0])
    for _ in range(300):
        c = pal[rng.integers(0, len(pal), rng.integers(1, 12))]
        want = int(XM.ncc_wta(c[None, None, :], 0)[0, 0])
        f = c.astype(np.float32)
        top = f.max()
        down = np.flatnonzero(c > float(top))
        got = int(down[-1]) if down.size else int(np.flatnonzero(f == top)[0])
        assert got == want, c


def right_view_numpy(O, L, R, D, win):
    """The definition, literally: costR[i][x][d] = ComputeCost(R window at (i, x), L window at (i, x + d)) -- the
    oracle's own ComputeCost, reached as the d = 0 hypothesis of a call on R and L shifted left by d -- while
    x + win + d <= W - 1, 255.0 beyond; dispR = WinTakeAll of the row; border 0 / 0.0."""
    H, W = L.shape
    cost = np.zeros((H, W, D))
    inner = (slice(win, H - win), slice(win, W - win))
    cost[inner] = 255.0
    for d in range(min(D, W - 2 * win)):
        Ls = np.ascontiguousarray(L[:, d:])                    # column x of Ls is column x + d of L
        _, c0 = O.ncc(np.ascontiguousarray(R[:, :W - d]), Ls, 1, win, want_cost=True)
        cost[win:H - win, win:W - d - win, d] = c0[win:H - win, win:W - d - win, 0]
    return XM.ncc_wta(cost, win), cost


@pytest.mark.parametrize("H,W,D,win", [(5, 19, 8, 1), (7, 12, 20, 2), (4, 30, 6, 0), (3, 15, 5, 1), (9, 25, 30, 3)])
def test_definition_equals_the_mirrored_oracle_call(O, H, W, D, win):
    """shapes: win 0, W < D, one interior row"""
    L, R = LC.pair(H, W, 77)
    disp, cost = right_view_numpy(O, L, R, D, win)
    md, mc = O.ncc(LC.flip(R), LC.flip(L), D, win, want_cost=True)
    mc = np.ascontiguousarray(mc[:, ::-1])
    inner = np.zeros((H, W), bool)
    inner[win:H - win, win:W - win] = True
    # the same windows in the same order of summation up to the flip: a flipped window sums the same bytes in another
    # order, so the costs agree within the oracle's own pair bound, the sentinels and NaNs exactly
    assert np.array_equal(np.isnan(cost[inner]), np.isnan(mc[inner]))
    assert np.array_equal(cost[inner] == 255.0, mc[inner] == 255.0)
    ok = inner[:, :, None] & ~np.isnan(cost)
    assert np.abs(cost[ok] - mc[ok]).max(initial=0.0) <= XM.ncc_pair_bound(win)
    x = np.arange(W)[None, :, None]
    assert np.array_equal((cost == 255.0) & inner[:, :, None], (x + win + np.arange(D)[None, None, :] > W - 1) & inner[:, :, None])
    if win > 0:                                                # (side 1: every cost NaN, both maps 0)
        assert no_near_ties(mc, win), "the shapes of this test must not hide a tie"
    assert np.array_equal(disp, LC.flip(md))


def no_near_ties(cost, win):
    """cost: a right-view volume [H][W][D] (float64, the oracle's).  True when every interior pixel that depends on its
    costs at all (no sentinel hypothesis, d = 0 not NaN) has a best cost more than g above every other."""
    H, W, D = cost.shape
    g = 2 * XM.ncc_forms_bound(win) + 2.0 ** -23
    c = cost[win:H - win, win:W - win]
    free = ~(c == 255.0).any(-1) & ~np.isnan(c[..., 0])
    if D == 1 or not free.any():
        return True
    s = np.sort(np.where(np.isnan(c[free]), -np.inf, c[free]), axis=-1)
    return bool((s[:, -1] - s[:, -2] > g).all())


_ALL = list({(n, p["H"], p["W"], p["D"], p["win"]): (n, p) for n, ps in (("smt_lrncc", LC.LRNCC_CASES), ("smt_lrncc_flow_run_batch", LC.FLOW_CASES))
             for p in ps}.values())                            # one case per entry and shape: the images depend on nothing else


@pytest.mark.parametrize("name,p", _ALL, ids=[f"{n}-{BC.case_id(p)}" for n, p in _ALL])
def test_oracle_map_inputs_have_no_near_ties(O, name, p):
    """every image pair whose maps the GPU tests compare with the oracle's (the shapes of the two case lists, whatever the
    form), in both views"""
    H, W, D, win = p["H"], p["W"], p["D"], p["win"]
    if H <= 2 * win or W <= 2 * win:
        return
    for L, R in LC.case_pairs(name, p):
        _, cl = O.ncc(L, R, D, win, want_cost=True)
        _, cr = O.ncc(LC.flip(R), LC.flip(L), D, win, want_cost=True)
        assert no_near_ties(cl, win) and no_near_ties(cr, win)


def test_the_shapes_of_the_lists_are_all_checked():
    seen = {(n, p["H"], p["W"], p["D"], p["win"]) for n, p in _ALL}
    assert seen == {("smt_lrncc", p["H"], p["W"], p["D"], p["win"]) for p in LC.LRNCC_CASES} | \
        {("smt_lrncc_flow_run_batch", p["H"], p["W"], p["D"], p["win"]) for p in LC.FLOW_CASES}
