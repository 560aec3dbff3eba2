"""The method of the large-volume tests (large_volume_cases.py) proved on the oracle alone, at small sizes: for every
stage of the table the full oracle result of a block tiled K = 5 times has the claimed block structure and its first,
middle and last blocks are the sub-problem's; the faithful up / down identity and the composed scanline sum equal
O.scanline; the torch first-minimum equals O.wta with ties and NaNs; the table keeps its conditions; and the comparison
helpers reject planted defects."""
import numpy as np
import pytest
import torch

import exact_matchers as X
import large_volume_cases as LV

K, H0, W0 = 5, LV.H0, LV.W0
WS, D = 3 * W0, 16                                 # 13 x 33 blocks, D <= 16
H = K * H0


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_row_structure(full, three, edges_differ=True, what=""):
    """blocks 1 .. K-2 of the full result are one block; blocks 0, 1, K-1 are the sub-problem's; the edge blocks are not
    the middle one (the inputs reach the edge)"""
    b = full.reshape((K, H0) + full.shape[1:])
    for k in range(2, K - 1):
        assert same(b[k], b[1]), (what, "block", k)
    for name, got, want in zip(("top", "middle", "bottom"), (b[0], b[1], b[K - 1]), three):
        assert same(got, want), (what, name)
    if edges_differ:
        assert not same(b[0], b[1]) and not same(b[K - 1], b[1]), (what, "the edge blocks equal the middle one")


# ------------------------------------------------------------------------------------------------------------- the table
def test_ids_are_unique_and_every_stage_of_the_issue_is_there():
    ids = [c.id for c in LV.CASES]
    assert len(set(ids)) == len(ids)
    agg = [c for c in LV.CASES if c.stage == "agg"]
    for v in LV.VARIANTS:
        for o in (0, 1):
            assert any(c.regime == "A" and c.D == 256 and c.params == dict(variant=v, order=o) for c in agg), (v, o)
    assert any(c.regime == "A" and c.params["order"] == 2 for c in agg)
    assert any(c.regime == "A" and c.D % 64 for c in agg)
    assert {(c.params["variant"], c.params["order"]) for c in agg if c.regime == "B"} == {(13, 0), (13, 1), (6, 0), (6, 1)}
    assert {c.params["order"] for c in agg if c.regime == "C"} == {0, 1}
    adc = {c.params["mode"]: c for c in LV.CASES if c.stage == "adc" and c.D == 256}
    assert set(adc) == {"compute", "lent", "deferred"}
    assert any(c.stage == "adc" and c.D == 512 for c in LV.CASES)
    assert {c.D for c in LV.CASES if c.stage == "wta"} == {256, 250}
    assert {c.params["scan_pass"] for c in LV.CASES if c.stage == "scan_rows"} == {0, 1}
    assert {(c.params["scan_pass"], c.params["fixed"]) for c in LV.CASES if c.stage == "scan_cols"} == \
        {(2, False), (2, True), (3, False), (3, True)}
    assert sum(c.stage == "scan_run" for c in LV.CASES) == 1
    assert {c.params["view"] for c in LV.CASES if c.stage == "cblsm_ad"} == {0, 1}
    assert {(c.regime, c.params["impl"]) for c in LV.CASES if c.stage == "ncc"} == \
        {("ncc4", 2), ("ncc4", 3), ("ncc8", 2), ("ncc8", 3)}
    assert sum(c.stage == "sad" for c in LV.CASES) == 1


@pytest.mark.parametrize("c", LV.CASES, ids=[c.id for c in LV.CASES])
def test_case_keeps_the_tables_conditions(c):
    V = LV.elements(c)
    row = c.W * c.D
    # the regime's bounds
    if c.regime == "A":
        assert V * 4 < 1 << 32 and (V + c.h0 * row) * 4 >= 1 << 32, "A: the largest multiple of h0 rows under 2^32 bytes"
        assert V * 4 > 1 << 31, "A: byte offsets with the top bit set"
    elif c.regime == "B":
        assert V * 4 >= 1 << 32 and (V - c.h0 * row) * 4 < 1 << 32, "B: the smallest multiple of h0 rows at 2^32 bytes"
    elif c.regime == "C":
        assert V > 1 << 31 and V - c.h0 * row <= 1 << 31, "C: the smallest multiple of h0 rows above 2^31 elements"
    elif c.regime == "ncc4":
        assert c.itemsize == 8 and V > 1 << 29 and V - c.h0 * row <= 1 << 29
    else:
        assert c.regime == "ncc8" and c.itemsize == 8 and V > 1 << 30 and V - c.h0 * row <= 1 << 30
    # periodic axes
    assert c.H % c.h0 == 0 and c.H // c.h0 >= 5
    assert c.W % c.w0 == 0 and c.W // c.w0 >= 5
    # no aliasing: a wrap by a threshold does not land on the same place of another block ...
    for t in LV.THRESHOLDS:
        assert t % LV.period_elements(c) != 0, (t, "is a multiple of the period")
        assert t % (c.h0 * c.W * c.D) != 0 and t % (c.w0 * c.D) != 0
        # ... and each threshold below V falls strictly inside a row
        if t < V:
            assert t % row != 0, (t, "falls on a row boundary")
    assert c.W & (c.W - 1) != 0
    # the block reaches: the census window is 7 rows high, an aggregation block holds the longest vertical arm
    assert c.h0 >= 7 and c.h0 > 2 * LV.MAX_ARM
    # memory
    assert LV.device_bytes(c) >= c.volumes * V * c.itemsize + LV.EXTRA
    assert LV.device_bytes(c) + LV.HEADROOM <= LV.LIMIT, (LV.device_bytes(c) / LV.GiB, "GiB")
    assert LV.CHUNK <= LV.GiB // 2


def test_full_size_blocks_hold_different_values_in_every_row():
    """the builders at the blocks' full size: seeded noise, no two rows alike, no ramp"""
    blocks = [LV.cost_block((LV.H0, LV.W, 256), 1), LV.cost_block((LV.H0, LV.W, 250), 2, levels=64),
              LV.cost_block((LV.H0, LV.W0, 256), 3), LV.image_block(LV.H0, LV.W, 4), LV.image_block(LV.H0, LV.W, 5)]
    blocks += LV.arm_block(LV.H0, LV.W, 6)
    for b in blocks:
        assert LV.rows_differ(b) and not LV.is_ramp(b)
    assert same(LV.cost_block((3, 4, 5), 9), LV.cost_block((3, 4, 5), 9))           # seeded
    assert not same(LV.cost_block((3, 4, 5), 9), LV.cost_block((3, 4, 5), 10))
    g = LV.flat_guide(7, 2 * W0, W0, 1)
    assert (g.reshape(-1) == np.tile(g[0, :W0], 14)).all() and len(set(g[0, :W0].tolist())) > 1
    assert LV.is_ramp(np.arange(24.0).reshape(2, 3, 4)) and not LV.rows_differ(np.zeros((2, 5)))


def test_full_arms_stay_inside_the_plane():
    arms = LV.full_arms(LV.arm_block(H0, WS, 3), K)
    l, r, t, b = arms
    ii, jj = np.mgrid[0:H, 0:WS]
    assert (l <= jj).all() and (r <= WS - 1 - jj).all() and (t <= ii).all() and (b <= H - 1 - ii).all()
    assert max(int(a.max()) for a in arms) == LV.MAX_ARM and (l + r >= 1).all() and (t + b >= 1).all()
    for a in arms:                                       # periodic between the edge blocks
        blk = a.reshape(K, H0, WS)
        assert all(same(blk[k], blk[1]) for k in range(2, K - 1))
    assert not same(t[:H0], t[H0:2 * H0]) and not same(b[-H0:], b[H0:2 * H0])


def test_image_sizes_beyond_int_pixel_indices_are_rejected_without_a_gpu():
    """include/smt.h, "Limits": H * W < 2^31 on every entry point of the table whose pixel indices are int, and the grid
    size of the one-thread-per-hypothesis helpers.  The checks come before any device work."""
    import ctypes as C
    from stereo_match_traditional_amd._lib import SMT_ERR_ARG, lib
    l = lib()
    a, b, c, d = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))          # never dereferenced
    h = C.c_void_p()
    for H, W in ((32768, 65536), (65536, 65536)):                        # 2^31, 2^32
        assert l.smt_wta(a, H, W, 64, b, None) == SMT_ERR_ARG
        assert l.smt_ncc(a, b, H, W, 64, 1, c, None, None) == SMT_ERR_ARG
        assert l.smt_crossarm_create(H, W, 64, None, C.byref(h)) == SMT_ERR_ARG and not h.value
        assert l.smt_scanline_create(H, W, 64, 10, 150, C.byref(h)) == SMT_ERR_ARG and not h.value
        assert l.smt_adcensus_create_ex(-1, H, W, 64, C.c_float(10.0), C.c_float(30.0), C.c_uint(3), C.byref(h)) == SMT_ERR_ARG
        assert not h.value
    # 2^41 hypotheses: 2^33 workgroups of 256 threads
    assert l.smt_cblsm_ad(a, b, 65536, 65536, 512, 1, c, None) == SMT_ERR_ARG
    assert l.smt_cblsm_choose_arm_length(0, a, None, b, c, 65536, 65536, 512, d, None) == SMT_ERR_ARG
    assert l.smt_cblsm_cost_aggregation_new(a, b, 65536, 65536, 512, 1, c, c, c, c, d, None) == SMT_ERR_ARG


# ------------------------------------------------------------------------------------------------------ the stages, small
@pytest.mark.parametrize("view", (0, 1))
def test_adcensus_rows(O, view):
    Lb, Rb = LV.image_block(H0, WS, 11), LV.image_block(H0, WS, 12)
    L, R = LV.tile_rows(Lb, K).astype(np.float32), LV.tile_rows(Rb, K).astype(np.float32)
    full = O.adcensus_view(L, R, D, LV.SIGMA_C, LV.SIGMA_S, view)
    three = LV.adcensus_expected(O, Lb, Rb, K, D, view)
    assert_row_structure(full, three, what=("adcensus", view))
    assert_row_structure(O.wta(full), [O.wta(v) for v in three], edges_differ=False, what=("adcensus map", view))
    # the three-block problem gives the same three blocks (the census window is 7 rows high, a block 13)
    assert all(same(a, b) for a, b in zip(LV.adcensus_expected(O, Lb, Rb, 3, D, view), three))


@pytest.mark.parametrize("order", (0, 1, 2))
def test_aggregation_rows(O, order):
    vb = LV.cost_block((H0, WS, D), 21)
    ab = LV.arm_block(H0, WS, 22)
    full, oob = O.aggregate_rect(LV.tile_rows(vb, K), LV.full_arms(ab, K), order)
    assert oob == 0
    vols, maps = LV.aggregate_expected(O, vb, ab, order)
    assert_row_structure(full, vols, what=("aggregate", order))
    assert_row_structure(O.wta(full), maps, edges_differ=False, what=("aggregate map", order))
    assert not np.isnan(full).any()


def test_per_pixel_stages_rows(O):
    """smt_wta and smt_cblsm_ad: the result of the tiled input is the tiled result"""
    vb = LV.cost_block((H0, WS, D), 31, levels=4)
    assert same(O.wta(LV.tile_rows(vb, K)), LV.tile_rows(O.wta(vb), K))
    Lb, Rb = LV.image_block(H0, WS, 32), LV.image_block(H0, WS, 33)
    for view in (0, 1):
        full = O.cblsm_ad(LV.tile_rows(Lb, K), LV.tile_rows(Rb, K), D, view)
        three = LV.split3(O.cblsm_ad(LV.tile_rows(Lb, 3), LV.tile_rows(Rb, 3), D, view), H0)
        assert_row_structure(full, three, edges_differ=False, what=("cblsm_ad", view))


@pytest.mark.parametrize("which", ("left", "right"))
def test_scan_rows(O, which):
    cb, gb = LV.cost_block((H0, WS, D), 41), LV.image_block(H0, WS, 42).astype(np.float32)
    full = O.scan_pass(LV.tile_rows(cb, K), LV.tile_rows(gb, K), LV.P1, LV.P2, which)
    one = LV.scan_rows_expected(O, cb, gb, which)
    assert_row_structure(full, (one, one, one), edges_differ=False, what=which)


@pytest.mark.parametrize("which", ("up", "down"))
def test_scan_cols_faithful_identity(O, which):
    """The faithful up / down passes read the guide at gray.flat[j +- s]: with a guide whose flat array has period w0 and
    a cost periodic along the columns, the pass over the full image is the pass over the strip [H][w0][D], column block
    by column block."""
    kc = WS // W0
    strip = LV.cost_block((H, W0, D), 51)
    guide = LV.flat_guide(H, WS, W0, 52)
    full = O.scan_pass(LV.tile_cols(strip, kc), guide, LV.P1, LV.P2, which)
    want = LV.scan_cols_expected(O, strip, guide[:, :W0], which, fixed=False)
    for k in range(kc):
        assert same(full[:, k * W0:(k + 1) * W0], want), (which, k)
    # the guide bites: a guide without the flat period breaks the identity
    other = LV.column_guide(H, W0, 53)
    assert not same(O.scan_pass(LV.tile_cols(strip, kc), LV.tile_cols(other, kc), LV.P1, LV.P2, which)[:, :W0],
                    O.scan_pass(strip, other, LV.P1, LV.P2, which))


@pytest.mark.parametrize("which", ("up", "down"))
def test_scan_cols_fixed(O, which):
    """under SMT_QUIRK_FIX_SCAN_VERTICAL the vertical pass is the horizontal pass of the transpose: column blocks of the
    transposed full problem are row blocks"""
    kc = WS // W0
    strip, gstrip = LV.cost_block((H, W0, D), 54), LV.column_guide(H, W0, 55)
    want = LV.scan_cols_expected(O, strip, gstrip, which, fixed=True)
    full_t = O.scan_pass(np.ascontiguousarray(LV.tile_cols(strip, kc).transpose(1, 0, 2)),
                         np.ascontiguousarray(LV.tile_cols(gstrip, kc).T), LV.P1, LV.P2, {"up": "left", "down": "right"}[which])
    full = np.ascontiguousarray(full_t.transpose(1, 0, 2))
    for k in range(kc):
        assert same(full[:, k * W0:(k + 1) * W0], want), (which, k)
    assert not same(want, LV.scan_cols_expected(O, strip, gstrip, which, fixed=False))


def test_composed_scanline_sum_is_the_oracles(O):
    kc = WS // W0
    cb = LV.cost_block((H0, W0, D), 61)
    guide = LV.flat_guide(H, WS, W0, 62)
    cost = LV.tile_rows(LV.tile_cols(cb, kc), K)
    want = O.scanline(cost, guide, LV.P1, LV.P2)
    l, r, u, d = [torch.from_numpy(a) for a in LV.scan_run_parts(O, cb, guide[0], H, WS)]
    got = torch.empty((H, WS, D))
    pieces = LV.row_chunks(H, H0, WS * D * 4, chunk=2 * H0 * WS * D * 4)
    assert len(pieces) == 3
    for r0, r1 in pieces:
        got[r0:r1] = LV.compose_scan_run(l + r, u, d, r0, r1, kc)
    assert same(got.numpy(), want)
    LV.check_pieces(torch.from_numpy(want), H0, lambda r0, r1: LV.compose_scan_run(l + r, u, d, r0, r1, kc), "composed",
                    chunk=2 * H0 * WS * D * 4)
    assert same(LV.first_min(got).numpy(), O.wta(want))
    for which, part in (("left", l), ("right", r)):
        assert same(O.scan_pass(cost, guide, LV.P1, LV.P2, which), LV.tile_rows(part.numpy(), K)), which
    for which, part in (("up", u), ("down", d)):
        assert same(O.scan_pass(cost, guide, LV.P1, LV.P2, which), LV.tile_cols(part.numpy(), kc)), which


@pytest.mark.parametrize("win", (1,))
def test_ncc_rows(O, win):
    Lb, Rb = LV.image_block(H0, WS, 71), LV.image_block(H0, WS, 72)
    full = X.ncc_exact(LV.tile_rows(Lb, K), LV.tile_rows(Rb, K), D, win)
    three = X.ncc_exact(LV.tile_rows(Lb, 3), LV.tile_rows(Rb, 3), D, win)
    for f, t in zip(full, three):
        b = f.reshape(K, H0, WS, D)
        for k in range(2, K - 1):
            assert np.array_equal(b[k], b[1], equal_nan=True)
        for got, want in zip((b[0], b[1], b[K - 1]), LV.split3(t, H0)):
            assert np.array_equal(got, want, equal_nan=True)
    disp, cost = O.ncc(LV.tile_rows(Lb, K), LV.tile_rows(Rb, K), D, win, want_cost=True)
    _, cost3 = O.ncc(LV.tile_rows(Lb, 3), LV.tile_rows(Rb, 3), D, win, want_cost=True)
    assert_row_structure(cost, LV.split3(cost3, H0), what="ncc costs")
    assert same(disp, X.ncc_wta(cost, win))
    assert_row_structure(disp, LV.split3(X.ncc_wta(cost3, win), H0), edges_differ=False, what="ncc map")
    X.check_ncc(cost3, *three, win, "loop")


def test_sad_rows(O):
    ws = 0
    left_costs = LV.left_costs_fn()
    Lb, Rb = LV.image_block(H0, WS, 81), LV.image_block(H0, WS, 82)

    def run(k):
        Lp, Rp = O.pad_replicate(LV.tile_rows(Lb, k), ws + 1), O.pad_replicate(LV.tile_rows(Rb, k), ws + 1)
        return left_costs(Lp, Rp, D, ws), O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
    full, three = run(K), run(3)
    assert_row_structure(full[0], LV.split3(three[0], H0), what="costL")
    for v in (1, 2):
        assert_row_structure(full[v], LV.split3(three[v], H0), edges_differ=False, what=("sad map", v))


# ---------------------------------------------------------------------------------------------------------- first minimum
def test_first_min_is_the_oracles_wta_with_ties_and_nans(O):
    rng = np.random.default_rng(91)
    v = rng.integers(0, 3, (H0, WS, D)).astype(np.float32)              # ties everywhere
    v[0, 0, 0] = np.nan                                                  # NaN at d = 0: frozen at 0
    v[0, 1, 0], v[0, 1, 5] = np.nan, -1.0
    v[1, 2, 7] = np.nan                                                  # NaN at d > 0: never wins
    v[1, 3, 1:] = np.nan
    v[2, 4, :] = np.nan
    v[3, 5, :] = 2.0                                                     # all tied: the first
    v[3, 6, :] = 2.0
    v[3, 6, D - 1] = 1.0                                                 # the minimum at the last d
    v[4, 7, 3], v[4, 7, 9] = -5.0, -5.0
    v[4, 8, 2], v[4, 8, 3] = np.nan, -7.0
    want = O.wta(v)
    t = torch.from_numpy(v)
    assert same(LV.first_min(t).numpy(), want)
    assert want[0, 0] == 0 and want[0, 1] == 0 and want[3, 6] == D - 1 and want[4, 7] == 3 and want[4, 8] == 3
    # chunked, as the GPU cases apply it
    got = torch.cat([LV.first_min(t[r0:r1]) for r0, r1 in LV.row_chunks(H0, 1, WS * D * 4, chunk=3 * WS * D * 4)])
    assert same(got.numpy(), want)


# ----------------------------------------------------------------------------------------------------- planted defects
def _periodic(k=10, h0=4, shape=(6, 5), dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    blk = lambda: torch.rand((h0,) + shape, generator=g).to(dtype)      # noqa: E731
    top, mid, bot = blk(), blk(), blk()
    return torch.cat([top] + [mid] * (k - 2) + [bot]).contiguous(), (top.numpy(), mid.numpy(), bot.numpy()), h0


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("chunk", (None, 1, 1000))
def test_row_helper_accepts_the_clean_result_and_rejects_planted_defects(dtype, chunk):
    out, three, h0 = _periodic(dtype=dtype)
    LV.check_rows(out, h0, *three, "clean", chunk=chunk)
    assert LV.differing_blocks(out, h0, chunk=chunk) == []
    # one unwritten element: the prefill's 0xFF bytes
    for at in ((5 * h0 + 1, 2, 3), (1, 0, 0), (1 * h0, 5, 4), (10 * h0 - 1, 5, 4), (8 * h0 + 3, 0, 0)):
        bad = out.clone()
        LV.bits(bad)[at] = -1
        with pytest.raises(AssertionError):
            LV.check_rows(bad, h0, *three, "unwritten", chunk=chunk)
    # one block shifted by a row
    bad = out.clone()
    bad[4 * h0:5 * h0] = out[4 * h0 - 1:5 * h0 - 1]
    with pytest.raises(AssertionError, match="first at block 4"):
        LV.check_rows(bad, h0, *three, "shifted", chunk=chunk)
    # one element changed in block 7, by one unit in the last place
    bad = out.clone()
    LV.bits(bad)[7 * h0 + 2, 3, 1] += 1
    assert LV.differing_blocks(bad, h0, chunk=chunk) == [7]
    with pytest.raises(AssertionError, match="first at block 7"):
        LV.check_rows(bad, h0, *three, "changed", chunk=chunk)
    # a wrong oracle block
    wrong = three[1].copy()
    wrong[0, 0, 0] += 1
    with pytest.raises(AssertionError, match="second block"):
        LV.check_rows(out, h0, three[0], wrong, three[2], "oracle", chunk=chunk)
    # -0.0 is not +0.0 and a NaN equals itself: bits, not values
    z = out.clone()
    z[:, 0, 0] = 0.0
    t3 = [a.copy() for a in three]
    for a in t3:
        a[:, 0, 0] = 0.0
    LV.check_rows(z, h0, *t3, "zeros", chunk=chunk)
    z[6 * h0, 0, 0] = -0.0
    with pytest.raises(AssertionError):
        LV.check_rows(z, h0, *t3, "minus zero", chunk=chunk)
    n = out.clone()
    n[:, 1, 1] = float("nan")
    t3 = [a.copy() for a in three]
    for a in t3:
        a[:, 1, 1] = np.nan
    LV.check_rows(n, h0, *t3, "NaNs", chunk=chunk)


def test_prefill_is_all_ones_and_maps_are_compared_too():
    for dt in (torch.float32, torch.float64, torch.int32):
        p = LV.prefilled((3, 4), dt, "cpu")
        assert (p.view(torch.uint8) == 255).all()
    out, three, h0 = _periodic(shape=(6,))
    LV.check_rows(out, h0, *three, "maps")
    bad = out.clone()
    bad[7 * h0, 0] += 1
    with pytest.raises(AssertionError):
        LV.check_rows(bad, h0, *three, "maps")


@pytest.mark.parametrize("chunk", (None, 1, 700))
def test_column_and_piece_helpers_reject_planted_defects(chunk):
    g = torch.Generator().manual_seed(6)
    Hh, w0, kc, d = 9, 3, 5, 4
    strip = torch.rand((Hh, w0, d), generator=g)
    out = strip.repeat(1, kc, 1).contiguous()
    LV.check_cols(out, w0, strip.numpy(), "clean", chunk=chunk)
    for at in ((0, 0, 0), (8, 14, 3), (4, 7, 2)):
        bad = out.clone()
        LV.bits(bad)[at] = -1
        with pytest.raises(AssertionError):
            LV.check_cols(bad, w0, strip.numpy(), "unwritten", chunk=chunk)
    bad = out.clone()
    bad[:, 3:6] = out[:, 2:5]                                            # one column block shifted by a column
    with pytest.raises(AssertionError, match="column block 1"):
        LV.check_cols(bad, w0, strip.numpy(), "shifted", chunk=chunk)
    piece = lambda r0, r1: out[r0:r1]                                    # noqa: E731
    LV.check_pieces(out.clone(), 3, piece, "clean", chunk=chunk)
    bad = out.clone()
    LV.bits(bad)[7, 2, 1] += 1
    with pytest.raises(AssertionError, match=r"first at \[7, 2, 1\]"):
        LV.check_pieces(bad, 3, piece, "changed", chunk=chunk)
