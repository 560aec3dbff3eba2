"""The case table of the flow sweep (tests/fuzz_flow_cases.py) is worth running: every row the families must reach is
reached (recomputed from the table here), the three batches of a group give different maps, no map of a non-constant
pair is constant, the LR checks meet all three classes and the speckle filters change pixels, and the oracle side of
every family finishes.  Oracle only, no GPU."""
import time

import numpy as np
import pytest

import cblsm_v4_cases as VC
import fuzz_flow_cases as FC

WALL = {}


def _all(O, family):
    """every batch of every group through the oracle (cached in fuzz_flow_cases); the wall time of the first pass"""
    t0 = time.perf_counter()
    res = {g["name"]: [FC.oracle_batch(family, g, k, O) for k in range(3)] for g in FC.groups(family)}
    WALL.setdefault(family, time.perf_counter() - t0)
    return res


def _in(lo, hi, values):
    return any(lo <= v <= hi for v in values)


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("family", FC.FAMILIES)
def test_groups_hold_three_different_batches(O, family):
    gs = FC.groups(family)
    assert any(5 in [b["P"] for b in g["batches"]] for g in gs), "no group with a five-pair batch"
    for g in gs:
        Ps = [b["P"] for b in g["batches"]]
        assert len(Ps) == 3 and len(set(Ps)) >= 2 and 1 in Ps, (g["name"], Ps)
        assert g["H"] * g["W"] * g["D"] * max(Ps) <= 1.3 * FC.BUDGET[family], g["name"]
        imgs = [FC.gray_pairs(g, k, O) for k in range(3)]
        for k in range(3):
            assert len(imgs[k]) == Ps[k]
            assert not FC.is_constant_pair(*imgs[k][-1]), (g["name"], k)
        for a, b in ((0, 1), (1, 2), (2, 0)):                    # (2, 0): the first batch is run again after the third
            assert not np.array_equal(imgs[a][-1][0], imgs[b][0][0]), (g["name"], a, b)
    # the table is the same everywhere: a second build from the seed gives the same rows
    assert FC._table()[family] == gs


def test_image_kinds_are_mixed(O):
    """synthetic pairs with and without noise, and random, piecewise-smooth and constant images all occur"""
    const = noisy = smooth = 0
    for family in FC.FAMILIES:
        for g in FC.groups(family):
            for k in range(3):
                for L, R in FC.gray_pairs(g, k, O):
                    for x in (L, R):
                        if x.min() == x.max():
                            const += 1
                        elif x.size >= 40 and len(np.unique(x)) > x.size // 3:
                            noisy += 1
                        else:
                            smooth += 1
    assert const >= 3 and noisy >= 10 and smooth >= 10, (const, noisy, smooth)


# ------------------------------------------------------------------------------------------------ coverage rows
def test_pipeline_rows():
    gs = FC.groups("pipeline")
    Ds = [g["D"] for g in gs]
    for lo, hi in FC.PIPE_D_BINS:
        assert _in(lo, hi, Ds), (lo, hi)
    assert any(g["H"] == 1 for g in gs)
    assert any(g["W"] < g["D"] for g in gs)
    assert any(g["W"] % 4 for g in gs) and any(g["W"] % 64 and g["W"] > 64 for g in gs)
    assert any(g["W"] > g["H"] and not g["fix_stride"] for g in gs)
    assert all(g["W"] >= g["H"] for g in gs if not g["fix_stride"])     # flags 0: the reference is undefined on portraits
    fixed = [g for g in gs if g["fix_stride"]]
    assert 4 * len(fixed) == len(gs)
    assert any(g["H"] == g["W"] for g in fixed) and any(g["H"] > g["W"] for g in fixed)
    by_sched = {s: [g for g in gs if g["schedule"] == s] for s in FC.PIPE_SCHEDULES}
    assert all(by_sched[s] for s in FC.PIPE_SCHEDULES)
    assert {b["P"] for g in by_sched["2"] for b in g["batches"]} >= {1, 2, 5}
    # scanline instantiations: C = ceil(D / 64) hypotheses per lane from 1 to 4, each with a full and a partial last chunk,
    # and C = 5 by some D in 257 .. 320 (full or partial, whichever is drawn).  C = 6 .. 8 (D up to 512) lie beyond the
    # bins this table takes and are NOT reached inside the pipeline here.
    assert {(-(-D // 64), D % 64 == 0) for D in Ds} >= {(c, f) for c in (1, 2, 3, 4) for f in (True, False)}
    assert any(D > 256 for D in Ds)                                    # the D > 256 aggregation kernel


def test_cblsm_rows():
    gs = FC.groups("cblsm")
    Ds = [g["D"] for g in gs]
    assert _in(1, 64, Ds) and _in(65, 256, Ds) and _in(257, 512, Ds)
    assert any(g["H"] == 1 for g in gs) and any(g["W"] == 1 for g in gs)
    assert {0, 255} <= {g["tau"] for g in gs} and len({g["tau"] for g in gs}) >= 3
    assert len({g["max_length"] for g in gs}) >= 2 and len({g["sec_length"] for g in gs}) >= 3


def test_crossagg_rows():
    gs = FC.groups("crossagg")
    assert {g["num_iters"] for g in gs} == {0, 1, 2, 3, 4}
    assert any(g["L1"] > g["W"] for g in gs)
    Ds = [g["D"] for g in gs]
    assert {1, 64, 65} <= set(Ds) and any(D > 256 for D in Ds)
    assert {g["gray_given"] for g in gs} == {False, True}


def test_sad_rows():
    gs = FC.groups("sad")
    assert {g["winsize"] for g in gs} == {0, 1, 2, 3, 4}
    assert {1, 64, 65, 130} <= {g["D"] for g in gs}
    assert any(g["W"] <= g["D"] and g["D"] > 1 for g in gs)


def test_ncc_rows():
    gs = FC.groups("ncc")
    full = [g for g in gs if g["H"] > 2 * g["winSize"] and g["W"] > 2 * g["winSize"]]
    rule = {(2 * g["winSize"] + 1, g["D"]): FC.ncc_rule(2 * g["winSize"] + 1, g["D"]) for g in full}
    # the rule switches between neighbouring sides at the same D ...
    for a, b in ((7, 9), (31, 33), (181, 183)):
        assert any(sa == a and (b, D) in rule and rule[a, D] != rule[b, D] for (sa, D) in rule), (a, b)
    # ... and between D = 32 | 33 and 64 | 65 at one side, reached from both sides
    assert any(rule.get((s, 32)) == FC.NCC_DOT4 and rule.get((s, 48)) == FC.NCC_BOX and rule.get((s, 65)) == FC.NCC_DOT4
               for s in {s for s, _ in rule})
    assert set(rule.values()) == {FC.NCC_LOOP, FC.NCC_DOT4, FC.NCC_BOX}
    for g in gs:
        assert {0, FC.NCC_LOOP} <= set(g["forms"])
    assert any(FC.NCC_BOX in g["forms"] for g in gs) and any(FC.NCC_DOT4 in g["forms"] for g in gs)
    assert any(g["H"] <= 2 * g["winSize"] or g["W"] <= 2 * g["winSize"] for g in gs)


def test_asw_rows():
    gs = FC.groups("asw")
    assert {g["winSize"] for g in gs} == {1, 2, 3}
    assert {1, 64, 70} <= {g["D"] for g in gs}


def test_host_rows():
    gs = FC.groups("host")
    assert {(g["channels"], g["u8"]) for g in gs} == {(1, False), (1, True), (3, False), (3, True)}
    Pmax = {g["name"]: max(b["P"] for b in g["batches"]) for g in gs}
    assert {1, 2} <= {g["chunk"] for g in gs} and any(g["chunk"] > Pmax[g["name"]] for g in gs)
    assert {64, 192, 256, 320} <= {g["D"] for g in gs}
    assert all(not g["u8"] for g in gs if g["D"] > 256)


# ------------------------------------------------------------------------------------------------ the oracle side
def test_v4_restatement_equals_cblsm_v4_cases():
    """fuzz_flow_cases.v4_volume is cblsm_v4_cases.v4_numpy in another loop order: the same bits, NaNs by position"""
    for seed, (H, W, D) in enumerate([(5, 7, 6), (1, 9, 4), (6, 1, 3)]):
        rng = np.random.default_rng(seed)
        vol = rng.integers(0, 256, (H, W, D)).astype(np.float32)
        arms = VC.random_arm_volumes(H, W, D, seed)
        a, b = FC.v4_volume(vol, *arms), VC.v4_numpy(vol, *arms)
        assert np.isnan(b).any() or D < 4
        assert VC.same_volume(a, b)


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_oracle_side_finishes_and_discriminates(O, family, capsys):
    res = _all(O, family)
    with capsys.disabled():
        print(f"\nflow sweep, oracle side of {family}: {WALL[family]:.1f} s for {len(res)} groups")
    maps = FC.MAPS[family]
    for g in FC.groups(family):
        batches = res[g["name"]]
        imgs = [FC.gray_pairs(g, k, O) for k in range(3)]
        # no map of a non-constant pair is constant, stereo pair or two independent rand_img draws.  Exempt are a pair with
        # a constant image, what is constant whatever the images are (FC.by_construction_constant: D = 1, W = 1, an empty
        # NCC interior, the costAggregationV4 map on one row), and that map on a pair none of whose rectangles holds a tap
        # (recomputed by the oracle per pair; it happens under tau = 0 on images without equal neighbours)
        for k in range(3):
            for p, o in enumerate(batches[k][0]):
                if FC.is_constant_pair(*imgs[k][p]):
                    continue
                for m in maps:
                    empty = m == "v4" and bool(o["v4_empty"])         # recomputed: no V4 rectangle of this pair holds a tap
                    assert not empty or g["tau"] == 0 or g["H"] == 1 or g["W"] == 1, (g["name"], k, p)
                    if FC.by_construction_constant(family, g, m) or empty:
                        assert o[m].min() == o[m].max(), (g["name"], k, p, m)        # the exemption is what it says
                    else:
                        assert o[m].min() != o[m].max(), (g["name"], k, p, m)
        # consecutive batches (and the third against the first, which is run again) differ in their maps, pair by pair
        # and against the previous batch's last pair: a stale table, volume or map would be seen
        for a, b in ((0, 1), (1, 2), (2, 0)):
            prev, cur = batches[a][0], batches[b][0]
            if g["D"] == 1 or g["W"] == 1 or (family == "ncc" and "exact" not in cur[0]):    # maps of zeros: the volumes
                vols_a, vols_b = batches[a][1], batches[b][1]
                for n in vols_a:
                    if vols_a[n].dtype.kind == "f" and not np.isnan(vols_a[n]).all():
                        assert not np.array_equal(vols_a[n], vols_b[n], equal_nan=True), (g["name"], a, b, n)
                continue
            for p, o in enumerate(cur):
                if FC.is_constant_pair(*imgs[b][p]):
                    continue
                for q in {min(p, len(prev) - 1), len(prev) - 1}:
                    look = maps + (("cost",) if family == "ncc" else ())
                    assert any(not np.array_equal(o[m], prev[q][m], equal_nan=m == "cost") for m in look), (g["name"], a, b, p, q)
                    if family in ("pipeline", "cblsm", "crossagg"):
                        assert not np.array_equal(o[maps[0]], prev[q][maps[0]]), (g["name"], a, b, p, q)


@pytest.mark.parametrize("family,cls,before,after", [("pipeline", "cls", "lr", "sp"), ("cblsm", "post_cls", "post_lr", "post_sp"),
                                                     ("crossagg", "post_cls", "post_lr", "post_sp")])
def test_lr_check_and_speckle_filter_have_work(O, family, cls, before, after):
    res = _all(O, family)
    classes, changed = set(), 0
    for batches in res.values():
        for outs, _ in batches:
            for o in outs:
                classes |= set(np.unique(o[cls]).tolist())
                changed += int((o[before].view(np.uint32) != o[after].view(np.uint32)).sum())
    assert classes == {0, 1, 2}, classes
    assert changed >= 1
