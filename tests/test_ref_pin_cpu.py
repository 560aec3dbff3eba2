"""Pins the CPU oracle to the reference's own AD-CensusV1 and CBLSM.h code, as test_crossagg_oracle_vs_reference_build
does for CrossAggregator: on every case of tests/golden/ref_pin_cases.py the oracle's outputs hash to
tests/golden/ref_pin_hashes.json (written from the reference builds by `make_golden.py ref-pin`), always, and equal
the reference builds bit for bit where oracle/_ref holds them.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ref_pin_cases as RP  # noqa: E402

GOLD = {r["case"]["name"]: r for r in
        json.load(open(os.path.join(ROOT, "tests", "golden", "ref_pin_hashes.json")))["cases"]}
IDS = [c["name"] for c in RP.CASES]


def _plain(case):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items()}


def test_fixture_holds_exactly_the_case_list():
    assert list(GOLD) == IDS
    for case in RP.CASES:
        assert GOLD[case["name"]]["case"] == _plain(case)
    kinds = {c["kind"] for c in RP.CASES}
    assert kinds == {"adcensus", "arms", "agg", "scan", "lrcheck", "lrvariant", "fill", "speckle", "median",
                     "cblsm_arms", "cblsm_ad", "cblsm_disp", "choose"}
    for kind in ("adcensus", "scan", "cblsm_ad"):
        assert {c["D"] for c in RP.CASES if c["kind"] == kind} >= set(RP.D_EDGES), kind
    assert {(c["D"], c["order"]) for c in RP.CASES if c["kind"] == "agg"} >= {(D, o) for D in RP.D_EDGES for o in (0, 1)}
    assert {c["order"] for c in RP.CASES if c["kind"] == "agg"} == {0, 1, 2}
    assert any(c["kind"] == "arms" and c["single"] and tuple(c["dirs"]) != (0, 1, 2, 3) for c in RP.CASES)


@pytest.mark.parametrize("case", RP.CASES, ids=IDS)
def test_oracle_vs_reference_build(O, case):
    rec = GOLD[case["name"]]
    inp = RP.inputs(case, O)
    assert RP.hashes(inp, O) == rec["inputs"], "regenerated inputs differ from the ones the fixture was made from"
    assert RP.admitted(case, inp, O), "the reference is undefined on this case: it must leave the list"
    out = RP.run(case, inp, O, "oracle")
    got = RP.hashes(out, O)
    assert list(got) == list(rec["outputs"])
    assert got == rec["outputs"], [k for k in got if got[k] != rec["outputs"][k]]
    need = O.have_ref_cblsm() if case["kind"].startswith(("cblsm", "choose")) else O.have_ref_adcensus()
    if case["kind"] == "agg" and case["order"] == 1:
        need = O.have_ref_cblsm()
    if need:
        ref = RP.run(case, inp, O, "ref")
        assert list(ref) == list(out)
        for k in out:
            a, b = RP.canon(out[k]), RP.canon(ref[k])
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


SCAN_TERM_CASES = [c for c in RP.CASES if c["kind"] == "scan" and c["terms"]]


def test_scan_term_cases_cover_the_vector_paths():
    """Partial and full vector paths with 1, 2, 4 and 5 hypotheses per 64-lane wave, and the reference's own
    penalties."""
    assert {64, 100, 256, 320} <= {c["D"] for c in SCAN_TERM_CASES}
    assert any((c["p1"], c["p2"]) == (10, 150) for c in SCAN_TERM_CASES)
    nf = {c["nonfinite"] for c in RP.CASES if c["kind"] == "scan"}
    assert nf >= {"nan_first_low", "nan_first_high", "nan_first_row", "interior", "inf_pixel"}


@pytest.mark.parametrize("case", SCAN_TERM_CASES, ids=[c["name"] for c in SCAN_TERM_CASES])
def test_scan_cases_reach_every_term(O, case):
    """In every pass l1, l3 and l4 -- and in the horizontal passes l2 -- are each the strict minimum in at least 2 % of
    the hypotheses, so a wrong neighbour exchange or pad cannot hide.  Counted by ref_pin_cases.term_shares from the
    reference build's path volumes (the oracle's where the build is absent; those hash to the same fixture), and
    only after the restatement reproduced those volumes bit for bit."""
    inp = RP.inputs(case, O)
    paths = RP.run(case, inp, O, "ref" if O.have_ref_adcensus() else "oracle")
    shares = RP.term_shares(case, inp, paths)
    print(case["name"], {p: tuple(round(x, 4) for x in s) for p, s in shares.items()})
    for name, (s1, s2, s3, s4) in shares.items():
        assert min(s1, s3, s4) >= RP.TERM_SHARE, (name, s1, s3, s4)
        if name in ("left", "right"):
            assert s2 >= RP.TERM_SHARE, (name, s2)
        else:
            assert s2 == 0.0          # l2 = l1 + p1 in ScanLineUpDown (:238): it can never win


def test_nan_first_pixel_changes_the_whole_line(O):
    """The reference reduces the first pixel with a sequential `minLastPath = min(cost, minLastPath)`
    (ScanlineOptimizer.h:163-166).  std::min(a, b) is `b < a ? b : a`: a NaN cost becomes the running minimum, and
    the next entry replaces it.  minLastPath is therefore the minimum of the entries AFTER the last NaN, the trailing
    pad included.  With the pixel's true minimum in front of the NaN, every later pixel of the line differs from
    what a NaN-ignoring minimum gives -- the case the GPU prologue must follow."""
    case = next(c for c in RP.CASES if c["name"] == "scan_nan_first_low_D64")
    inp = RP.inputs(case, O)
    got = O.scan_pass(inp["cost"], inp["gray"], case["p1"], case["p2"], "left")
    clean = inp["cost"].copy()
    first = clean[:, 0, :]
    first[np.isnan(first)] = 65535.0          # what fminf-style reduction would see
    other = O.scan_pass(clean, inp["gray"], case["p1"], case["p2"], "left")
    # hypotheses far from the NaN (at d = 2) see it only through minLastPath
    assert not np.isnan(got[:, 1, 10:]).any()
    # (where l4 wins, minLastPath cancels: not every hypothesis differs, but some do in every line)
    assert (got[:, 1, 10:] != other[:, 1, 10:]).any(axis=1).all()


def test_hostile_maps_hold_what_they_promise(O):
    """checked on the oracle alone: every kind of value is there, the columns land on the row ends, and the chain that
    lr_rejected recomputes is exercised both ways and decides classes"""
    H, W, seed, _ = RP.HOSTILE_LR[-1]
    dL, dR = RP.hostile_lr_maps(H, W, seed)
    for m in (dL, dR):
        assert np.isnan(m).any() and (m == np.inf).any() and (m == -np.inf).any()
        assert (m == np.float32(3e9)).any() and (m == np.float32(-3e9)).any() and (m == np.float32(1e30)).any()
        assert ((m != 0) & (np.abs(m) < np.finfo(np.float32).tiny)).any()                       # the denormal
        assert (np.signbit(m) & (m == 0)).any()                                                # -0.0
        fin = m[np.isfinite(m) & (np.abs(m) < 1e6)]
        assert {0.25, 0.5, 0.75} <= set(np.round(np.abs(fin) % 1, 2).tolist())
        assert (fin < 0).any()
    for gate in (0, 1, 2, -1):
        after, cls, _, _ = O.lrcheck(dL, dR, gate)
        rejected, kept, decides, ends_cr, ends_crl = RP.chain_counts(dL, dR, gate, after)
        # (under a negative gate every comparable pixel is rejected: nothing is left to be kept)
        assert rejected > 0 and decides > 0 and (kept > 0 or gate < 0), (gate, rejected, kept, decides)
        assert ends_cr == {-1, 0, W - 1, W}, (gate, ends_cr)
        # col_rl == j needs |d - dR| <= 1 up to the roundings: only the gates below 1 call that a mismatch
        assert ends_crl >= ({0, "j", W - 1, W} if gate < 1 else {0, W - 1, W}), (gate, ends_crl)
        assert set(np.unique(cls).tolist()) == {0, 1, 2}, gate
    # an x.5 tie of j - d + 0.5 on both sides of zero: -0.5 truncates to column 0, not to -1
    jj = np.broadcast_to(np.arange(W, dtype=np.float32), (H, W))
    with np.errstate(invalid="ignore"):
        t = jj - dL + np.float32(0.5)
        assert (t == -0.5).any() and (t == -1.0).any() and (np.isfinite(t) & (t > 0) & (t % 1 == 0.5)).any()


def test_reference_builds_are_clean_under_asan():
    """`make -C oracle ref-asan`: the two reference wrappers built with AddressSanitizer run every admitted case once
    (host code; leaks are not reported, the reference leaks by design).  Skipped as the reference build is where the
    reference tree is absent."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref-asan", "PYTHON=" + sys.executable],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if "reference tree absent" in r.stdout:
        return
    assert "reference sanitizer run clean (%d cases)" % len(RP.CASES) in r.stdout
