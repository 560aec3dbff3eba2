"""The scanline optimiser on both views (include/smt_scan_views.h): the case tables and oracle
compositions that tests/test_scan_views_cpu.py and tests/test_scan_views_gpu.py share.  A plain module, importable
without a GPU; every reference is computed once per process and returned read-only.

Scanline cases.  SHAPES covers a single row, a single column, W no multiple of the four columns per workgroup, the FULL
form (D = 64 C) for C = 1 and 3, the predicated form for C = 2 and 5, and more lines than one grid row of workgroups.
The two views get different volumes and different guides (view 1's are drawn from another stream), so a swapped pointer
shows.  Costs are small random integers as in bounds_cases._scanline: every sum is exact, so the association order is
the only thing that could differ, and results are held bit for bit.

Pipeline cases.  PIPE_CASES: (12, 40, 16), (9, 70, 70) and a square shape under QUIRK_FIX_RIGHT_ARM_STRIDE, each with
batches of 1, 2, 3 and 5 pairs of fuzz_flow_cases._synth_pair's column-offset inputs.  The draws were chosen on the CPU
so that the oracle alone meets the conditions check_pipe_conditions asserts."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import fuzz_flow_cases as FC  # noqa: E402
from subpixel_cases import restate  # noqa: E402

P1, P2, GATE = 10, 150, 2
SHAPES = ((1, 8, 16), (8, 1, 16), (5, 7, 3), (9, 13, 64), (6, 10, 70), (4, 9, 192), (3, 6, 320), (3, 70, 16))
# smt_scanline_run_pair uses the view axis up to H = 512 and the single-view launches beyond: both sides of the switch
TALL = ((512, 3, 16), (513, 3, 16))
MIN_DENS = (None, 1.0, 2.0 ** -20)
COMBOS = ((True, True), (True, False), (False, True), (False, False))     # per view: the sum is stored
QUIRK_FIX_SCAN_VERTICAL, QUIRK_FIX_RIGHT_ARM_STRIDE = 0x4, 0x1


def _ro(a):
    a.setflags(write=False)
    return a


_in, _ref = {}, {}


def inputs(H, W, D, view):
    """(cost [H][W][D], gray [H][W]) of a view, float32"""
    key = (H, W, D, view)
    if key not in _in:
        rng = np.random.default_rng([H, W, D, 17 + view])
        _in[key] = (_ro(rng.integers(0, 8, (H, W, D)).astype(np.float32)), _ro(rng.integers(0, 256, (H, W)).astype(np.float32)))
    return _in[key]


def scan_pass_ref(O, cost, gray, which, fixed):
    """bounds_cases._scan_ref's identity, restated: under SMT_QUIRK_FIX_SCAN_VERTICAL the up / down passes are the left /
    right passes of the transposed volume and guide"""
    if fixed and which in ("up", "down"):
        t = O.scan_pass(np.ascontiguousarray(cost.transpose(1, 0, 2)), np.ascontiguousarray(gray.T), P1, P2,
                        "left" if which == "up" else "right")
        return np.ascontiguousarray(t.transpose(1, 0, 2))
    return O.scan_pass(cost, gray, P1, P2, which)


def scan_sum(O, cost, gray, fixed):
    """ScanLine's volume: O.scanline, or ((left + right) + up) + down with the fixed vertical passes"""
    if not fixed:
        return O.scanline(cost, gray, P1, P2)
    p = [scan_pass_ref(O, cost, gray, w, True) for w in ("left", "right", "up", "down")]
    with np.errstate(invalid="ignore"):
        return ((p[0] + p[1]) + p[2]) + p[3]


def disp_of(O, vol, min_den):
    return O.wta(vol) if min_den is None else restate(O, vol, min_den)


def reference(O, H, W, D, view, fixed):
    key = (H, W, D, view, fixed)
    if key not in _ref:
        cost, gray = inputs(H, W, D, view)
        _ref[key] = _ro(scan_sum(O, cost, gray, fixed))
    return _ref[key]


# ---- non-finite costs: ref_pin_cases' constructions, one volume row with a NaN and one with +inf per view
NONFINITE = ((6, 11, 64), (5, 9, 70))


def nonfinite_inputs(H, W, D, view):
    import ref_pin_cases as RP
    nf = ("nan_first_low", "nan_first_row")[view]
    c = RP._scan_inputs(dict(H=H, W=W, D=D, seed=900 + view, gen="u2", nonfinite=nf, scale=1.0))
    cost, gray = c["cost"], c["gray"]
    cost[H // 2, W // 2, :] = np.inf                       # inf_pixel's row
    cost[1, W - 2, D // 3] = np.nan                        # an interior NaN
    cost[H - 2, 1, D - 1] = np.inf
    assert np.isnan(cost).any() and np.isinf(cost).any()
    return cost, gray


# ---- the pipeline under SMT_VIEW_BOTH
# Pair k of a case is drawn from default_rng([seed, k, draws[k]]).  draws[k] is the first draw whose pair meets the
# conditions of check_pipe_conditions, found on the CPU with the oracle alone and recorded here; the test asserts them.
PIPE_CASES = (dict(name="12x40x16", H=12, W=40, D=16, fix=False, seed=101, draws=(2, 2, 7, 4, 2, 9, 1, 0, 0, 8, 0)),
              dict(name="9x70x70", H=9, W=70, D=70, fix=False, seed=202, draws=(1, 4, 0, 2, 1, 1, 2, 0, 0, 1, 1)),
              dict(name="20x20x16_fix", H=20, W=20, D=16, fix=True, seed=303, draws=(5, 2, 3, 20, 10, 9, 1, 2, 1, 1, 1)))
PIPE_BATCHES = (1, 2, 3, 5)
SCHEDULES = (None, "0", "1", "2")
INT_MIN = FC.INT_MIN

_pairs, _pipe = {}, {}


def pipe_pairs(O, case):
    """the 11 gray pairs of a case, batch after batch: uint8 [H][W] each, none with a constant image"""
    if case["name"] not in _pairs:
        out = []
        for k in range(sum(PIPE_BATCHES)):
            rng = np.random.default_rng([case["seed"], k, case["draws"][k]])
            L, R = FC._synth_pair(O, rng, case["H"], case["W"], case["D"], bool(k % 2), turn=k)
            assert not FC.is_constant_pair(L, R)
            out.append((_ro(np.ascontiguousarray(L)), _ro(np.ascontiguousarray(R))))
        _pairs[case["name"]] = out
    return _pairs[case["name"]]


def pipe_pair_oracle(O, case, k, min_den=None):
    """pipeline_pair plus the right view's scanline: dict(left = LEFT's per-pair maps, both = BOTH's, sumR, vols)"""
    key = (case["name"], k, min_den)
    if key not in _pipe:
        L, R = pipe_pairs(O, case)[k]
        left, vols = FC.pipeline_pair(O, L, R, case["D"], case["fix"])
        sumR = O.scanline(vols["agg_right"], R.astype(np.float32), P1, P2)
        raw = disp_of(O, vols["scanline_sum"], min_den)
        dr = disp_of(O, sumR, min_den)
        lr, cls, no, nm = O.lrcheck(raw, dr, GATE)
        sp = O.remove_speckles(lr, 1, 30, INT_MIN)
        both = dict(raw=raw, dr=dr, lr=lr, cls=cls, counts=np.array([no, nm], np.int32), sp=sp, med=O.median(sp, 3))
        for d in (left, both, vols):
            for a in d.values():
                a.setflags(write=False)
        _pipe[key] = dict(left=left, both=both, sumR=_ro(sumR), vols=vols)
    return _pipe[key]


def check_pipe_conditions(O, case):
    """conditions on the inputs that the oracle alone must meet (not measurements)"""
    for k in range(sum(PIPE_BATCHES)):
        o = pipe_pair_oracle(O, case, k)
        plain = O.wta(o["vols"]["agg_right"])
        share = float((o["both"]["dr"] != plain).mean())
        assert share >= 0.05, (case["name"], k, "the optimised right map equals the aggregated volume's WTA almost everywhere", share)
        assert (o["both"]["cls"] != o["left"]["cls"]).any(), (case["name"], k, "BOTH's class map equals LEFT's")
        for m in ("raw", "dr"):
            assert o["both"][m].min() != o["both"][m].max(), (case["name"], k, m, "constant map")
        assert o["left"]["dr"].min() != o["left"]["dr"].max(), (case["name"], k, "constant LEFT right map")


def batch_slices():
    out, k = [], 0
    for P in PIPE_BATCHES:
        out.append(range(k, k + P))
        k += P
    return out
