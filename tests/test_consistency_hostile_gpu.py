"""The consistency checks on maps a matcher is not supposed to produce.  smt_lrcheck -- the in-place LeftRightConsistency
that closes the pipeline and the CBLSM / CrossAgg tails -- on fractions and x.5 ties, negative, non-finite and out-of-int
disparities and on columns that land on -1, 0, W - 1 and W (tests/golden/ref_pin_cases.hostile_lr_maps; the same inputs
are lrcheck cases of the reference pin, where the oracle must equal the reference's own compiled code); the two
CrossCheckDiaparity kernels on negative, out-of-map and non-finite values; CBLSMTail on one such pair.  All against the
oracle, bit for bit, into prefilled outputs.  That the maps hold what they promise, and that the chain lr_rejected recomputes
is taken both ways, is asserted on the oracle alone in tests/test_ref_pin_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import median_inplace_cases as MC  # noqa: E402
import ref_pin_cases as RP  # noqa: E402
from prefill import first_diff, flows  # noqa: E402,F401  (the fixture: the api's output tensors come prefilled)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INT_MIN = -(2 ** 31)
GATES = (0, 1, 2, -1)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), \
        f"{what}: {first_diff(got, want)}"


@pytest.mark.parametrize("H,W,seed,_gate", RP.HOSTILE_LR, ids=[f"{c[0]}x{c[1]}" for c in RP.HOSTILE_LR])
def test_lrcheck_in_place_on_hostile_maps(flows, O, H, W, seed, _gate):
    smt = flows
    dL, dR = RP.hostile_lr_maps(H, W, seed)
    for gate in GATES:
        ref, cls, no, nm = O.lrcheck(dL, dR, gate)
        t, r = T(dL.copy()), T(dR)
        gcls, gno, gnm, occ, mis = smt.LeftRightConsistency(W, H, gate, t, r, want_lists=True)
        tag = f"smt_lrcheck {H}x{W} gate {gate}"
        same(gcls, cls, tag + " cls")
        assert (gno, gnm) == (no, nm), (tag, (gno, gnm), (no, nm))
        # NaN inputs stay where they are kept: compare bits, not values
        same(t, ref, tag + " leftDisp")
        same(r, dR, tag + " rightDisp (read only)")
        same(occ, np.argwhere(cls == 1).astype(np.int32).reshape(-1, 2), tag + " occlusion list")
        same(mis, np.argwhere(cls == 2).astype(np.int32).reshape(-1, 2), tag + " mismatch list")


def _hostile_int_maps(H, W, seed):
    rng = np.random.default_rng(seed)
    n = H * W
    dL = rng.integers(0, 20, (H, W)).astype(np.int32)
    dR = rng.integers(0, 20, (H, W)).astype(np.int32)
    special = np.array([-1, -7, -n + 1, -n, -n - 1, n - 1, n, n + 1, 3 * n, INT_MIN, INT_MIN + 1, 2 ** 31 - 1, 2 ** 31 - 6,
                        -5, 5, 6], np.int64)
    for m in (dL, dR):
        k = rng.random((H, W)) < 0.3
        m[k] = rng.choice(special, int(k.sum())).astype(np.int32)
    return dL, dR


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (5, 300), (33, 77)])
def test_sad_crosscheck_on_hostile_maps(flows, O, H, W):
    dL, dR = _hostile_int_maps(H, W, 100 * H + W)
    if H * W > 50:
        assert (dL < 0).any() and (dL == INT_MIN).any() and (dL > H * W).any()
    smt = flows
    want, wcls = O.sad_crosscheck(dL, dR)
    out, cls = smt.sad_CrossCheckDiaparity(T(dL), T(dR))
    same(out, want, f"smt_sad_crosscheck {H}x{W} lastdisp")
    same(cls, wcls, f"smt_sad_crosscheck {H}x{W} cls")


def _hostile_float_maps(H, W, seed):
    rng = np.random.default_rng(seed)
    dL = rng.integers(0, 20, (H, W)).astype(np.float32)
    dR = rng.integers(0, 20, (H, W)).astype(np.float32)
    special = np.array([0.25, 4.5, 7.75, 255.9, 256.0, 300.7, -0.0, -0.75, -1.0, -3.5, -300.7, np.nan, np.inf, -np.inf, 3e9, -3e9,
                        float(H * W), float(-H * W)], np.float32)
    for m in (dL, dR):
        k = rng.random((H, W)) < 0.35
        m[k] = rng.choice(special, int(k.sum()))
    return dL, dR


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (5, 300), (33, 77)])
def test_asw_crosscheck_on_hostile_maps(flows, O, H, W):
    dL, dR = _hostile_float_maps(H, W, 100 * H + W)
    if H * W > 50:
        for m in (dL, dR):
            assert np.isnan(m).any() and np.isinf(m).any() and (m < 0).any() and (m == np.float32(300.7)).any() and (m == np.float32(3e9)).any()
    smt = flows
    same(smt.asw_CrossCheckDiaparity(T(dL), T(dR)), O.asw_crosscheck(dL, dR), f"smt_asw_crosscheck {H}x{W}")


def test_cblsm_tail_on_a_hostile_pair(flows, O):
    """CBLSM.cpp:160-162 with the default post parameters (gate 5, RemoveSpeckles(1, 50, INT_MIN), a 3 x 3 in-place
    median) on the 33 x 77 hostile pair, as one [H][W] pair and as a batch of two different pairs"""
    (H, W, seed, _), (_, _, seed2, _) = RP.HOSTILE_LR[-1], RP.HOSTILE_LR[-2]
    smt = flows
    pairs = [RP.hostile_lr_maps(H, W, seed), RP.hostile_lr_maps(H, W, seed2)]

    def chain(dL, dR):
        lr, cls, no, nm = O.lrcheck(dL, dR, 5)
        sp = O.remove_speckles(lr, 1, 50, INT_MIN)
        return MC.oracle_inplace(sp, 3), cls, np.array([no, nm], np.int32)

    fin, cls, counts = chain(*pairs[0])
    out, gcls, gcounts = smt.CBLSMTail(T(pairs[0][0].copy()), T(pairs[0][1]))
    same(out, fin, "CBLSMTail map")
    same(gcls, cls, "CBLSMTail cls")
    same(gcounts[0], counts, "CBLSMTail counts")
    out, gcls, gcounts = smt.CBLSMTail(T(np.stack([p[0] for p in pairs])), T(np.stack([p[1] for p in pairs])))
    for b, pr in enumerate(pairs):
        fin, cls, counts = chain(*pr)
        same(out[b], fin, f"CBLSMTail batch map {b}")
        same(gcls[b], cls, f"CBLSMTail batch cls {b}")
        same(gcounts[b], counts, f"CBLSMTail batch counts {b}")
