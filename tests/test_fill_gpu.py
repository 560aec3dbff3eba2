"""FillTheHole (PostProcessing.h:156-248) on the GPU against the oracle: bit-exact maps and the
replaced mismatch list.  The oracle is pinned to PostProcessing.h's own compiled code by tests/test_ref_pin_cpu.py
and cross-checked by an independent restatement in tests/test_cpu_oracle.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_case(rng, row, col, D, hole_frac, n_occ, extra_mis):
    d = rng.integers(0, D, (row, col)).astype(np.float32)
    holes = rng.random((row, col)) < hole_frac
    d[holes] = 65535
    d[rng.random((row, col)) < 0.02] = np.inf
    n = row * col

    def pairs(k):
        flat = rng.integers(0, n, k)
        p = np.stack([flat // row, flat % row], 1).astype(np.int32)
        # some entries in LeftRightConsistency's own (i, j) form: second >= width but inside the buffer
        if col > row and k > 4:
            i = rng.integers(0, row, k // 4)
            j = rng.integers(0, col, k // 4)
            p[: k // 4] = np.stack([i, j], 1)
        return p
    occ = pairs(n_occ)
    mis = pairs(int(holes.sum()) + extra_mis)
    if len(mis) > 9:
        mis[len(mis) // 3, 0] = col // 2          # angle switch in the middle of the list
        mis[-1] = mis[0]                          # a duplicate: the later entry wins
    return d, occ, mis


@pytest.mark.parametrize("row,col,D,seed", [(40, 40, 16, 0), (37, 61, 32, 1), (64, 150, 64, 2), (48, 100, 5, 3),
                                            (30, 45, 2, 4), (33, 33, 1, 5)])
def test_fill_the_hole_matches_oracle(smt, O, row, col, D, seed):
    rng = np.random.default_rng(seed)
    d, occ, mis = make_case(rng, row, col, D, 0.12, 50, 20)
    ref, third = O.fill_the_hole(d, D, occ, mis)
    g = T(d)
    out_list = smt.FillTheHole(row, col, D, g, occ, mis)
    assert np.array_equal(bits(g.cpu().numpy()), bits(ref))
    assert np.array_equal(out_list, third)


def test_switch_in_occlusion_list_persists(smt, O):
    """`angle` is declared outside the pass loop (:166): a switch in pass 0 holds for passes 1, 2."""
    rng = np.random.default_rng(11)
    row, col, D = 50, 70, 24
    d, occ, mis = make_case(rng, row, col, D, 0.2, 40, 10)
    mis[:, 0] = np.where(mis[:, 0] == col // 2, col // 2 + 1, mis[:, 0])      # no switch in the mismatch list
    occ[5, 0] = col // 2
    ref, third = O.fill_the_hole(d, D, occ, mis)
    g = T(d)
    out_list = smt.FillTheHole(row, col, D, g, occ, mis)
    assert np.array_equal(bits(g.cpu().numpy()), bits(ref))
    assert np.array_equal(out_list, third)


def test_empty_lists_and_skipped_third_pass(smt, O):
    rng = np.random.default_rng(12)
    row, col, D = 32, 48, 16
    d, occ, _ = make_case(rng, row, col, D, 0.1, 30, 0)
    none = np.empty((0, 2), np.int32)
    # empty mismatch list: the third pass does not run (:174), holes survive, list unchanged
    ref, third = O.fill_the_hole(d, D, occ, none)
    g = T(d)
    out_list = smt.FillTheHole(row, col, D, g, occ, none)
    assert third is None and len(out_list) == 0
    assert np.array_equal(bits(g.cpu().numpy()), bits(ref))
    assert (g == 65535).sum().item() > 0
    # both lists empty: nothing happens
    g2 = T(d)
    smt.FillTheHole(row, col, D, g2, none, none)
    assert np.array_equal(bits(g2.cpu().numpy()), bits(d))
    # no holes at all: the third pass finds nothing and the mismatch list becomes empty
    d3 = np.where(d == 65535, np.float32(3), d)
    mis = np.array([[1, 2], [3, 4]], np.int32)
    ref3, third3 = O.fill_the_hole(d3, D, none, mis)
    g3 = T(d3)
    out3 = smt.FillTheHole(row, col, D, g3, none, mis)
    assert np.array_equal(bits(g3.cpu().numpy()), bits(ref3)) and len(third3) == 0 and len(out3) == 0


def test_reference_ub_is_reported(smt, O):
    from stereo_match_traditional_amd import SmtError
    rng = np.random.default_rng(13)
    row, col, D = 30, 20, 8                      # portrait: (i, j) pairs can leave the buffer
    d, occ, mis = make_case(rng, row, col, D, 0.1, 10, 5)
    bad = np.concatenate([occ, np.array([[row - 1, col - 1]], np.int32)])     # (29*30 + 19) >= 600
    g = T(d)
    with pytest.raises(SmtError):
        smt.FillTheHole(row, col, D, g, bad, mis)
    assert np.array_equal(bits(g.cpu().numpy()), bits(d)), "nothing may be modified"
    with pytest.raises(ValueError):
        O.fill_the_hole(d, D, bad, mis)
    # more third-pass holes than mismatch entries
    g = T(d)
    with pytest.raises(SmtError):
        smt.FillTheHole(row, col, D, g, occ, mis[:2])
    with pytest.raises(ValueError):
        O.fill_the_hole(d, D, occ, mis[:2])


def test_after_left_right_consistency(smt, O):
    """main.cpp's order: LeftRightConsistency marks +inf (not 65535), so FillTheHole's rays treat
    those as valid values and its third pass finds no holes -- reproduced as is."""
    from stereo_match_traditional_amd import synth
    H, W, D = 64, 64, 32                        # square: the lists' (i, j) stay inside the swapped view
    L, R = synth.synth_pair(H, W, D, 5)
    adc = smt.AD_Census().Initialize(T(L.astype(np.float32)), T(R.astype(np.float32)), D, H, W, 10, 30)
    dl = torch.empty((H, W), device=DEV); dr = torch.empty((H, W), device=DEV)
    adc.ComputeBoth(dl, dr)
    cls, no, nm, occ, mis = smt.LeftRightConsistency(W, H, 2, dl, dr, want_lists=True)
    assert no + nm > 0
    before = dl.cpu().numpy()
    ref, third = O.fill_the_hole(before, D, occ, mis)
    out_list = smt.FillTheHole(H, W, D, dl, occ, mis)
    assert np.array_equal(bits(dl.cpu().numpy()), bits(ref))
    assert (third is None and np.array_equal(out_list, mis)) or np.array_equal(out_list, third)


def test_full_size_map(smt, O):
    """1920x1080 map, 4 % holes, D=192 search length."""
    rng = np.random.default_rng(21)
    row, col, D = 1080, 1920, 192
    d, occ, mis = make_case(rng, row, col, D, 0.04, 20000, 1000)
    ref, third = O.fill_the_hole(d, D, occ, mis)
    g = T(d)
    out_list = smt.FillTheHole(row, col, D, g, occ, mis)
    assert np.array_equal(bits(g.cpu().numpy()), bits(ref))
    assert np.array_equal(out_list, third)
