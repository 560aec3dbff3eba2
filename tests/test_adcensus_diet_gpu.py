"""The shared maps-only launch of smt_adcensus_compute_batch (adcensus_kernels.h, k_cost_maps_shared) after its vector diet:
the D = 192 walk takes whole groups of 3 pixels without a per-pixel exit and computes the ring base once per group
(shared_ring_slot), so a group reaches up to 4 slots past the ring's end.  Batches of 3 different pairs -- pair 0's
tables from k_prep, pairs 1 and 2's from table workgroups that write the two table sets alternately -- with every map
against the oracle bit for bit, and the last pair's lent volumes, which every table entry feeds, masks included.
Shapes: table rows with every count of missing taps, a tile's last partial row block, W at and past a tile edge; last
waves of 1, 2, 3 and 16 pixels, walks of 16 to 64 pixels (0, 1 and 2 tail pixels), the ring wrapped once and twice."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (1, 70, 64): every row lacks 4 taps above and 4 below, W six past a tile edge.  (4, 64, 64), (5, 67, 64): every count
# of missing taps above and below, W at and 3 past a tile edge (the two-view kernels' table workgroups: W - 3 - D < 3).
# (9, 131, 128): the first H with a row that lacks none.  (33, 200, 130): one row in the second tile row.
# (41, 257, 192): a 9-row last row block, W one past a tile edge.
TABLE_SHAPES = [(1, 70, 64), (4, 64, 64), (5, 67, 64), (9, 131, 128), (33, 200, 130), (41, 257, 192)]
# W = 257, 258, 259: a last wave of 1, 2, 3 pixels; 304: of 16.  (6, 700, 192): runs of 1 to 4 chunks, i.e. walks of 16,
# 32, 48 and 64 pixels -- 5, 10, 16 and 21 whole groups with 1, 2, 0 and 1 tail pixels -- and right columns past 512: the
# ring wrapped once.  (4, 1030, 192): wrapped twice, columns of residue 0..3 mod 512 in the spill slots.
# (6, 530, 128): C = 2, which keeps the per-pixel base, across the ring's end.
WALK_SHAPES = [(3, 257, 192), (3, 258, 192), (3, 259, 192), (3, 304, 192), (6, 700, 192), (4, 1030, 192), (6, 530, 128)]
_ORACLE = None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _handle(smt, Lb, Rb, D):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False, store_calibration=False)


def _batch(adc, Lb, Rb):
    """NaN-prefilled maps of one smt_adcensus_compute_batch call, and the status behind it (read-and-clear)"""
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), float("nan"), device=Lb.device)
    dr = torch.full((B, H, W), float("nan"), device=Lb.device)
    adc._bind_stream()
    assert lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), B, VIEW_BOTH, _p(dl), _p(dr)) == 0
    return dl, dr, lib().smt_adcensus_status(adc._h)


@functools.lru_cache(maxsize=None)
def _case(H, W, D):
    """3 different pairs with the oracle's maps of each and its volumes of the last, computed once per shape"""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 4700 + 17 * b + W + H, noise=(b != 1)) for b in range(3)])
    maps = []
    for b in range(3):
        vols = tuple(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, v) for v in (0, 1))
        maps.append((O.wta(vols[0]), O.wta(vols[1])))
    for v in vols:
        v.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), maps, vols


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS", "SMT_SHARED_FINISH"):
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, maps, what):
    for b, (ml, mr) in enumerate(maps):
        got = dl[b].cpu().numpy()
        assert np.array_equal(got, ml), ("left", b, np.argwhere(got != ml)[:4].tolist()) + what
        got = dr[b].cpu().numpy()
        assert np.array_equal(got, mr), ("right", b, np.argwhere(got != mr)[:4].tolist()) + what


@pytest.mark.parametrize("H,W,D", TABLE_SHAPES + WALK_SHAPES)
def test_maps_of_every_pair_and_volumes_of_the_last(smt, H, W, D):
    Ls, Rs, maps, vols = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    for call in range(2):                                  # the second call starts from the other table set
        dl, dr, status = _batch(adc, Lb, Rb)
        assert status == 0
        _check(dl, dr, maps, (call,))
    assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), vols[0].view(np.uint32))
    assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), vols[1].view(np.uint32))
    adc.close()


@pytest.mark.parametrize("K", ["1", "64"])
@pytest.mark.parametrize("H,W,D", [(6, 700, 192), (4, 1030, 192)])
def test_other_chunks_per_workgroup(smt, H, W, D, K, monkeypatch):
    """K = 1: every run is one chunk, 16-pixel walks everywhere; K = 64: a workgroup's runs follow each other on one ring"""
    Ls, Rs, maps, _ = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    monkeypatch.setenv("SMT_MAPS_CHUNKS", K)
    dl, dr, status = _batch(adc, Lb, Rb)
    assert status == 0
    _check(dl, dr, maps, (K,))
    adc.close()


def test_constant_images_first_strict_minimum(smt):
    """everything ties: hypothesis 0 must win in every pixel of both maps"""
    H, W, D = 6, 330, 192
    Lb = torch.full((3, H, W), 131.0, device="cuda:0")
    Rb = torch.full((3, H, W), 131.0, device="cuda:0")
    adc = _handle(smt, Lb, Rb, D)
    dl, dr, status = _batch(adc, Lb, Rb)
    assert status == 0
    assert np.array_equal(dl.cpu().numpy(), np.zeros((3, H, W), np.float32))
    assert np.array_equal(dr.cpu().numpy(), np.zeros((3, H, W), np.float32))
    adc.close()


@pytest.mark.parametrize("pair", [0, 1, 2])
def test_domain_flag_from_halo_and_last_row(smt, pair):
    """one out-of-domain input in one image of one pair -- its tables come from k_prep (pair 0) or from either table set's
    table workgroups (pairs 1, 2) -- sets the status flag; a clean batch after it reports clean.  0.5 in column 64, the
    right halo of tile column 0 and the first column of tile column 1; 256 in row 31, the last row of tile row 0 and the
    upper halo of tile row 1."""
    from stereo_match_traditional_amd._lib import SMT_ERR_DOMAIN
    H, W, D = 40, 330, 192
    Ls, Rs, _, _ = _case(6, 330, 192)
    clean_L = np.tile(Ls, (1, 7, 1))[:, :H]
    clean_R = np.tile(Rs, (1, 7, 1))[:, :H]
    adc = _handle(smt, _dev(clean_L), _dev(clean_R), D)
    for (i, j, value, right) in [(7, 64, 0.5, False), (31, 200, 256.0, True), (39, 329, -1.0, False)]:
        Lb, Rb = clean_L.astype(np.float32), clean_R.astype(np.float32)
        (Rb if right else Lb)[pair, i, j] = value
        _, _, status = _batch(adc, _dev(Lb), _dev(Rb))
        assert status == SMT_ERR_DOMAIN, (i, j, value)
        _, _, status = _batch(adc, _dev(clean_L), _dev(clean_R))
        assert status == 0, (i, j, value)
    adc.close()
