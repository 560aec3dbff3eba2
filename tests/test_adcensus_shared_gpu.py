"""The shared maps-only form of smt_adcensus_compute_batch (adcensus_kernels.h, k_cost_maps_shared + k_shared_finish): the right
map of the columns 3 <= j' <= W-3-D comes from the keys the left pass publishes, the other columns from the VIEW 1 body.
Every map of every pair against the oracle's WTA and against the same call under SMT_MAPS_SHARED=0 (the two-view
kernel), under every batch schedule and run length; ties at run edges; the census edge fix; one / no map requested and
the last pair's volumes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# H, W, D, B
SHAPES = [(9, 70, 256, 2),        # identity set empty: the two-view kernel serves it
          (8, 198, 192, 3),       # exactly one shared column
          (18, 330, 192, 3),      # several runs, edge merges
          (21, 200, 100, 3),      # D not a multiple of 64
          (24, 200, 64, 4),       # C = 1
          (5, 450, 256, 2)]       # C = 4
SCHEDS = ["0", "1", "2", None]    # SMT_OVERLAP
CHUNKS = [None, "1", "3", "64"]   # SMT_MAPS_CHUNKS
# SMT_MAPS_SHARED: unset is the host's choice per shape (the shared form for D <= 192), "force" the shared form wherever
# the identity set is not empty, so that four hypotheses per lane (D = 256) run it too
FORMS = [None, "force"]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(mp, name, value):
    if value is None: mp.delenv(name, raising=False)
    else: mp.setenv(name, value)


def _batch(adc, Lb, Rb, maps="both"):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), -1.0, device=Lb.device) if maps in ("both", "left") else None
    dr = torch.full((B, H, W), -1.0, device=Lb.device) if maps in ("both", "right") else None
    adc._bind_stream()
    assert lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), B, VIEW_BOTH, _p(dl), _p(dr)) == 0
    adc.status()
    return dl, dr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


_ORACLE = None


@functools.lru_cache(maxsize=None)
def _case(H, W, D, B):
    """images and the oracle's volumes of the last pair and maps of every pair, computed once per shape"""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 5200 + 7 * b + W, noise=(b % 2 == 0)) for b in range(B)])
    vols = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1)) for b in range(B)]
    maps = [(O.wta(a), O.wta(c)) for a, c in vols]
    return np.stack(Ls), np.stack(Rs), maps, vols[-1]


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS"):
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, maps, what):
    for b, (ml, mr) in enumerate(maps):
        assert np.array_equal(dl[b].cpu().numpy(), ml), ("left", b) + what
        got = dr[b].cpu().numpy()
        bad = np.argwhere(got != mr)
        assert bad.size == 0, ("right", b, bad[:4].tolist()) + what


@pytest.mark.parametrize("H,W,D,B", SHAPES)
def test_shared_batch_against_the_oracle(smt, H, W, D, B, monkeypatch):
    Ls, Rs, maps, _ = _case(H, W, D, B)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    for sched in SCHEDS:
        _env(monkeypatch, "SMT_OVERLAP", sched)
        for K in CHUNKS:
            _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
            for form in FORMS:
                _env(monkeypatch, "SMT_MAPS_SHARED", form)
                dl, dr = _batch(adc, Lb, Rb)
                _check(dl, dr, maps, (sched, K, form))
            if K in (None, "3"):
                monkeypatch.setenv("SMT_MAPS_SHARED", "0")
                dl0, dr0 = _batch(adc, Lb, Rb)
                monkeypatch.delenv("SMT_MAPS_SHARED")
                assert torch.equal(dl, dl0) and torch.equal(dr, dr0), (sched, K)
    adc.close()


@pytest.mark.parametrize("H,W,D,B", SHAPES)
def test_one_or_no_map_and_the_last_pairs_volumes(smt, H, W, D, B, monkeypatch):
    Ls, Rs, maps, vol = _case(H, W, D, B)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    monkeypatch.setenv("SMT_MAPS_SHARED", "force")
    for m in ("both", "left", "right", "none"):
        dl, dr = _batch(adc, Lb, Rb, m)
        for b in range(B):
            if dl is not None: assert np.array_equal(dl[b].cpu().numpy(), maps[b][0]), (m, b)
            if dr is not None: assert np.array_equal(dr[b].cpu().numpy(), maps[b][1]), (m, b)
        assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), vol[0].view(np.uint32)), m
        assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), vol[1].view(np.uint32)), m
    adc.close()


@pytest.mark.parametrize("H,W,D", [(6, 330, 192), (5, 450, 256), (7, 200, 100)])
def test_constant_images_tie_everywhere(smt, H, W, D, monkeypatch):
    """every cost of a pixel is equal: both maps are 0 everywhere, at every run edge too"""
    Lb = torch.full((3, H, W), 77.0, device="cuda:0")
    Rb = torch.full((3, H, W), 77.0, device="cuda:0")
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    monkeypatch.setenv("SMT_MAPS_SHARED", "force")
    for K in CHUNKS:
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        dl, dr = _batch(adc, Lb, Rb)
        assert not dl.any() and not dr.any(), K
    adc.close()


@pytest.mark.parametrize("K", ["1", "2", None])
def test_equal_best_costs_in_different_runs(smt, O, K, monkeypatch):
    """Rows of period 64 and R[x] = L[x + 5]: a right pixel's cost is the same (zero) at d = 5, 69 and 133, whose left
    columns lie in three different chunks -- three different runs with one chunk per workgroup.  The smallest d wins."""
    H, W, D, B = 12, 330, 192, 3
    rs = np.random.RandomState(11)
    Ls, Rs = [], []
    for b in range(B):
        base = rs.randint(0, 256, (H, 64))
        L = np.tile(base, (1, 7))[:, :W + 5]
        Ls.append(L[:, :W]); Rs.append(L[:, 5:W + 5])
    Lb, Rb = _dev(np.stack(Ls)), _dev(np.stack(Rs))
    _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    dl, dr = _batch(adc, Lb, Rb)
    for b in range(B):
        want = O.wta(O.adcensus_view(Ls[b].astype(np.float32), Rs[b].astype(np.float32), D, 10.0, 30.0, 1))
        assert (want[4:H - 4, 3:W - 3 - D + 1] == 5).all()                 # the tie is there, away from the image border
        assert np.array_equal(dr[b].cpu().numpy(), want), b
        assert np.array_equal(dl[b].cpu().numpy(), O.wta(O.adcensus_view(Ls[b].astype(np.float32), Rs[b].astype(np.float32), D, 10.0, 30.0, 0))), b
    adc.close()


@pytest.mark.parametrize("H,W,D", [(12, 330, 192), (9, 210, 64)])
def test_census_right_edge_fix(smt, H, W, D, monkeypatch):
    """SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE changes the left census only at columns >= W-3, outside the identity set: the
    shared form gives the two-view kernel's maps, and the right map is the mirrored, swapped pair's left map."""
    from stereo_match_traditional_amd import QUIRK_FIX_CENSUS_RIGHT_EDGE
    rs = np.random.RandomState(300 + W)
    Lb = _dev(rs.randint(0, 256, (3, H, W)))
    Rb = _dev(rs.randint(0, 256, (3, H, W)))
    kw = dict(placement_search=False, store_calibration=False)
    fixed = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, quirks=QUIRK_FIX_CENSUS_RIGHT_EDGE, **kw)
    mirror = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, quirks=0, **kw)
    dl, dr = _batch(fixed, Lb, Rb)
    monkeypatch.setenv("SMT_MAPS_SHARED", "0")
    dl0, dr0 = _batch(fixed, Lb, Rb)
    ml, _ = _batch(mirror, Rb.flip(2).contiguous(), Lb.flip(2).contiguous())
    monkeypatch.delenv("SMT_MAPS_SHARED")
    assert torch.equal(dl, dl0) and torch.equal(dr, dr0)
    assert torch.equal(dr, ml.flip(2))
    fixed.close(); mirror.close()
