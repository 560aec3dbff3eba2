"""The shared maps-only form of smt_adcensus_compute_batch with the edges finished apart (adcensus_kernels.h,
k_cost_maps_shared + k_shared_finish): the left pass publishes every shareable cost, the finishing launch evaluates the
edge hypotheses W-3 <= j' + d <= W+3 of the columns j' > W-3-D and every hypothesis of the columns 0..2 and merges them
with the column's key.  Every map of every pair, NaN-prefilled, against the oracle's WTA and against the same call under
SMT_MAPS_SHARED=0 (the two-view kernel), at the smallest shapes that reach each rule and every run length; ties; edge
hypotheses that win and that tie; the census edge fix; one map requested; the deferred volumes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# H, W, D, B, SMT_MAPS_SHARED
SHAPES = [(3, 70, 64, 2, None),        # one identity column (W-3-D == 3), one chunk and a bit
          (4, 71, 64, 3, None),
          (5, 198, 192, 2, None),      # one identity column at C = 3
          (6, 259, 192, 3, None),      # (W-2-D) % 64 == 1, W % 64 == 3
          (4, 330, 192, 2, None),      # several runs per row
          (1, 500, 192, 3, None),      # H = 1
          (7, 129, 33, 2, None),       # C = 1, D no multiple of 64, W % 64 == 1
          (5, 140, 100, 3, None),      # C = 2, D no multiple of 64
          (4, 262, 256, 2, "force"),   # C = 4, one identity column
          (5, 450, 256, 2, "force")]
CHUNKS = [None, "1", "3", "64"]        # SMT_MAPS_CHUNKS
ENV = ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS")
_ORACLE = None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(mp, name, value):
    if value is None: mp.delenv(name, raising=False)
    else: mp.setenv(name, value)


def _batch(adc, Lb, Rb, maps="both"):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), float("nan"), device=Lb.device) if maps in ("both", "left") else None
    dr = torch.full((B, H, W), float("nan"), device=Lb.device) if maps in ("both", "right") else None
    adc._bind_stream()
    assert lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), B, VIEW_BOTH, _p(dl), _p(dr)) == 0
    adc.status()
    return dl, dr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _handle(smt, Lb, Rb, D, **kw):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False,
                                      store_calibration=False, **kw)


@functools.lru_cache(maxsize=None)
def _case(H, W, D, B):
    """images, the oracle's maps of every pair and its volumes of the last pair, computed once per shape"""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 6300 + 11 * b + W, noise=(b % 2 == 0)) for b in range(B)])
    vols = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1)) for b in range(B)]
    maps = [(O.wta(a), O.wta(c)) for a, c in vols]
    for a, c in vols:
        a.setflags(write=False); c.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), maps, vols[-1]


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, maps, what):
    for b, (ml, mr) in enumerate(maps):
        got = dl[b].cpu().numpy()
        assert np.array_equal(got, ml), ("left", b, np.argwhere(got != ml)[:4].tolist()) + what
        got = dr[b].cpu().numpy()
        assert np.array_equal(got, mr), ("right", b, np.argwhere(got != mr)[:4].tolist()) + what


@pytest.mark.parametrize("H,W,D,B,form", SHAPES)
def test_batch_against_the_oracle_and_the_other_forms(smt, H, W, D, B, form, monkeypatch):
    Ls, Rs, maps, _ = _case(H, W, D, B)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    for K in CHUNKS:
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        dl, dr = _batch(adc, Lb, Rb)
        _check(dl, dr, maps, (K, "finish"))
        monkeypatch.setenv("SMT_MAPS_SHARED", "0")
        dl0, dr0 = _batch(adc, Lb, Rb)
        _env(monkeypatch, "SMT_MAPS_SHARED", form)
        for a, b in ((dl, dl0), (dr, dr0)):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), K
        # the key map was left reset: the same call again gives the same maps
        dl2, dr2 = _batch(adc, Lb, Rb)
        assert np.array_equal(dl.cpu().numpy(), dl2.cpu().numpy()) and np.array_equal(dr.cpu().numpy(), dr2.cpu().numpy()), K
    adc.close()


@pytest.mark.parametrize("H,W,D,form", [(4, 330, 192, None), (3, 70, 64, None), (5, 140, 100, None), (4, 262, 256, "force")])
def test_constant_images_tie_everywhere(smt, H, W, D, form, monkeypatch):
    """every cost of a pixel is equal, edge hypotheses included: both maps are 0 everywhere"""
    Lb = torch.full((2, H, W), 77.0, device="cuda:0")
    Rb = torch.full((2, H, W), 77.0, device="cuda:0")
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    for K in CHUNKS:
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        dl, dr = _batch(adc, Lb, Rb)
        assert np.array_equal(dl.cpu().numpy(), np.zeros((2, H, W), np.float32)), K
        assert np.array_equal(dr.cpu().numpy(), np.zeros((2, H, W), np.float32)), K
    adc.close()


def edge_pair(H, W, s, a, seed):
    """Rows 0 .. H/2-1: R[x] = L[x + s], so the right pixels with W-3 <= x + s <= W-1 match a left pixel whose
    hypothesis is an edge one.  The other rows: R is 90 from column `a` on and L from column a + s on, so a right pixel
    x >= a + 3 has the same cost at every hypothesis that lands in L's flat part, shared (x + d <= W-4) and edge ones
    (L's column 0, which the reference's census reads for neighbours past the right edge, is 90 there too)."""
    rs = np.random.RandomState(seed)
    L = rs.randint(0, 256, (H, W)).astype(np.float32)
    R = rs.randint(0, 256, (H, W)).astype(np.float32)
    h = H // 2
    R[:h, :W - s] = L[:h, s:]
    R[h:, a:] = 90.0
    L[h:, a + s:] = 90.0
    L[h:, 0] = 90.0
    return L, R


def edge_stats(volL, volR, W, D):
    """(right pixels whose first minimum is an edge hypothesis, right pixels of the columns 3 .. W-4 where the smallest
    edge cost equals the smallest shared cost) of a pair of oracle volumes"""
    wins = ties = 0
    for c in range(3, W):
        lo, hi = max(0, W - 3 - c), min(D - 1, W + 3 - c)
        if lo > hi:
            continue
        edge = volR[:, c, lo:hi + 1].min(axis=1)
        if c > W - 4:
            continue
        shared = np.stack([volL[:, c + d, d] for d in range(min(D, W - 3 - c))], axis=1).min(axis=1)
        wins += int((edge < shared).sum())
        ties += int((edge == shared).sum())
    return wins, ties


@pytest.mark.parametrize("H,W,D,form", [(12, 330, 192, None), (10, 140, 100, None), (10, 300, 256, "force")])
def test_edge_hypotheses_that_win_and_that_tie(smt, O, H, W, D, form, monkeypatch):
    pairs = [edge_pair(H, W, 10 + 3 * b, W - 45, 70 + b + W) for b in range(2)]
    vols = [(O.adcensus_view(L, R, D, 10.0, 30.0, 0), O.adcensus_view(L, R, D, 10.0, 30.0, 1)) for L, R in pairs]
    for volL, volR in vols:
        wins, ties = edge_stats(volL, volR, W, D)
        assert wins >= 3 and ties >= 3, (wins, ties)          # the pair does what it was built for
    Lb, Rb = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    for K in CHUNKS:
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        dl, dr = _batch(adc, Lb, Rb)
        _check(dl, dr, [(O.wta(a), O.wta(c)) for a, c in vols], (K,))
    adc.close()


@pytest.mark.parametrize("fix", [False, True])
def test_census_right_edge_fix(smt, O, fix, monkeypatch):
    """SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE changes the left census at the columns >= W-3, which only edge hypotheses read"""
    from stereo_match_traditional_amd import QUIRK_FIX_CENSUS_RIGHT_EDGE
    H, W, D = 12, 330, 192
    rs = np.random.RandomState(412)
    Lb = _dev(rs.randint(0, 256, (3, H, W)))
    Rb = _dev(rs.randint(0, 256, (3, H, W)))
    adc = _handle(smt, Lb, Rb, D, quirks=QUIRK_FIX_CENSUS_RIGHT_EDGE if fix else 0)
    dl, dr = _batch(adc, Lb, Rb)
    monkeypatch.setenv("SMT_MAPS_SHARED", "0")
    dl0, dr0 = _batch(adc, Lb, Rb)
    monkeypatch.delenv("SMT_MAPS_SHARED")
    for a, b in ((dl, dl0), (dr, dr0)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    if fix:
        # the right map is the mirrored, swapped pair's left map
        mirror = _handle(smt, Lb, Rb, D, quirks=0)
        ml, _ = _batch(mirror, Rb.flip(2).contiguous(), Lb.flip(2).contiguous())
        assert np.array_equal(dr.cpu().numpy(), ml.flip(2).cpu().numpy())
        mirror.close()
    else:
        for b in range(3):
            L, R = Lb[b].cpu().numpy(), Rb[b].cpu().numpy()
            assert np.array_equal(dr[b].cpu().numpy(), O.wta(O.adcensus_view(L, R, D, 10.0, 30.0, 1))), b
            assert np.array_equal(dl[b].cpu().numpy(), O.wta(O.adcensus_view(L, R, D, 10.0, 30.0, 0))), b
    adc.close()


@pytest.mark.parametrize("H,W,D,B,form", [(6, 259, 192, 3, None), (5, 140, 100, 3, None), (4, 262, 256, 2, "force")])
def test_one_map_and_the_deferred_volumes(smt, H, W, D, B, form, monkeypatch):
    Ls, Rs, maps, vol = _case(H, W, D, B)
    Lb, Rb = _dev(Ls), _dev(Rs)
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    for m in ("left", "right", "both"):
        adc = _handle(smt, Lb, Rb, D)
        dl, dr = _batch(adc, Lb, Rb, m)
        for b in range(B):
            if dl is not None: assert np.array_equal(dl[b].cpu().numpy(), maps[b][0]), (m, b)
            if dr is not None: assert np.array_equal(dr[b].cpu().numpy(), maps[b][1]), (m, b)
        # the last pair's volumes, written on first read
        assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), vol[1].view(np.uint32)), m
        assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), vol[0].view(np.uint32)), m
        adc.close()
