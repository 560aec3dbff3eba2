"""The shared maps-only form of smt_adcensus_compute_batch with a pair finished inside its neighbours' launches
(adcensus_kernels.h, k_cost_maps_shared): the edge items of a pair ride in its own launch, the conversion of its partial keys
in the next pair's, and only the last shared pair of a call is converted by a launch of its own (k_shared_convert).
Every map of every pair, NaN-prefilled, against the oracle's WTA: several batches on one handle (key-map parity across
calls, the lone pair, a carried pair beside a stand-alone one), the other forms between shared calls, no write behind a
call's return, edge hypotheses that win and that tie.  SMT_SHARED_FINISH=apart keeps one conversion launch per pair."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# H, W, D, SMT_MAPS_SHARED
SHAPES = [(5, 198, 192, None),         # one identity column, columns 0..2
          (6, 259, 192, None),         # a 3-pixel last chunk
          (6, 330, 192, None),         # a 4-chunk run and a row change in a workgroup
          (5, 140, 100, None),         # C = 2, ragged D
          (7, 129, 33, None),          # C = 1
          (4, 262, 256, "force")]      # C = 4
BATCHES = (3, 1, 2, 5, 3)
ENV = ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS", "SMT_SHARED_FINISH")
_ORACLE = None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(mp, name, value):
    if value is None: mp.delenv(name, raising=False)
    else: mp.setenv(name, value)


def _batch_into(adc, Lb, Rb, dl, dr):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    adc._bind_stream()
    assert lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), Lb.shape[0], VIEW_BOTH, _p(dl), _p(dr)) == 0
    adc.status()                                           # synchronises the stream


def _batch(adc, Lb, Rb, maps="both"):
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), float("nan"), device=Lb.device) if maps in ("both", "left") else None
    dr = torch.full((B, H, W), float("nan"), device=Lb.device) if maps in ("both", "right") else None
    _batch_into(adc, Lb, Rb, dl, dr)
    return dl, dr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _handle(smt, Lb, Rb, D):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False, store_calibration=False)


@functools.lru_cache(maxsize=None)
def _case(H, W, D, B):
    """B different pairs, the oracle's maps of each and its volumes of each, computed once per shape"""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 9100 + 13 * b + W, noise=(b % 2 == 0)) for b in range(B)])
    vols = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1)) for b in range(B)]
    maps = [(O.wta(a), O.wta(c)) for a, c in vols]
    for a, c in vols:
        a.setflags(write=False); c.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), maps, vols


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, maps, what):
    for b, (ml, mr) in enumerate(maps):
        if dl is not None:
            got = dl[b].cpu().numpy()
            assert np.array_equal(got, ml), ("left", b, np.argwhere(got != ml)[:4].tolist()) + what
        if dr is not None:
            got = dr[b].cpu().numpy()
            assert np.array_equal(got, mr), ("right", b, np.argwhere(got != mr)[:4].tolist()) + what


@pytest.mark.parametrize("H,W,D,form", SHAPES)
def test_several_batches_on_one_handle(smt, H, W, D, form, monkeypatch):
    """batches of 3, 1, 2, 5 and 3 pairs, different images in every pair, one handle for every schedule"""
    Ls, Rs, maps, _ = _case(H, W, D, sum(BATCHES))
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    for K in (None, "1", "64"):
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        for overlap in (None, "0", "1", "2"):
            _env(monkeypatch, "SMT_OVERLAP", overlap)
            got = {}
            for finish in (None, "apart"):
                _env(monkeypatch, "SMT_SHARED_FINISH", finish)
                outs, o = [], 0
                for n in BATCHES:
                    dl, dr = _batch(adc, Lb[o:o + n], Rb[o:o + n])
                    _check(dl, dr, maps[o:o + n], (K, overlap, finish, o))
                    outs.append((dl.cpu().numpy(), dr.cpu().numpy()))
                    o += n
                got[finish] = outs
            for (a, b), (c, d) in zip(got[None], got["apart"]):
                assert np.array_equal(a, c) and np.array_equal(b, d), (K, overlap)
    adc.close()


@pytest.mark.parametrize("H,W,D", [(6, 259, 192), (5, 140, 100)])
def test_other_forms_between_shared_calls(smt, H, W, D, monkeypatch):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    B = 3
    Ls, Rs, maps, vols = _case(H, W, D, sum(BATCHES))
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    o = 0

    def call(what, env=(), which="both"):
        nonlocal o
        for name, value in env:
            monkeypatch.setenv(name, value)
        dl, dr = _batch(adc, Lb[o:o + B], Rb[o:o + B], which)
        for name, _ in env:
            monkeypatch.delenv(name)
        _check(dl, dr, maps[o:o + B], (what, o))
        o += 1                                             # other pairs in every call

    call("shared 1")
    call("two-view", [("SMT_MAPS_SHARED", "0")])
    call("shared 2")
    call("all volumes", [("SMT_BATCH_VOLUMES", "all")])
    call("shared 3")
    # one single pair: an odd number of pairs shifts the parity of the table sets and of the key maps
    dl = torch.full((H, W), float("nan"), device="cuda:0")
    dr = torch.full((H, W), float("nan"), device="cuda:0")
    adc._bind_stream()
    assert lib().smt_adcensus_compute(adc._h, _p(Lb[o]), _p(Rb[o]), VIEW_BOTH, _p(dl), _p(dr)) == 0
    adc.status()
    _check(dl[None], dr[None], maps[o:o + 1], ("single",))
    call("shared 4")
    call("right map only", which="right")
    call("shared 5")
    last = o - 1 + B - 1
    assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), vols[last][1].view(np.uint32))
    assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), vols[last][0].view(np.uint32))
    adc.close()


@pytest.mark.parametrize("finish", [None, "apart"])
def test_no_write_behind_the_return(smt, finish, monkeypatch):
    """call A into X; X refilled with NaN; call B into Y: nothing of A is still pending, and nothing lands beside a map"""
    H, W, D, B = 6, 330, 192, 3
    Ls, Rs, maps, _ = _case(H, W, D, sum(BATCHES))
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_SHARED_FINISH", finish)
    G, n = 4096, B * H * W
    nan = float("nan")

    def guarded():
        buf = torch.full((G + n + G,), nan, device="cuda:0")
        return buf, buf[G:G + n].view(B, H, W)

    xl, XL = guarded()
    xr, XR = guarded()
    _batch_into(adc, Lb[:B], Rb[:B], XL, XR)
    torch.cuda.synchronize()
    _check(XL, XR, maps[:B], ("A",))
    xl.fill_(nan); xr.fill_(nan)
    torch.cuda.synchronize()
    yl, YL = guarded()
    yr, YR = guarded()
    _batch_into(adc, Lb[B:2 * B], Rb[B:2 * B], YL, YR)
    torch.cuda.synchronize()
    _check(YL, YR, maps[B:2 * B], ("B",))
    assert bool(torch.isnan(xl).all()) and bool(torch.isnan(xr).all())
    for buf in (yl, yr):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())
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


@pytest.mark.parametrize("H,W,D", [(12, 330, 192), (10, 140, 100)])
def test_edge_hypotheses_that_win_and_that_tie(smt, O, H, W, D, monkeypatch):
    pairs = [edge_pair(H, W, 10 + 3 * b, W - 45, 70 + b + W) for b in range(3)]
    vols = [(O.adcensus_view(L, R, D, 10.0, 30.0, 0), O.adcensus_view(L, R, D, 10.0, 30.0, 1)) for L, R in pairs]
    for volL, volR in vols:
        wins, ties = edge_stats(volL, volR, W, D)
        assert wins >= 3 and ties >= 3, (wins, ties)          # the pair does what it was built for
    want = [(O.wta(a), O.wta(c)) for a, c in vols]
    Lb, Rb = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    adc = _handle(smt, Lb, Rb, D)
    for finish in (None, "apart"):
        _env(monkeypatch, "SMT_SHARED_FINISH", finish)
        for K in (None, "1", "64"):
            _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
            dl, dr = _batch(adc, Lb, Rb)
            _check(dl, dr, want, (finish, K))
    adc.close()


@pytest.mark.parametrize("H,W,D", [(12, 330, 192), (10, 140, 100)])
def test_constant_images_tie_everywhere(smt, H, W, D, monkeypatch):
    """every cost of a pixel is equal, edge hypotheses included: both maps are 0 everywhere"""
    Lb = torch.full((3, H, W), 77.0, device="cuda:0")
    Rb = torch.full((3, H, W), 77.0, device="cuda:0")
    adc = _handle(smt, Lb, Rb, D)
    for finish in (None, "apart"):
        _env(monkeypatch, "SMT_SHARED_FINISH", finish)
        dl, dr = _batch(adc, Lb, Rb)
        assert np.array_equal(dl.cpu().numpy(), np.zeros((3, H, W), np.float32)), finish
        assert np.array_equal(dr.cpu().numpy(), np.zeros((3, H, W), np.float32)), finish
    adc.close()
