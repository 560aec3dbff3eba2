"""The chained schedule of smt_adcensus_compute_batch (adcensus_rules.h, chain_plan): pair b of a call runs on chain b % NC,
every chain on two table sets and two key maps of its own, chain 0 on the caller's stream and the others on internal
streams that are forked from it and joined into it by events.  Every map of every pair, NaN-prefilled, against the
oracle's WTA, and every form bit-equal to every other: batches of several sizes on one handle (chain counters of every
parity), the schedules, chain counts and device orders (SMT_OVERLAP, SMT_CHAINS, SMT_CHAIN_ORDER), single pairs and the
other forms between chained batches, the last pair's volumes from either chain, a busy caller's stream with late inputs
and an on-stream reader right behind the call (the fork and the join edge), guard bands, and the timing entries."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import stream_order_cases as SC

pytestmark = pytest.mark.gpu

# H, W, D; none forced: (4, 262, 256) takes the two-view kernel k_cost_maps2p, the others the shared form
SHAPES = [(6, 330, 192),           # a 4-chunk run and a row change in a workgroup
          (5, 140, 100),           # C = 2, ragged D
          (7, 129, 33),            # C = 1
          (4, 262, 256)]           # the two-view kernel: chains without key maps
BATCHES = (3, 1, 2, 5, 8, 4)       # odd and even sizes and a single pair: the chains' counters take every parity
ENV = ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS", "SMT_SHARED_FINISH",
       "SMT_CHAINS", "SMT_CHAIN_ORDER", "SMT_CHAIN_FORK", "SMT_MAPS_TAPER")
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


def _batch(adc, Lb, Rb):
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), float("nan"), device=Lb.device)
    dr = torch.full((B, H, W), float("nan"), device=Lb.device)
    _batch_into(adc, Lb, Rb, dl, dr)
    return dl, dr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _handle(smt, Lb, Rb, D):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False, store_calibration=False)


@functools.lru_cache(maxsize=None)
def _case(H, W, D):
    """sum(BATCHES) different pairs, the oracle's volumes and maps of each, computed once per shape"""
    O, B = _ORACLE, sum(BATCHES)
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 7300 + 11 * b + W, noise=(b % 2 == 0)) for b in range(B)])
    vols = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1)) for b in range(B)]
    for a, c in vols:
        a.setflags(write=False); c.setflags(write=False)
    mapL = np.stack([O.wta(a) for a, _ in vols])
    mapR = np.stack([O.wta(c) for _, c in vols])
    mapL.setflags(write=False); mapR.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), mapL, mapR, vols


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, mapL, mapR, what):
    for side, got, want in (("left", dl.cpu().numpy(), mapL), ("right", dr.cpu().numpy(), mapR)):
        assert np.array_equal(got, want), (side, np.argwhere(got != want)[:4].tolist()) + tuple(what)


def _run_batches(adc, Lb, Rb, mapL, mapR, what):
    outs, o = [], 0
    for n in BATCHES:
        dl, dr = _batch(adc, Lb[o:o + n], Rb[o:o + n])
        _check(dl, dr, mapL[o:o + n], mapR[o:o + n], what + (o,))
        outs.append((dl, dr))
        o += n
    return torch.cat([a for a, _ in outs]).cpu().numpy(), torch.cat([b for _, b in outs]).cpu().numpy()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_batches_on_one_handle_under_every_form(smt, H, W, D, monkeypatch):
    """batches of 3, 1, 2, 5, 8 and 4 pairs, different images in every pair, one handle for every form"""
    Ls, Rs, mapL, mapR, _ = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    first = None
    for overlap, chains, order, K in itertools.product((None, "3", "2"), (None, "2", "3"), (None, "pairs", "ab", "ba"),
                                                       (None, "1")):
        _env(monkeypatch, "SMT_OVERLAP", overlap)
        _env(monkeypatch, "SMT_CHAINS", chains)
        _env(monkeypatch, "SMT_CHAIN_ORDER", order)
        _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
        got = _run_batches(adc, Lb, Rb, mapL, mapR, (overlap, chains, order, K))
        if first is None:
            first = got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (overlap, chains, order, K)
    adc.close()


@pytest.mark.parametrize("chains", [None, "3"])
def test_single_pair_between_chained_batches(smt, chains, monkeypatch):
    """smt_adcensus_compute runs on chain 0's state and shifts its parity alone"""
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    H, W, D = 6, 330, 192
    Ls, Rs, mapL, mapR, _ = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_CHAINS", chains)
    o = 0
    for n in (4, 0, 5, 0, 0, 3, 2):                        # 0: one smt_adcensus_compute
        if n:
            dl, dr = _batch(adc, Lb[o:o + n], Rb[o:o + n])
        else:
            n = 1
            dl = torch.full((1, H, W), float("nan"), device="cuda:0")
            dr = torch.full((1, H, W), float("nan"), device="cuda:0")
            adc._bind_stream()
            assert lib().smt_adcensus_compute(adc._h, _p(Lb[o]), _p(Rb[o]), VIEW_BOTH, _p(dl), _p(dr)) == 0
            adc.status()
        _check(dl, dr, mapL[o:o + n], mapR[o:o + n], (chains, o))
        o += n
    adc.close()


@pytest.mark.parametrize("H,W,D", [(6, 330, 192), (5, 140, 100)])
def test_other_forms_between_chained_batches(smt, H, W, D, monkeypatch):
    Ls, Rs, mapL, mapR, vols = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    o = 0

    def call(what, B, env=()):
        nonlocal o
        for name, value in env:
            monkeypatch.setenv(name, value)
        dl, dr = _batch(adc, Lb[o:o + B], Rb[o:o + B])
        for name, _ in env:
            monkeypatch.delenv(name)
        _check(dl, dr, mapL[o:o + B], mapR[o:o + B], (what, o))
        o += 1                                             # other pairs in every call

    call("chained 1", 3)
    call("two-view", 3, [("SMT_MAPS_SHARED", "0")])        # chained too, without key maps
    call("chained 2", 4)
    call("all volumes", 3, [("SMT_BATCH_VOLUMES", "all")])  # keeps the fused schedule: every pair stores the volumes
    call("chained 3", 5)
    call("fused", 3, [("SMT_OVERLAP", "2")])
    call("internal stream", 3, [("SMT_OVERLAP", "1")])     # the table stream is chain 1's stream
    call("chained 4", 2)
    last = o - 1 + 2 - 1
    assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), vols[last][1].view(np.uint32))
    assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), vols[last][0].view(np.uint32))
    adc.close()


@pytest.mark.parametrize("chains", [None, "3"])
@pytest.mark.parametrize("H,W,D", [(6, 330, 192), (4, 262, 256)])
def test_volumes_of_the_last_pair(smt, H, W, D, chains, monkeypatch):
    """an even and an odd batch (the last pair on chain 1 and on chain 0 of two); first deferred -- written by the first
    GetPtr* from the last pair's table set -- then, the pointers lent, by the batch itself on the last pair's stream"""
    Ls, Rs, mapL, mapR, vols = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    _env(monkeypatch, "SMT_CHAINS", chains)

    def volumes_equal(adc, b, what):
        for view, got in ((0, adc.GetPtrLeft()), (1, adc.GetPtrRight())):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), vols[b][view].view(np.uint32)), (view, b) + what

    for first in (4, 3, 5, 6):
        adc = _handle(smt, Lb, Rb, D)
        o = 0
        for n in (first, 4, 3, 2):                         # the first call deferred, the others on a lent handle
            dl, dr = _batch(adc, Lb[o:o + n], Rb[o:o + n])
            _check(dl, dr, mapL[o:o + n], mapR[o:o + n], (first, n, o))
            volumes_equal(adc, o + n - 1, (first, n, o))
            o += n
        adc.close()


@pytest.mark.parametrize("chains", [None, "3"])
def test_busy_stream_late_inputs_and_a_reader_right_behind(smt, chains, monkeypatch):
    """The caller's stream sleeps; the inputs hold decoys until an on-stream copy behind the sleep brings the data (the
    fork edge: no chain may start before it).  The entry returns while the stream is busy, and an on-stream copy of both
    maps enqueued right behind the call, with no synchronisation, holds the oracle's maps (the join edge)."""
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    H, W, D, B = 6, 330, 192, 5
    Ls, Rs, mapL, mapR, _ = _case(H, W, D)
    data_l, data_r = _dev(Ls[:B]), _dev(Rs[:B])
    adc = _handle(smt, data_l, data_r, D)
    _env(monkeypatch, "SMT_CHAINS", chains)
    nan = float("nan")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):                                     # a first call on the handle and a warm one
        Lb = data_l.flip(0).flip(2).contiguous()           # decoys: admissible images, other maps
        Rb = data_r.flip(0).flip(2).contiguous()
        dl = torch.full((B, H, W), nan, device="cuda:0")
        dr = torch.full((B, H, W), nan, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(SC.DELAY)
            slept = torch.cuda.Event()
            slept.record()
            Lb.copy_(data_l, non_blocking=True)
            Rb.copy_(data_r, non_blocking=True)
            adc._bind_stream()
            rc = lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), B, VIEW_BOTH, _p(dl), _p(dr))
            busy = not slept.query()
            snap_l, snap_r = dl.clone(), dr.clone()        # on the stream, right behind the call
        side.synchronize()
        assert rc == 0
        assert busy, "the entry waited for the caller's stream"
        _check(snap_l, snap_r, mapL[:B], mapR[:B], (chains,))
    torch.cuda.synchronize()
    adc.close()


@pytest.mark.parametrize("chains,order", [(None, None), ("3", None), (None, "ba")])
def test_no_write_behind_the_return_or_beside_a_map(smt, chains, order, monkeypatch):
    """call A into X; X refilled with NaN; call B into Y: nothing of A is still pending, and nothing lands beside a map"""
    H, W, D, B = 6, 330, 192, 5
    Ls, Rs, mapL, mapR, _ = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_CHAINS", chains)
    _env(monkeypatch, "SMT_CHAIN_ORDER", order)
    G, n = 4096, B * H * W
    nan = float("nan")

    def guarded():
        buf = torch.full((G + n + G,), nan, device="cuda:0")
        return buf, buf[G:G + n].view(B, H, W)

    xl, XL = guarded()
    xr, XR = guarded()
    _batch_into(adc, Lb[:B], Rb[:B], XL, XR)
    torch.cuda.synchronize()
    _check(XL, XR, mapL[:B], mapR[:B], ("A",))
    xl.fill_(nan); xr.fill_(nan)
    torch.cuda.synchronize()
    yl, YL = guarded()
    yr, YR = guarded()
    _batch_into(adc, Lb[B:2 * B], Rb[B:2 * B], YL, YR)
    torch.cuda.synchronize()
    _check(YL, YR, mapL[B:2 * B], mapR[B:2 * B], ("B",))
    assert bool(torch.isnan(xl).all()) and bool(torch.isnan(xr).all())
    for buf in (yl, yr):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())
    adc.close()


@pytest.mark.parametrize("chains", [None, "3"])
def test_one_timing_entry_per_timed_pair(smt, chains, monkeypatch):
    H, W, D = 6, 330, 192
    Ls, Rs, mapL, mapR, _ = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    _env(monkeypatch, "SMT_CHAINS", chains)
    adc.timing(True)
    o = 0
    for n in (5, 4):
        dl, dr = _batch(adc, Lb[o:o + n], Rb[o:o + n])
        _check(dl, dr, mapL[o:o + n], mapR[o:o + n], (chains, o))
        o += n
        prep_ms, cost_ms = adc.kernel_times()
        assert len(prep_ms) == len(cost_ms) == o
        assert all(np.isfinite(t) and t >= 0 for t in prep_ms) and all(np.isfinite(t) and t > 0 for t in cost_ms)
    adc.timing(2)                                          # every second pair
    dl, dr = _batch(adc, Lb[o:o + 6], Rb[o:o + 6])
    _check(dl, dr, mapL[o:o + 6], mapR[o:o + 6], (chains, "stride"))
    assert len(adc.kernel_times()[1]) == 3
    adc.close()
