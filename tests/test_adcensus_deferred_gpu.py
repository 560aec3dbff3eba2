"""The last pair's volumes of smt_adcensus_compute_batch, written on first read.  While no volume pointer of a handle has
been lent, the last pair of a both-views batch with D <= 256 takes the maps-only path like the others and the handle
keeps its volumes pending; smt_adcensus_volume (GetPtrLeft / GetPtrRight) writes them with the both-views cost kernel
and from then on every batch on the handle writes its last pair's volumes itself.  Every map against the oracle's WTA,
every volume against the oracle bit for bit, at one shape per form the last pair can take."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# H, W, D: the form the deferred last pair takes
SHAPES = [(6, 80, 64),      # shared form, FULL, C = 1
          (7, 150, 70),     # shared form, C = 2, D not a multiple of 64
          (8, 262, 192),    # shared form, C = 3
          (9, 268, 200),    # two-view maps kernel (D > 192)
          (10, 280, 260)]   # generic kernel (D > 256): never deferred
NA, NB = 3, 2               # pairs of batch A (pairs 0..2 of a case) and batch B (pairs 3..4)
ENV = ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS")
_ORACLE = None


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)


def deferred(D):
    return D <= 256


@functools.lru_cache(maxsize=None)
def _case(H, W, D):
    """NA + NB pairs of one shape with the oracle's volumes and maps, computed once and shared by every test."""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 9100 + 13 * b + W, noise=(b % 2 == 1)) for b in range(NA + NB)])
    vols = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1))
            for b in range(NA + NB)]
    maps = [(O.wta(a), O.wta(c)) for a, c in vols]
    for a, c in vols:
        a.setflags(write=False); c.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), vols, maps


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _handle(smt, Lb, Rb, D, **kw):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False,
                                      store_calibration=False, **kw)


def _batch(adc, Lb, Rb):
    """ComputeBatch into maps prefilled with -1 (which no WTA writes)"""
    dl = torch.full(tuple(Lb.shape), -1.0, device=DEV)
    dr = torch.full(tuple(Lb.shape), -1.0, device=DEV)
    adc.ComputeBatch(Lb, Rb, dl, dr)
    return dl, dr


def _check_maps(dl, dr, maps, what):
    gl, gr = dl.cpu().numpy(), dr.cpu().numpy()
    for b, (ml, mr) in enumerate(maps):
        assert np.array_equal(gl[b], ml), ("left map", b) + what
        assert np.array_equal(gr[b], mr), ("right map", b) + what


def _check_vols(adc, vol, what):
    assert np.array_equal(bits(adc.GetPtrLeft()), bits(vol[0])), ("left volume",) + what
    assert np.array_equal(bits(adc.GetPtrRight()), bits(vol[1])), ("right volume",) + what


def _setup(smt, H, W, D, **kw):
    Ls, Rs, vols, maps = _case(H, W, D)
    La, Ra, Lb, Rb = T(Ls[:NA]), T(Rs[:NA]), T(Ls[NA:]), T(Rs[NA:])
    return _handle(smt, La, Ra, D, **kw), (La, Ra, vols[:NA], maps[:NA]), (Lb, Rb, vols[NA:], maps[NA:])


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_maps_then_the_last_pairs_volumes(smt, H, W, D):
    """1, 2 and 5: every pair's maps and the last pair's volumes, read once; batch A then batch B with no read in
    between gives B's last pair; a batch of one pair."""
    adc, (La, Ra, va, ma), (Lb, Rb, vb, mb) = _setup(smt, H, W, D)
    dl, dr = _batch(adc, La, Ra)
    adc.status()
    _check_maps(dl, dr, ma, ("A",))
    _check_vols(adc, va[-1], ("A",))
    adc.close()
    # a fresh handle: nothing lent between A and B
    adc = _handle(smt, La, Ra, D)
    dl, dr = _batch(adc, La, Ra)
    dl2, dr2 = _batch(adc, Lb, Rb)
    adc.status()
    _check_maps(dl, dr, ma, ("A then B",))
    _check_maps(dl2, dr2, mb, ("A then B",))
    _check_vols(adc, vb[-1], ("A then B",))
    # lent now: the eager path, a batch of one
    dl, dr = _batch(adc, La[:1], Ra[:1])
    adc.status()
    _check_maps(dl, dr, ma[:1], ("one pair, eager",))
    _check_vols(adc, va[0], ("one pair, eager",))
    adc.close()
    # a batch of one pair on a fresh handle: deferred
    adc = _handle(smt, La, Ra, D)
    dl, dr = _batch(adc, Lb[:1], Rb[:1])
    adc.status()
    _check_maps(dl, dr, mb[:1], ("one pair",))
    _check_vols(adc, vb[0], ("one pair",))
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_pointer_taken_before_the_first_compute(smt, H, W, D):
    """3: a pointer lent before any compute stays good: the batch writes its last pair's volumes itself, and the views
    made before it show them with no further call into the library."""
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    vl, vr = adc.GetPtrLeft(), adc.GetPtrRight()
    dl, dr = _batch(adc, La, Ra)
    torch.cuda.synchronize()
    assert np.array_equal(bits(vl), bits(va[-1][0])) and np.array_equal(bits(vr), bits(va[-1][1]))
    _check_maps(dl, dr, ma, ("lent first",))
    adc.status()
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_single_pairs_around_a_batch(smt, H, W, D):
    """4: batch, ComputeBoth, read gives the single pair's volumes (the pending ones are dropped); ComputeBoth, batch,
    read gives the batch's last pair."""
    adc, (La, Ra, va, ma), (Lb, Rb, vb, mb) = _setup(smt, H, W, D)      # Initialize binds pair 0 of A
    dl, dr = _batch(adc, Lb, Rb)
    sl, sr = torch.full((H, W), -1.0, device=DEV), torch.full((H, W), -1.0, device=DEV)
    adc.ComputeBoth(sl, sr)
    adc.status()
    _check_maps(dl, dr, mb, ("batch, single",))
    _check_maps(sl[None], sr[None], ma[:1], ("batch, single",))
    _check_vols(adc, va[0], ("batch, single",))
    adc.close()
    adc = _handle(smt, La, Ra, D)
    adc.ComputeBoth(sl, sr)
    dl, dr = _batch(adc, Lb, Rb)
    adc.status()
    _check_maps(dl, dr, mb, ("single, batch",))
    _check_vols(adc, vb[-1], ("single, batch",))
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_set_quirks_between_a_batch_and_its_read(smt, O, H, W, D):
    """6: set_quirks acts from the next compute on; the read gives the volumes of the pair as it was computed.  With
    the census edge fix the right volume is the mirrored left volume of the mirrored, swapped pair."""
    from stereo_match_traditional_amd import QUIRK_FIX_CENSUS_RIGHT_EDGE
    Ls, Rs, vols, maps = _case(H, W, D)
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    _batch(adc, La, Ra)
    adc.set_quirks(QUIRK_FIX_CENSUS_RIGHT_EDGE)
    adc.status()
    _check_vols(adc, va[-1], ("faithful batch, fix set before the read",))
    adc.close()
    b = NA - 1
    fixed_r = O.adcensus_view(Rs[b][:, ::-1], Ls[b][:, ::-1], D, 10.0, 30.0, 0)[:, ::-1, :]
    assert not np.array_equal(bits(fixed_r), bits(va[-1][1]))          # the fix shows in this pair
    adc = _handle(smt, La, Ra, D, quirks=QUIRK_FIX_CENSUS_RIGHT_EDGE)
    _batch(adc, La, Ra)
    adc.set_quirks(0)
    adc.status()
    _check_vols(adc, (va[-1][0], fixed_r), ("fixed batch, fix cleared before the read",))
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_batch_on_another_stream(smt, H, W, D):
    """7: the batch on a non-default stream; after a synchronise of that stream the volumes are read from the default
    one."""
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dl, dr = _batch(adc, La, Ra)
    s.synchronize()
    _check_vols(adc, va[-1], ("side stream",))
    _check_maps(dl, dr, ma, ("side stream",))
    adc.status()
    adc.close()


@pytest.mark.parametrize("read", ["never", "before the status", "after the status"])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_domain_error_is_reported_exactly_once(smt, H, W, D, read):
    """8: one non-integer pixel in the last pair: one status() reports it and the next is clean, whether the pending
    volumes are written before the first status(), after it or not at all."""
    from stereo_match_traditional_amd._lib import SmtError, SMT_ERR_DOMAIN
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    La = La.clone()
    La[-1, H // 2, W // 3] += 0.5
    _batch(adc, La, Ra)
    if read == "before the status":
        adc.GetPtrLeft()
    with pytest.raises(SmtError) as e:
        adc.status()
    assert e.value.status == SMT_ERR_DOMAIN
    if read == "after the status":
        adc.GetPtrRight()
    adc.status()
    adc.status()
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_batch_volumes_last_and_all(smt, H, W, D, monkeypatch):
    """9: SMT_BATCH_VOLUMES=last and =all give the default's maps and volumes."""
    _, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    for mode in ("last", "all", None):
        if mode: monkeypatch.setenv("SMT_BATCH_VOLUMES", mode)
        else: monkeypatch.delenv("SMT_BATCH_VOLUMES")
        adc = _handle(smt, La, Ra, D)
        dl, dr = _batch(adc, La, Ra)
        adc.status()
        _check_maps(dl, dr, ma, (mode,))
        _check_vols(adc, va[-1], (mode,))
        adc.close()


@pytest.mark.parametrize("mode", [None, "last"])
@pytest.mark.parametrize("H,W,D", SHAPES)
def test_second_read_launches_nothing(smt, H, W, D, mode, monkeypatch):
    """10: with timing on, every pair and the launch that writes pending volumes is one entry of kernel_times.  The
    first read adds one where the last pair was deferred, none where it was not (D > 256, SMT_BATCH_VOLUMES=last); a
    second read adds none and returns the same pointers; batches after it defer nothing."""
    if mode: monkeypatch.setenv("SMT_BATCH_VOLUMES", mode)
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    adc.timing(True)
    _batch(adc, La, Ra)
    assert len(adc.kernel_times()[0]) == NA
    pl, pr = adc.GetPtrLeft().data_ptr(), adc.GetPtrRight().data_ptr()
    first = NA + (1 if deferred(D) and mode is None else 0)
    assert len(adc.kernel_times()[0]) == first
    assert (adc.GetPtrLeft().data_ptr(), adc.GetPtrRight().data_ptr()) == (pl, pr)
    assert len(adc.kernel_times()[0]) == first
    _check_vols(adc, va[-1], (mode,))
    _batch(adc, La, Ra)
    _check_vols(adc, va[-1], (mode, "second batch"))
    assert len(adc.kernel_times()[0]) == first + NA
    adc.status()
    adc.close()


def test_diag_with_volumes_pending(smt):
    """11: diag on a handle whose volumes are pending (D = 64): the volumes hold the last pair's costs on return."""
    H, W, D = SHAPES[0]
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    adc.timing(True)
    _batch(adc, La, Ra)
    adc.diag(2)
    _check_vols(adc, va[-1], ("after diag",))
    assert len(adc.kernel_times()[0]) == NA                      # diag's own launches wrote them: nothing was pending
    adc.status()
    adc.close()


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_destroy_with_volumes_pending(smt, H, W, D):
    """12: destroy right after a batch whose volumes nobody read; the maps the batch wrote are complete."""
    from stereo_match_traditional_amd._lib import lib
    adc, (La, Ra, va, ma), _ = _setup(smt, H, W, D)
    dl, dr = _batch(adc, La, Ra)
    h, adc._h = adc._h, None
    assert lib().smt_adcensus_destroy(h) == 0
    torch.cuda.synchronize()
    _check_maps(dl, dr, ma, ("destroyed",))
