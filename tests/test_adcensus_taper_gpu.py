"""Tapered tail of the maps-only launches of smt_adcensus_compute_batch (adcensus_rules.h: maps_span, fused_grid's body
placement): the slice's last n1 workgroups take 1 chunk, the n2 before them max(1, K/2), and the auxiliary workgroups
(table tiles, conversion and edge items) go in front of the first tapered one.  Maps must not depend on it: every map of a
3-pair batch on one reused handle -- so that the table tiles and the carried conversion pass through the new placement --
NaN-prefilled, bit for bit against the oracle's adcensus_view + wta, under forced tapers (SMT_MAPS_TAPER=n2,n1), with K
unset and 8, for the shared form, the two-view kernel (SMT_MAPS_SHARED=0) and its rank mode, and the domain flag clear.

Every case first asserts, on a Python recomputation of the span rule kept here, that the shape does taper: some slice has
a 1-chunk group of the tail behind a longer group.  The slices of these shapes have 5 to 22 chunks, so a group has all K
chunks only where per >= K + the tails: test_every_taper_and_k_has_a_strict_case asserts that every taper, K and kernel
family has such a case (a K-chunk group and a 1-chunk group in one slice); the taller shape (12, 700, 192) is there for
K = 8 in the shared form."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
ENV = ("SMT_MAPS_SHARED", "SMT_MAPS_KERNEL", "SMT_BATCH_VOLUMES", "SMT_OVERLAP", "SMT_MAPS_CHUNKS", "SMT_SHARED_FINISH",
       "SMT_MAPS_TAPER")
TAPERS = [(1, 2), (0, 3)]
CHUNKS = [None, "8"]                    # SMT_MAPS_CHUNKS; unset is 4
SHARED = [(6, 330, 192, None), (7, 259, 192, None), (6, 700, 192, None), (6, 390, 64, None), (5, 460, 100, None),
          (8, 700, 256, "force"), (12, 700, 192, None)]
TWO_VIEW = [(6, 330, 192), (8, 700, 256)]
_ORACLE = None


def spans(per, K, n2, n1):
    """the span rule: [(first chunk, chunks)] of the groups of a slice of `per` chunks"""
    K2 = max(1, K // 2)
    n1 = min(n1, per)
    n2 = min(n2, (per - n1) // K2)
    body = per - n1 - n2 * K2
    out = [(c, min(K, body - c)) for c in range(0, body, K)]
    out += [(body + g * K2, K2) for g in range(n2)]
    out += [(body + n2 * K2 + g, 1) for g in range(n1)]
    return out, len(range(0, body, K)), n2, n1


def tapers_at(H, W, K, nviews, n2, n1):
    """(some slice has a longer group in front of a 1-chunk tail group, ... a K-chunk group and a 1-chunk tail group)"""
    nb = ((W + 63) // 64) * H * nviews
    per = (nb + 7) >> 3
    groups, nbody, e2, e1 = spans(per, K, n2, n1)
    assert sum(n for _, n in groups) == per and all(a + n == b for (a, n), (b, _) in zip(groups, groups[1:]))
    some = strict = False
    for x in range(8):
        mine = [min(n, nb - (x * per + c)) for c, n in groups if x * per + c < nb]      # cut by the launch's end
        tail = mine[nbody + e2:]
        some |= 1 in tail and max(mine[:nbody + e2], default=0) > 1
        strict |= K in mine[:nbody] and 1 in tail
    return some, strict


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _env(mp, name, value):
    if value is None: mp.delenv(name, raising=False)
    else: mp.setenv(name, value)


def _batch(adc, Lb, Rb):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    n, H, W = Lb.shape
    dl = torch.full((n, H, W), float("nan"), device=Lb.device)
    dr = torch.full((n, H, W), float("nan"), device=Lb.device)
    adc._bind_stream()
    assert lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), n, VIEW_BOTH, _p(dl), _p(dr)) == 0
    adc.status()                        # raises if the domain flag is set
    return dl.cpu().numpy(), dr.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _handle(smt, Lb, Rb, D):
    _, H, W = Lb.shape
    return smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0, placement_search=False, store_calibration=False)


@functools.lru_cache(maxsize=None)
def _case(H, W, D):
    """images and the oracle's maps of every pair, computed once per shape"""
    O = _ORACLE
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 9300 + 17 * b + W, noise=(b % 2 == 0)) for b in range(B)])
    maps = [(O.wta(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0)), O.wta(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1)))
            for b in range(B)]
    for a, c in maps:
        a.setflags(write=False); c.setflags(write=False)
    return np.stack(Ls), np.stack(Rs), maps


@pytest.fixture(autouse=True)
def _oracle(O, monkeypatch):
    global _ORACLE
    _ORACLE = O
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _check(dl, dr, maps, what):
    for b, (ml, mr) in enumerate(maps):
        assert np.array_equal(dl[b], ml), ("left", b, np.argwhere(dl[b] != ml)[:4].tolist()) + what
        assert np.array_equal(dr[b], mr), ("right", b, np.argwhere(dr[b] != mr)[:4].tolist()) + what


def _run(smt, monkeypatch, H, W, D, nviews):
    Ls, Rs, maps = _case(H, W, D)
    Lb, Rb = _dev(Ls), _dev(Rs)
    adc = _handle(smt, Lb, Rb, D)
    for n2, n1 in TAPERS:
        for K in CHUNKS:
            some, _ = tapers_at(H, W, int(K or 4), nviews, n2, n1)
            assert some, ("the shape does not taper", n2, n1, K)
            monkeypatch.setenv("SMT_MAPS_TAPER", "%d,%d" % (n2, n1))
            _env(monkeypatch, "SMT_MAPS_CHUNKS", K)
            dl, dr = _batch(adc, Lb, Rb)
            _check(dl, dr, maps, (n2, n1, K))
    adc.close()


def test_every_taper_and_k_has_a_strict_case():
    """a K-chunk group and a 1-chunk group in one slice, for every taper and K, in the shared and the two-view family"""
    for shapes, nviews in ((SHARED, 1), (TWO_VIEW, 2)):
        for n2, n1 in TAPERS:
            for K in CHUNKS:
                assert any(tapers_at(s[0], s[1], int(K or 4), nviews, n2, n1)[1] for s in shapes), (nviews, n2, n1, K)
    # the plain rule is the parent's: group g takes [g K, g K + K)
    for per in (1, 5, 9, 22, 4050):
        for K in (1, 4, 8):
            assert spans(per, K, 0, 0)[0] == [(c, min(K, per - c)) for c in range(0, per, K)]


@pytest.mark.parametrize("H,W,D,form", SHARED)
def test_shared_form_under_forced_tapers(smt, H, W, D, form, monkeypatch):
    _env(monkeypatch, "SMT_MAPS_SHARED", form)
    _run(smt, monkeypatch, H, W, D, 1)


@pytest.mark.parametrize("H,W,D", TWO_VIEW)
def test_two_view_kernel_under_forced_tapers(smt, H, W, D, monkeypatch):
    monkeypatch.setenv("SMT_MAPS_SHARED", "0")
    _run(smt, monkeypatch, H, W, D, 2)


def test_rank_kernel_under_forced_tapers(smt, monkeypatch):
    monkeypatch.setenv("SMT_MAPS_KERNEL", "rank")
    _run(smt, monkeypatch, 6, 330, 192, 2)
