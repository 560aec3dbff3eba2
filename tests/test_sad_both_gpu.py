"""smt_sad_both (both SAD maps from one box-summed evaluation of the hypotheses) and smt_sad_flow_* (SADmain.cpp:47-48,
:66-68 for batches).  The feature carries no tolerance: both maps are smt_sad's and the oracle's, and costL is the integer
box-sum volume, exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from test_sad_both_cpu import SATURATED, SHAPES, left_costs, make_pair

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMT_ERR_ARG = -1
COMPOSED, BOX_KEYS, BOX_VOLUME = 1, 2, 3

# (H, W, D, winsize, seed): O.synth_pair shapes over D of 1, 64, 200, 320, 512 and winsize of 0, 1, 3, 10, 21, 30
SYNTH = [(6, 80, 1, 3, 1), (8, 100, 64, 0, 2), (6, 260, 200, 1, 3), (5, 340, 320, 10, 4), (4, 530, 512, 3, 5),
         (6, 70, 64, 21, 6), (5, 90, 200, 30, 7), (3, 200, 512, 30, 8), (33, 130, 64, 3, 9), (70, 67, 130, 1, 10), (40, 70, 64, 21, 11),
         (70, 40, 130, 30, 12), (24, 150, 320, 21, 13)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def hooks(smt):
    yield smt
    smt.sad_set_impl(2)
    smt.sad_both_set_impl(2)
    smt.sad_both_set_dispatch(0)
    smt.sad_both_set_band(0)


def check_shape(smt, O, L, R, D, ws):
    """Every combination of the hooks with the box form forced, and the default dispatch: maps against smt_sad and the
    oracle, costL against the numpy box sums.  Returns the oracle's left map."""
    Lp, Rp = O.pad_replicate(L, ws + 1), O.pad_replicate(R, ws + 1)
    tl, tr = T(Lp), T(Rp)
    want_l, want_r = T(O.sad(Lp, Rp, D, ws, 0)), T(O.sad(Lp, Rp, D, ws, 1))
    vol = left_costs(Lp, Rp, D, ws)
    for sad_impl in (2, 1):
        smt.sad_set_impl(sad_impl)
        assert torch.equal(smt.GetPointDepthLeft(tl, tr, D, ws), want_l), sad_impl
        assert torch.equal(smt.GetPointDepthRight(tl, tr, D, ws), want_r), sad_impl
        for dispatch in (1, 0):
            smt.sad_both_set_dispatch(dispatch)
            for both, form in ((2, BOX_KEYS), (1, BOX_VOLUME)):
                smt.sad_both_set_impl(both)
                dl, dr = smt.GetPointDepthBoth(tl, tr, D, ws)
                ran = smt.sad_both_last_form()
                if dispatch == 1:
                    assert ran == form, (sad_impl, both, ran)            # the fallback must not carry the suite
                assert torch.equal(dl, want_l) and torch.equal(dr, want_r), (sad_impl, dispatch, both)
                dl, dr, cl = smt.GetPointDepthBoth(tl, tr, D, ws, want_cost=True)
                assert torch.equal(dl, want_l) and torch.equal(dr, want_r), (sad_impl, dispatch, both, "cost")
                got = cl.cpu().numpy()
                assert np.array_equal(got.astype(np.int64), vol) and np.array_equal(got, got.astype(np.int64)), (dispatch, both)
    # Small images get bands of one row, which only ever add rows.  Bands of 2, 3, 7 rows and of the whole image make the
    # same shapes take rows out of the running sums, reuse both halves of the row and key buffers and cross band edges.
    smt.sad_set_impl(2)
    smt.sad_both_set_dispatch(1)
    for band in (2, 3, 7, L.shape[0]):
        smt.sad_both_set_band(band)
        for both, form in ((2, BOX_KEYS), (1, BOX_VOLUME)):
            smt.sad_both_set_impl(both)
            dl, dr, cl = smt.GetPointDepthBoth(tl, tr, D, ws, want_cost=True)
            assert smt.sad_both_last_form() == form
            assert torch.equal(dl, want_l) and torch.equal(dr, want_r), (band, both)
            assert np.array_equal(cl.cpu().numpy().astype(np.int64), vol), (band, both)
            dl, dr = smt.GetPointDepthBoth(tl, tr, D, ws)
            assert torch.equal(dl, want_l) and torch.equal(dr, want_r), (band, both, "maps only")
    smt.sad_both_set_band(0)
    return want_l


@pytest.mark.parametrize("H,W,D,winsize,kind", SHAPES)
def test_both_maps_and_costs_on_the_pinned_shapes(hooks, O, H, W, D, winsize, kind):
    L, R = make_pair(kind, H, W, H + W)
    want_l = check_shape(hooks, O, L, R, D, winsize)
    if kind in SATURATED:
        assert int((want_l == 65535).sum()) > 0


@pytest.mark.parametrize("H,W,D,winsize,seed", SYNTH)
def test_both_maps_and_costs_on_synthetic_pairs(hooks, O, H, W, D, winsize, seed):
    L, R = O.synth_pair(H, W, min(D, 64), seed, seed % 2 == 0)
    check_shape(hooks, O, L, R, D, winsize)


@pytest.mark.parametrize("winsize,form", [(40, BOX_KEYS), (89, BOX_KEYS), (90, COMPOSED), (95, COMPOSED)])
def test_large_windows_and_the_forced_fallback(hooks, O, winsize, form):
    """The box form covers windows up to 181 x 181 (winsize 89: the 32-bit key bound); beyond it the call composes smt_sad."""
    smt = hooks
    H, W, D = 5, 21, 12
    L, R = make_pair("noise", H, W, winsize)
    Lp, Rp = O.pad_replicate(L, winsize + 1), O.pad_replicate(R, winsize + 1)
    tl, tr = T(Lp), T(Rp)
    for both in (2, 1):
        smt.sad_both_set_impl(both)
        dl, dr, cl = smt.GetPointDepthBoth(tl, tr, D, winsize, want_cost=True)
        ran = smt.sad_both_last_form()
        assert ran == (form if form == COMPOSED or both == 2 else BOX_VOLUME)
        assert torch.equal(dl, smt.GetPointDepthLeft(tl, tr, D, winsize))
        assert torch.equal(dr, smt.GetPointDepthRight(tl, tr, D, winsize))
        assert np.array_equal(dl.cpu().numpy(), O.sad(Lp, Rp, D, winsize, 0))
        assert np.array_equal(dr.cpu().numpy(), O.sad(Lp, Rp, D, winsize, 1))
        assert np.array_equal(cl.cpu().numpy().astype(np.int64), left_costs(Lp, Rp, D, winsize))
    smt.sad_both_set_dispatch(2)                                           # composed on request at any size
    dl, dr = smt.GetPointDepthBoth(tl, tr, D, winsize)
    assert smt.sad_both_last_form() == COMPOSED
    assert torch.equal(dl, smt.GetPointDepthLeft(tl, tr, D, winsize)) and torch.equal(dr, smt.GetPointDepthRight(tl, tr, D, winsize))


def test_flow_batch(hooks, O):
    """Three different pairs of (24, 96), D = 48, winsize 2 in one run_batch against three composed single-pair sequences
    and the oracle; NULL outputs in every combination; pairs == 0; a warm call; a non-default stream; the sharding unit."""
    smt = hooks
    from stereo_match_traditional_amd._lib import lib
    H, W, D, ws = 24, 96, 48, 2
    pairs = [O.synth_pair(H, W, 32, 11, True), O.synth_pair(H, W, 32, 12, False), make_pair("shift", H, W, 3)]
    L = T(np.stack([p[0] for p in pairs]))
    R = T(np.stack([p[1] for p in pairs]))
    f = smt.SADFlow(H, W, D, winsize=ws)
    dl, dr, last, cls = f.run(L, R)
    assert smt.sad_both_last_form() in (BOX_KEYS, COMPOSED)
    for b, (l, r) in enumerate(pairs):
        tl, tr = smt.copyMakeBorder_replicate(T(l), ws + 1), smt.copyMakeBorder_replicate(T(r), ws + 1)
        bl, br = smt.GetPointDepthLeft(tl, tr, D, ws), smt.GetPointDepthRight(tl, tr, D, ws)
        blast, bcls = smt.sad_CrossCheckDiaparity(bl, br)
        assert torch.equal(dl[b], bl) and torch.equal(dr[b], br), b
        assert torch.equal(last[b], blast) and torch.equal(cls[b], bcls), b
        Lp, Rp = O.pad_replicate(l, ws + 1), O.pad_replicate(r, ws + 1)
        ol, orr = O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
        olast, ocls = O.sad_crosscheck(ol, orr)
        assert np.array_equal(dl[b].cpu().numpy(), ol) and np.array_equal(dr[b].cpu().numpy(), orr), b
        assert np.array_equal(last[b].cpu().numpy(), olast) and np.array_equal(cls[b].cpu().numpy(), ocls), b
    assert not torch.equal(dl[0], dl[1]) and not torch.equal(dl[1], dl[2])
    # a second and a third run on the same handle: the same bytes, and no growth of the scratch arena
    out2 = f.run(L, R)
    torch.cuda.synchronize()
    r2 = smt.scratch_info()
    out3 = f.run(L, R)
    torch.cuda.synchronize()
    r3 = smt.scratch_info()
    for a, b, c in zip((dl, dr, last, cls), out2, out3):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert r3[0] == r2[0], (r2, r3)
    # NULL outputs in every combination; what is written equals the full run, what is not stays untouched
    p = lambda t: C.c_void_p(t.data_ptr())
    full = (dl, dr, last, cls)
    for mask in range(16):
        bufs = [torch.full_like(t, 77) for t in full]
        args = [p(bufs[k]) if mask >> k & 1 else None for k in range(4)]
        assert lib().smt_sad_flow_run_batch(f._h, p(L), p(R), 3, *args) == 0, mask
        torch.cuda.synchronize()
        for k in range(4):
            assert torch.equal(bufs[k], full[k] if mask >> k & 1 else torch.full_like(full[k], 77)), (mask, k)
    # pairs == 0 leaves the outputs untouched
    keep = [t.clone() for t in full]
    assert lib().smt_sad_flow_run_batch(f._h, p(L), p(R), 0, p(dl), p(dr), p(last), p(cls)) == 0
    assert lib().smt_sad_flow_run_batch(f._h, None, None, 0, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, full))
    assert lib().smt_sad_flow_run_batch(f._h, p(L), p(R), -1, p(dl), p(dr), p(last), p(cls)) == SMT_ERR_ARG
    assert lib().smt_sad_flow_run_batch(f._h, None, p(R), 1, p(dl), p(dr), p(last), p(cls)) == SMT_ERR_ARG
    assert lib().smt_sad_flow_run_batch(f._h, p(L), None, 1, p(dl), p(dr), p(last), p(cls)) == SMT_ERR_ARG
    assert lib().smt_sad_flow_run_batch(None, p(L), p(R), 1, p(dl), p(dr), p(last), p(cls)) == SMT_ERR_ARG
    # a non-default stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = f.run(L, R)
        tl, tr = smt.copyMakeBorder_replicate(L[1], ws + 1), smt.copyMakeBorder_replicate(R[1], ws + 1)
        sl, sr = smt.GetPointDepthBoth(tl, tr, D, ws)
    s.synchronize()
    for a, b in zip(full, outs):
        assert torch.equal(a, b)
    assert torch.equal(sl, dl[1]) and torch.equal(sr, dr[1])
    f.close()
    # the sharding unit
    from stereo_match_traditional_amd import shard
    gl, gr = shard.run_sharded(L, R, D, lambda a, b, d: shard.sad_batch(a, b, d, winsize=ws))
    assert torch.equal(gl, dl) and torch.equal(gr, dr)
    el, er = shard.sad_batch(L[:0], R[:0], D, winsize=ws)
    assert el.shape == (0, H, W) and er.dtype == torch.int32


def test_bad_arguments_get_smt_sads_answer(smt):
    from stereo_match_traditional_amd import _lib as Lb
    lib = Lb.lib()
    H, W, D, ws = 8, 16, 4, 2
    Lp = torch.full((H + 2 * ws + 2, W + 2 * ws + 2), 7, dtype=torch.uint8, device=DEV)
    dl = torch.full((H, W), -5, dtype=torch.int32, device=DEV)
    dr = torch.full((H, W), -5, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = smt.current_stream_ptr()
    cases = [(H, W, 0, ws), (H, W, -1, ws), (H, W, 513, ws), (H, W, D, -1), (0, W, D, ws), (H, 0, D, ws), (-3, W, D, ws),
             (H, -3, D, ws)]
    for hh, ww, dd, w_ in cases:
        for view in (Lb.VIEW_LEFT, Lb.VIEW_RIGHT):
            assert lib.smt_sad(p(Lp), p(Lp), hh, ww, dd, w_, view, p(dl), st) == SMT_ERR_ARG, (hh, ww, dd, w_)
        assert lib.smt_sad_both(p(Lp), p(Lp), hh, ww, dd, w_, p(dl), p(dr), None, st) == SMT_ERR_ARG, (hh, ww, dd, w_)
        h = C.c_void_p()
        prm = Lb.SADParams()
        prm.winsize = w_
        assert lib.smt_sad_flow_create_on(0, hh, ww, dd, C.byref(prm), C.byref(h)) == SMT_ERR_ARG, (hh, ww, dd, w_)
    assert lib.smt_sad_both(None, p(Lp), H, W, D, ws, p(dl), p(dr), None, st) == SMT_ERR_ARG
    assert lib.smt_sad_both(p(Lp), None, H, W, D, ws, p(dl), p(dr), None, st) == SMT_ERR_ARG
    assert lib.smt_sad_both(p(Lp), p(Lp), H, W, D, ws, None, p(dr), None, st) == SMT_ERR_ARG
    assert lib.smt_sad_both(p(Lp), p(Lp), H, W, D, ws, p(dl), None, None, st) == SMT_ERR_ARG
    torch.cuda.synchronize()
    assert bool((dl == -5).all()) and bool((dr == -5).all())                      # nothing was launched
    h = C.c_void_p()
    assert lib.smt_sad_flow_create_on(0, H, W, D, None, None) == SMT_ERR_ARG
    assert lib.smt_sad_flow_create_on(-1, H, W, D, None, C.byref(h)) == SMT_ERR_ARG
    assert lib.smt_sad_flow_create_on(0, H, W, D, None, C.byref(h)) == 0          # NULL params: the defaults
    assert lib.smt_sad_flow_set_stream(None, None) == SMT_ERR_ARG
    assert lib.smt_sad_flow_destroy(None) == SMT_ERR_ARG
    assert lib.smt_sad_flow_destroy(h) == 0
    # what smt_sad accepts is accepted: one-pixel images, W < D, winsize 0
    one = torch.full((3, 3), 9, dtype=torch.uint8, device=DEV)
    a, b = smt.GetPointDepthBoth(one, one, 512, 0)
    assert a.shape == (1, 1) and int(a[0, 0]) == int(smt.GetPointDepthLeft(one, one, 512, 0)[0, 0]) and int(b[0, 0]) == 0


def test_sad_main_counterpart(smt, O):
    """host/sad_main.cpp = SADmain.cpp with :67-68 enabled through the C++ mirror, at SADmain.cpp's own size (450 x 375,
    MaxDisparity 60, winsize 3): the three maps' hashes against the oracle."""
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "sad_main")
    assert os.path.exists(exe)
    H, W, D, seed, ws = 375, 450, 60, 6, 3
    r = subprocess.run([exe, str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    L, R = O.synth_pair(H, W, D, seed)
    Lp, Rp = O.pad_replicate(L, ws + 1), O.pad_replicate(R, ws + 1)
    ol, orr = O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
    olast, _ = O.sad_crosscheck(ol, orr)
    for k, v in {"depthleft": ol, "depthright": orr, "lastdisp": olast}.items():
        assert got[k] == f"{O.fnv1a(v):016x}", k


@pytest.mark.parametrize("H,W,D,winsize,oracle", [(375, 450, 60, 3, True), (375, 450, 64, 1, True), (1080, 1920, 128, 3, False)])
def test_full_size(hooks, O, H, W, D, winsize, oracle):
    """SADmain's own size, config 1 and 1080p: the maps of both forms equal smt_sad's (and the oracle's at the two small
    sizes; it is too slow at 1080p)."""
    smt = hooks
    from stereo_match_traditional_amd import synth
    L, R = synth.synth_pair(H, W, D, 4)
    tl, tr = smt.copyMakeBorder_replicate(T(L), winsize + 1), smt.copyMakeBorder_replicate(T(R), winsize + 1)
    want_l, want_r = smt.GetPointDepthLeft(tl, tr, D, winsize), smt.GetPointDepthRight(tl, tr, D, winsize)
    assert int((want_l != 0).sum()) > H * W // 4                                  # a real map, not a field of zeros
    for dispatch in (1, 0):
        smt.sad_both_set_dispatch(dispatch)
        for both in (2, 1):
            smt.sad_both_set_impl(both)
            dl, dr = smt.GetPointDepthBoth(tl, tr, D, winsize)
            if dispatch == 1:
                assert smt.sad_both_last_form() == (BOX_KEYS if both == 2 else BOX_VOLUME)
            assert torch.equal(dl, want_l) and torch.equal(dr, want_r), (dispatch, both)
    if oracle:
        Lp, Rp = tl.cpu().numpy(), tr.cpu().numpy()
        assert np.array_equal(want_l.cpu().numpy(), O.sad(Lp, Rp, D, winsize, 0))
        assert np.array_equal(want_r.cpu().numpy(), O.sad(Lp, Rp, D, winsize, 1))
