"""Sub-pixel SAD on the device (include/smt_sad_subpixel.h), bit for bit against the NumPy restatement of
tests/sad_subpixel_cases.py and form against form: smt_sad_subpixel under smt_sad_set_impl(1 / 2), smt_sad_both_subpixel
as box + keys + k_sad_refine_right, box + volume and composed, under bands of 1 and 3 rows, and the flow.  Outputs are
prefilled (tests/prefill.py) or sit between guards (tests/arena.py); one case runs behind a sleep on a side stream.  The
integer winners every float entry writes are smt_sad's maps, and smt_sad / smt_sad_both still give the oracle's.  No
tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import sad_subpixel_cases as SS  # noqa: E402
from prefill import first_diff, flows  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSED, BOX_KEYS, BOX_VOLUME = 1, 2, 3
VIEW_LEFT, VIEW_RIGHT = 1, 2


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the table's arrays are read-only


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (what, first_diff(got, ref))


@pytest.fixture
def hooks(flows):
    yield flows
    flows.sad_set_impl(2)
    flows.sad_both_set_impl(2)
    flows.sad_both_set_dispatch(0)
    flows.sad_both_set_band(0)


def both_forms(smt, tl, tr, D, ws, md, ref, what, forms=((1, 2, BOX_KEYS), (1, 1, BOX_VOLUME), (2, 2, COMPOSED), (0, 2, None))):
    """smt_sad_both_subpixel under every (dispatch, impl): maps, winners and the volume's presence"""
    rl, rr, wl, wr = ref
    for dispatch, impl, form in forms:
        smt.sad_both_set_dispatch(dispatch)
        smt.sad_both_set_impl(impl)
        dl, dr, gl, gr = smt.GetPointDepthBothSubpixel(tl, tr, D, ws, md, want_winner=True)
        if form is not None:
            assert smt.sad_both_last_form() == form, (what, dispatch, impl)       # the fallback must not carry the suite
        w = what + (dispatch, impl)
        same(dl, rl, w + ("dispL",)); same(dr, rr, w + ("dispR",)); same(gl, wl, w + ("winL",)); same(gr, wr, w + ("winR",))
        dl2, dr2 = smt.GetPointDepthBothSubpixel(tl, tr, D, ws, md)               # without the winners: NULL maps
        same(dl2, rl, w + ("dispL, no winners",)); same(dr2, rr, w + ("dispR, no winners",))
    smt.sad_both_set_dispatch(0)
    smt.sad_both_set_impl(2)


@pytest.mark.parametrize("name", SS.NAMES)
def test_every_form_equals_the_restatement(hooks, O, name):
    smt = hooks
    Lp, Rp, D, ws = SS.pair(name)
    tl, tr = T(Lp), T(Rp)
    ol, orr = O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
    for md in SS.MIN_DENS:
        ref = SS.restate(name, md)
        rl, rr, wl, wr = ref
        assert np.array_equal(wl, ol) and np.array_equal(wr, orr)
        for impl in (2, 1):                                    # k_sad2 / k_sad (k_sad8 beyond D = 256, k_sad at 3 x 3)
            smt.sad_set_impl(impl)
            for view, r, w in ((VIEW_LEFT, rl, wl), (VIEW_RIGHT, rr, wr)):
                d, g = smt.GetPointDepthSubpixel(tl, tr, D, ws, view, md, want_winner=True)
                same(d, r, (name, md, "smt_sad_set_impl", impl, view)); same(g, w, (name, md, impl, view, "winner"))
                same(smt.GetPointDepthSubpixel(tl, tr, D, ws, view, md), r, (name, md, impl, view, "no winner"))
            both_forms(smt, tl, tr, D, ws, md, ref, (name, md, "sad impl", impl), forms=((2, 2, COMPOSED),))
        smt.sad_set_impl(2)
        both_forms(smt, tl, tr, D, ws, md, ref, (name, md))
    # the integer entry points are what they were: the oracle's maps, after and between the float calls
    for impl in (2, 1):
        smt.sad_set_impl(impl)
        same(smt.GetPointDepthLeft(tl, tr, D, ws), ol, (name, "smt_sad left", impl))
        same(smt.GetPointDepthRight(tl, tr, D, ws), orr, (name, "smt_sad right", impl))
    for dispatch, impl in ((1, 2), (1, 1), (2, 2)):
        smt.sad_both_set_dispatch(dispatch); smt.sad_both_set_impl(impl)
        il, ir = smt.GetPointDepthBoth(tl, tr, D, ws)
        same(il, ol, (name, "smt_sad_both left", dispatch, impl)); same(ir, orr, (name, "smt_sad_both right", dispatch, impl))


@pytest.mark.parametrize("name", SS.BAND_CASES)
@pytest.mark.parametrize("band", [1, 3])
def test_bands_of_the_box_kernel(hooks, name, band):
    """bands of 3 rows take rows out of the running sums and cross band edges at H = 7; bands of 1 only add"""
    smt = hooks
    Lp, Rp, D, ws = SS.pair(name)
    tl, tr = T(Lp), T(Rp)
    smt.sad_both_set_band(band)
    for md in SS.MIN_DENS:
        both_forms(smt, tl, tr, D, ws, md, SS.restate(name, md), (name, band, md), forms=((1, 2, BOX_KEYS), (1, 1, BOX_VOLUME)))


def test_the_volume_comes_with_the_maps(hooks):
    smt = hooks
    for name in ("D130", "W65-H7", "win3"):
        Lp, Rp, D, ws = SS.pair(name)
        rowsL = SS.winners(name)[0]
        rl, rr, _, _ = SS.restate(name, 1.0)
        for dispatch, impl in ((1, 2), (1, 1), (2, 2)):
            smt.sad_both_set_dispatch(dispatch); smt.sad_both_set_impl(impl)
            dl, dr, cl = smt.GetPointDepthBothSubpixel(T(Lp), T(Rp), D, ws, 1.0, want_cost=True)
            same(dl, rl, (name, dispatch, impl)); same(dr, rr, (name, dispatch, impl))
            same(cl, rowsL.astype(np.float32), (name, dispatch, impl, "costL"))


ARENA = [("planted-64", "single", 2), ("D257", "single", 2), ("win0", "single", 2), ("W65-H7", "single", 1),
         ("planted-129", "both", (1, 2)), ("D512", "both", (1, 2)), ("W130-H7", "both", (1, 1)), ("win8-sat", "both", (1, 2)),
         ("W20-H2", "both", (2, 2)), ("W63-H1", "both", (1, 2))]


@pytest.mark.parametrize("name,entry,how", ARENA, ids=[f"{n}-{e}-{h}" for n, e, h in ARENA])
def test_in_the_arena(hooks, name, entry, how):
    """guards on both sides of every tensor, both prefill seeds (one all-NaN), the inputs untouched"""
    smt = hooks
    from stereo_match_traditional_amd import _lib
    lib = _lib.lib()
    Lp, Rp, D, ws = SS.pair(name)
    H, W = Lp.shape[0] - 2 * (ws + 1), Lp.shape[1] - 2 * (ws + 1)
    md = 2.0 ** -20
    rl, rr, wl, wr = SS.restate(name, md)
    p = _lib.SubpixelParams(md)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "single":
        smt.sad_set_impl(how)
        for view, r, w in ((VIEW_LEFT, rl, wl), (VIEW_RIGHT, rr, wr)):
            def make(A):
                A.inp("Lp", Lp); A.inp("Rp", Rp); A.out("disp", (H, W), np.float32); A.out("winner", (H, W), np.int32)
                return lambda A: lib.smt_sad_subpixel(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, view, C.byref(p), A.ptr("disp"),
                                                      A.ptr("winner"), st())
            out, _ = arena.run_two_seeds(make, "cuda:0", torch.cuda.synchronize)
            same(out["disp"], r, (name, view)); same(out["winner"], w, (name, view, "winner"))
    else:
        smt.sad_both_set_dispatch(how[0]); smt.sad_both_set_impl(how[1])

        def make(A):
            A.inp("Lp", Lp); A.inp("Rp", Rp)
            for n, dt in (("dispL", np.float32), ("dispR", np.float32), ("winL", np.int32), ("winR", np.int32)):
                A.out(n, (H, W), dt)
            A.out("costL", (H, W, D), np.float32)
            return lambda A: lib.smt_sad_both_subpixel(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, C.byref(p), A.ptr("dispL"), A.ptr("dispR"),
                                                       A.ptr("winL"), A.ptr("winR"), A.ptr("costL"), st())
        out, _ = arena.run_two_seeds(make, "cuda:0", torch.cuda.synchronize)
        same(out["dispL"], rl, name); same(out["dispR"], rr, name); same(out["winL"], wl, name); same(out["winR"], wr, name)
        same(out["costL"], SS.winners(name)[0].astype(np.float32), (name, "costL"))


@pytest.mark.parametrize("entry", ["single", "both", "flow"])
def test_asynchronous_on_a_busy_side_stream(hooks, entry):
    """enqueued behind a long sleep on a side stream, the call returns while the stream is still busy and reads the
    images that a copy behind the sleep put there: it is ordered on that stream"""
    smt = hooks
    name = "planted-65"
    Lp, Rp, D, ws = SS.pair(name)
    w = ws + 1
    rl, rr, wl, wr = SS.restate(name, 1.0)
    src = (Lp, Rp) if entry != "flow" else (Lp[w:-w, w:-w], Rp[w:-w, w:-w])
    s = torch.cuda.Stream(DEV)
    f = smt.SADFlow(rl.shape[0], rl.shape[1], D, winsize=ws) if entry == "flow" else None
    with torch.cuda.stream(s):
        a, b = T(src[0]), T(src[1])
        tl, tr = torch.zeros_like(a), torch.zeros_like(b)
        if f is not None:
            f.run_subpixel(tl, tr)                             # the handle's float maps exist: a warm call
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        tl.copy_(a, non_blocking=True); tr.copy_(b, non_blocking=True)
        if entry == "single":
            out = smt.GetPointDepthSubpixel(tl, tr, D, ws, VIEW_LEFT, 1.0, want_winner=True) + \
                smt.GetPointDepthSubpixel(tl, tr, D, ws, VIEW_RIGHT, 1.0, want_winner=True)
            out = (out[0], out[2], out[1], out[3])
        elif entry == "both":
            out = smt.GetPointDepthBothSubpixel(tl, tr, D, ws, 1.0, want_winner=True)
            assert smt.sad_both_last_form() == BOX_KEYS
        else:
            dl, dr, last, cls = f.run_subpixel(tl, tr)
            out = (dl[0], dr[0])
        pending = not s.query()
    s.synchronize()
    assert pending, f"{entry} waited for the stream"
    same(out[0], rl, (entry, "dispL")); same(out[1], rr, (entry, "dispR"))
    if entry != "flow":
        same(out[2], wl, (entry, "winL")); same(out[3], wr, (entry, "winR"))
    else:
        elast, ecls = SS.crosscheck(wl, wr, rl)
        same(last[0], elast, "lastdisp"); same(cls[0], ecls, "cls")
        f.close()


def test_flow_batch(hooks, O):
    """the nine planted pairs in one batch: maps against the restatement, the cross-check decided on the integer winners
    (cls is the integer flow's and the oracle's), lastdisp dispL or +inf; NULL outputs in every combination; a warm call
    allocates nothing; pairs == 0; the sharding unit"""
    smt = hooks
    from stereo_match_traditional_amd import _lib, shard
    lib = _lib.lib()
    names = [n for n in SS.NAMES if n.startswith("planted-")]
    Lp0, _, D, ws = SS.pair(names[0])
    w = ws + 1
    L = T(np.stack([SS.pair(n)[0][w:-w, w:-w] for n in names]))
    R = T(np.stack([SS.pair(n)[1][w:-w, w:-w] for n in names]))
    P, H, W = L.shape
    f = smt.SADFlow(H, W, D, winsize=ws)
    il, ir, ilast, icls = f.run(L, R)
    for md in SS.MIN_DENS:
        dl, dr, last, cls = f.run_subpixel(L, R, md)
        assert smt.sad_both_last_form() == BOX_KEYS
        for b, n in enumerate(names):
            rl, rr, wl, wr = SS.restate(n, md)
            elast, ecls = SS.crosscheck(wl, wr, rl)
            assert np.array_equal(ecls, O.sad_crosscheck(wl, wr)[1]), n
            same(dl[b], rl, (n, md, "dispL")); same(dr[b], rr, (n, md, "dispR"))
            same(last[b], elast, (n, md, "lastdisp")); same(cls[b], ecls, (n, md, "cls"))
            same(il[b], wl, (n, "integer flow")); same(ir[b], wr, (n, "integer flow"))
        same(cls, icls, (md, "cls is the integer flow's"))
        lastn = last.cpu().numpy()
        assert np.isinf(lastn).sum() == int((icls != 0).sum()) > 0 and (lastn != np.floor(lastn))[np.isfinite(lastn)].any()
    full = f.run_subpixel(L, R, 1.0)
    # a second and a third run: the same bytes, and no growth of the scratch arena
    out2 = f.run_subpixel(L, R, 1.0)
    torch.cuda.synchronize()
    r2 = smt.scratch_info()
    out3 = f.run_subpixel(L, R, 1.0)
    torch.cuda.synchronize()
    r3 = smt.scratch_info()
    for a, b, c in zip(full, out2, out3):
        same(a, b, "second run"); same(a, c, "third run")
    assert r3[0] == r2[0], (r2, r3)
    # NULL outputs in every combination; what is written equals the full run, what is not stays untouched
    p = lambda t: C.c_void_p(t.data_ptr())
    prm = C.byref(_lib.SubpixelParams(1.0))
    for mask in range(16):
        bufs = [torch.full_like(t, 77) for t in full]
        args = [p(bufs[k]) if mask >> k & 1 else None for k in range(4)]
        assert lib.smt_sad_flow_run_batch_subpixel(f._h, p(L), p(R), P, prm, *args) == 0, mask
        torch.cuda.synchronize()
        for k in range(4):
            same(bufs[k], full[k] if mask >> k & 1 else torch.full_like(full[k], 77), (mask, k))
    keep = [t.clone() for t in full]
    assert lib.smt_sad_flow_run_batch_subpixel(f._h, p(L), p(R), 0, prm, *[p(t) for t in full]) == 0
    assert lib.smt_sad_flow_run_batch_subpixel(f._h, None, None, 0, None, None, None, None, None) == 0
    assert lib.smt_sad_flow_run_batch_subpixel(f._h, p(L), p(R), -1, prm, *[p(t) for t in full]) == -1
    assert lib.smt_sad_flow_run_batch_subpixel(f._h, None, p(R), 1, prm, *[p(t) for t in full]) == -1
    assert lib.smt_sad_flow_run_batch_subpixel(f._h, p(L), p(R), 1, C.byref(_lib.SubpixelParams(0.0)), *[p(t) for t in full]) == -1
    torch.cuda.synchronize()
    for a, b in zip(keep, full):
        same(a, b, "rejected calls write nothing")
    # the integer flow on the same handle afterwards: unchanged
    for a, b in zip(f.run(L, R), (il, ir, ilast, icls)):
        same(a, b, "integer flow after the float flow")
    f.close()
    gl, gr = shard.run_sharded(L, R, D, lambda a, b, d: shard.sad_subpixel_batch(a, b, d, min_den=64.0, winsize=ws))
    for b, n in enumerate(names):
        rl, rr, _, _ = SS.restate(n, 64.0)
        same(gl[b], rl, (n, "shard")); same(gr[b], rr, (n, "shard"))
    el, er = shard.sad_subpixel_batch(L[:0], R[:0], D, winsize=ws)
    assert el.shape == (0, H, W) and er.dtype == torch.float32


def test_sad_main_subpixel_flag(smt, O):
    """host/sad_main.cpp --subpixel [min_den] through the C++ mirror smt_sad_subpixel.hpp: the float maps are the host
    twin's, the class map is the oracle's cross-check of the integer maps; without the flag the output is the integer
    flow's"""
    from stereo_match_traditional_amd import _lib
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "sad_main")
    assert os.path.exists(exe)
    H, W, D, seed, ws = 40, 150, 60, 6, 3
    L, R = O.synth_pair(H, W, D, seed)
    Lp, Rp = O.pad_replicate(L, ws + 1), O.pad_replicate(R, ws + 1)
    ol, orr = O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
    olast, ocls = O.sad_crosscheck(ol, orr)

    def run(*extra):
        r = subprocess.run([exe, str(H), str(W), str(D), str(seed), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return dict(line.split() for line in r.stdout.strip().splitlines())

    got = run()
    assert set(got) == {"depthleft", "depthright", "lastdisp"}
    for k, v in {"depthleft": ol, "depthright": orr, "lastdisp": olast}.items():
        assert got[k] == f"{O.fnv1a(v):016x}", k
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for extra, md in ((("--subpixel",), 1.0), (("--subpixel", "0.25"), 0.25)):
        got = run(*extra)
        dl, dr = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
        wl, wr = np.empty((H, W), np.int32), np.empty((H, W), np.int32)
        assert _lib.lib().smt_sad_subpixel_host(vp(Lp), vp(Rp), H, W, D, ws, C.byref(_lib.SubpixelParams(md)), vp(dl), vp(dr), vp(wl),
                                                vp(wr)) == 0
        assert np.array_equal(wl, ol) and np.array_equal(wr, orr)
        last, cls = SS.crosscheck(wl, wr, dl)
        assert np.array_equal(cls, ocls)
        for k, v in {"depthleft": dl, "depthright": dr, "lastdisp": last, "cls": cls}.items():
            assert got[k] == f"{O.fnv1a(v):016x}", (k, md)
        assert (dl != np.floor(dl)).sum() > H * W // 4
