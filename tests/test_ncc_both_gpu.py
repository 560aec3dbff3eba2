"""smt_lrncc and smt_lrncc_flow_run_batch on the device.  The feature carries no tolerance of its own.  Everything is bit
for bit: dispL and costL against smt_ncc under the same impl; dispR and costR under KEYS against the mirrored
NCC_algorithem call (torch.flip done here) and against COMPOSED; lastdisp and cls against smt_sad_crosscheck on the flow's
own maps.  The only bound is exact_matchers.check_ncc's, for costR against the exact rational function of the mirrored
pair, and dispR is WinTakeAll of the call's own costR exactly."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402
import exact_matchers as X  # noqa: E402
import ncc_both_cases as LC  # noqa: E402
from test_ncc_box_cpu import top_images  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMT_ERR_ARG = -1
LOOP, DOT4, BOX = 1, 2, 3
COMPOSED, KEYS = 1, 2


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def images(O, H, W, kind, seed):
    return top_images(H, W, seed) if kind == "top" else X.ncc_images(O, H, W, kind, seed)


@pytest.fixture
def hooks(smt):
    yield smt
    smt.ncc_set_impl(2)
    smt.ncc_box_set_band(0)
    smt.lrncc_set_impl(0)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def both(smt, L, R, D, win, impl, lr, want_cost=True):
    """-> (dispL, dispR, costL, costR, form) as numpy"""
    smt.ncc_set_impl(impl)
    smt.lrncc_set_impl(lr)
    out = smt.NCC_both(T(L), T(R), win, D, want_cost=want_cost)
    form = smt.lrncc_last_form()
    out = [o.cpu().numpy() for o in out] + ([] if want_cost else [None, None])
    return (*out, form)


def single(smt, L, R, D, win, impl):
    smt.ncc_set_impl(impl)
    d, c = smt.NCC_algorithem(T(L), T(R), win, D, want_cost=True)
    return d.cpu().numpy(), c.cpu().numpy()


def mirrored(smt, L, R, D, win, impl):
    """the right view by its definition, on the device: fliplr(NCC_algorithem(fliplr(R), fliplr(L))), costs likewise"""
    smt.ncc_set_impl(impl)
    fl, fr = torch.flip(T(R), [1]).contiguous(), torch.flip(T(L), [1]).contiguous()
    d, c = smt.NCC_algorithem(fl, fr, win, D, want_cost=True)
    return torch.flip(d, [1]).cpu().numpy(), torch.flip(c, [1]).cpu().numpy()


def hold(smt, L, R, D, win, impl, want_form=KEYS):
    """one pair under KEYS (or what the hooks must fall to): both views against the single-view calls, the maps-only call,
    and COMPOSED.  -> (dispL, dispR, costL, costR)"""
    dl, dr, cl, cr, form = both(smt, L, R, D, win, impl, KEYS)
    assert form == want_form
    d1, c1 = single(smt, L, R, D, win, impl)
    assert same_bits(cl, c1) and np.array_equal(dl, d1), "left view != smt_ncc"
    dm, cm = mirrored(smt, L, R, D, win, impl)
    assert same_bits(cr, cm), "costR != the mirrored call"
    assert np.array_equal(dr, dm), "dispR != the mirrored call"
    ml, mr, _, _, f = both(smt, L, R, D, win, impl, KEYS, want_cost=False)
    assert f == want_form and np.array_equal(ml, dl) and np.array_equal(mr, dr), "maps-only call"
    kl, kr, kcl, kcr, f = both(smt, L, R, D, win, impl, COMPOSED)
    assert f == COMPOSED
    assert np.array_equal(kl, dl) and np.array_equal(kr, dr) and same_bits(kcl, cl) and same_bits(kcr, cr), "COMPOSED != KEYS"
    return dl, dr, cl, cr


# ------------------------------------------------------------------------------------------ 1. every instantiation
# W > D: hypotheses of every slot have real costs; D = 130 is three dot4 slots and the four-slot box kernel
@pytest.mark.parametrize("impl", [2, 3])
@pytest.mark.parametrize("D", [1, 64, 65, 130, 200, 256, 300, 512])
def test_keys_equal_the_mirror_at_every_slot_count(hooks, O, impl, D):
    H, W, win = 4, D + 37, 1
    L, R = X.ncc_images(O, H, W, "noise", 300 + D)
    dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
    real = (cr != 255.0) & ~np.isnan(cr)
    assert real[..., D - 1].sum() > 0 and real[..., 64 * ((D - 1) // 64)].sum() > 0   # real costs in the last slot
    exact, flat, sentinel = LC.mirror_exact(L, R, D, win)
    X.check_ncc(cr, exact, flat, sentinel, win, "int")
    assert np.array_equal(dr, X.ncc_wta(cr, win))


@pytest.mark.parametrize("impl", [2, 3])
@pytest.mark.parametrize("H,W,D,win", [(5, 40, 100, 1), (6, 30, 300, 2)])
def test_keys_with_fewer_columns_than_hypotheses(hooks, O, impl, H, W, D, win):
    L, R = X.ncc_images(O, H, W, "noise", 17)
    dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
    assert np.array_equal(dr, X.ncc_wta(cr, win))


# ------------------------------------------------------------------------------------------ 2. strips, groups, bands
@pytest.mark.parametrize("Wi", [1, 15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("Hi", [1, 2])
def test_strip_and_group_edges(hooks, O, Hi, Wi):
    win, D = 2, 20
    H, W = Hi + 2 * win, Wi + 2 * win
    L, R = X.ncc_images(O, H, W, "noise", 100 + Wi)
    for impl in (2, 3):
        hold(hooks, L, R, D, win, impl)


@pytest.mark.parametrize("H,W,D,win,kind", [(25, 41, 12, 10, "synth"), (9, 150, 70, 1, "noise")])
def test_bands_give_identical_bits(hooks, O, H, W, D, win, kind):
    L, R = X.ncc_images(O, H, W, kind, 9)
    outs = []
    for band in (1, 3, 0):
        hooks.ncc_box_set_band(band)
        outs.append(hold(hooks, L, R, D, win, 3))
    for o in outs[1:]:
        assert np.array_equal(o[1], outs[0][1]) and same_bits(o[3], outs[0][3])


def test_a_right_pixel_fed_from_two_strips(hooks, O):
    """6 x 150, D = 70, win 1: interior width 148 = three box strips; right pixel x' takes offers from columns x' .. x' + 69"""
    H, W, D, win = 6, 150, 70, 1
    L, R = X.ncc_images(O, H, W, "noise", 23)
    for impl in (2, 3):
        dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
    wi = np.arange(W - 2 * win)
    fed = (wi[:, None] + np.arange(D)[None, :]) // 64                      # strip of the left column behind each offer
    assert ((fed.max(1) > fed.min(1)) & (wi + D <= W - 2 * win)).any()


# ------------------------------------------------------------------------------------------ 3. window sides
def test_side_1_is_all_nan_and_zero(hooks, O):
    H, W, D, win = 9, 30, 33, 0
    L, R = X.ncc_images(O, H, W, "synth", 45)
    for impl in (2, 3):
        dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
        assert np.isnan(cr[cr != 255.0]).all() and (dr == 0).all()


@pytest.mark.parametrize("H,W,D,win,kind", [(8, 50, 30, 1, "synth_flat"), (12, 60, 40, 2, "synth_flat"), (12, 40, 20, 2, "nearly_flat")])
def test_sides_3_and_5_with_flat_windows(hooks, O, H, W, D, win, kind):
    L, R = X.ncc_images(O, H, W, kind, 40)
    for impl in (2, 3):
        dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
        exact, flat, sentinel = LC.mirror_exact(L, R, D, win)
        X.check_ncc(cr, exact, flat, sentinel, win, "int")
        assert np.array_equal(dr, X.ncc_wta(cr, win))
        if kind == "synth_flat":
            assert flat.any() and (dr[np.isnan(cr[..., 0])] == 0).all()    # a NaN at d = 0 gives 0


def test_side_33_box_only(hooks, O):
    H, W, D, win = 36, 60, 12, 16
    L, R = X.ncc_images(O, H, W, "synth", 41)
    dl, dr, cl, cr = hold(hooks, L, R, D, win, 3)
    exact, flat, sentinel = LC.mirror_exact(L, R, D, win)
    X.check_ncc(cr, exact, flat, sentinel, win, "int")
    # impl 2 has no integer form at this side: the loop nest, and with it COMPOSED
    dl2, dr2, cl2, cr2, form = both(hooks, L, R, D, win, 2, KEYS)
    assert form == COMPOSED
    dm, cm = mirrored(hooks, L, R, D, win, 2)
    assert np.array_equal(dr2, dm) and same_bits(cr2, cm)


def test_past_181_is_composed_on_the_loop_nest(hooks, O):
    H, W, D, win = 185, 190, 3, 91
    L, R = X.ncc_images(O, H, W, "bright", 5)
    for lr in (0, KEYS):
        dl, dr, cl, cr, form = both(hooks, L, R, D, win, 3, lr)
        assert form == COMPOSED and hooks.ncc_last_form() == LOOP
        d1, c1 = single(hooks, L, R, D, win, 3)
        dm, cm = mirrored(hooks, L, R, D, win, 3)
        assert np.array_equal(dl, d1) and same_bits(cl, c1) and np.array_equal(dr, dm) and same_bits(cr, cm)
        assert np.array_equal(dr, X.ncc_wta(cr, win))


# ------------------------------------------------------------------------------------------ 4. sentinels, NaNs, ties
def test_sentinel_columns_take_the_first_sentinel(hooks, O):
    H, W, D, win = 8, 60, 40, 1
    L, R = X.ncc_images(O, H, W, "noise", 21)
    for impl in (2, 3):
        dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
        x = np.arange(W)
        cols = (x >= win) & (x < W - win) & (W - win - x < D)
        assert cols.sum() == D - 1
        want = np.broadcast_to(W - win - x, (H, W))
        rows = slice(win, H - win)
        assert not np.isnan(cr[rows][:, cols][..., 0]).any()
        assert np.array_equal(dr[rows][:, cols], want[rows][:, cols])
        sent = np.zeros((H, W, D), bool)
        sent[rows] = ((x[:, None] + win + np.arange(D)[None, :] > W - 1) & ((x >= win) & (x < W - win))[:, None])[None]
        assert np.array_equal(cr == 255.0, sent)


@pytest.mark.parametrize("kind,H,W,D,win", [("bright", 10, 90, 70, 4), ("top", 12, 80, 40, 3), ("top", 8, 200, 130, 1),
                                            ("bright", 6, 330, 300, 1)])
def test_bright_and_top_images(hooks, O, kind, H, W, D, win):
    """NaNs (flat windows of 255) and costs that narrow to one float: the rank key against the sequential rule"""
    L, R = images(O, H, W, kind, 60 + D)
    for impl in (2, 3):
        dl, dr, cl, cr = hold(hooks, L, R, D, win, impl)
        assert np.array_equal(dr, X.ncc_wta(cr, win))
        if kind == "top":
            f = cr.astype(np.float32)
            inner = cr[win:H - win, win:W - win]
            fi = f[win:H - win, win:W - win]
            with np.errstate(invalid="ignore"):
                top2 = np.sort(np.where(np.isnan(fi) | (inner == 255.0), -np.inf, fi), -1)[..., -2:]
                tied = np.ptp(top2, -1) == 0
            assert tied.any(), "the image must produce ties of narrowed costs"


# ------------------------------------------------------------------------------------------ 5. flow
def _pairs(O, H, W, P=3, seed=30):
    kinds = ("synth", "bright", "noise")
    imgs = [X.ncc_images(O, H, W, kinds[b % 3], seed + b) for b in range(P)]
    return np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])


def _crosscheck(smt, dl, dr):
    outs = [smt.sad_CrossCheckDiaparity(dl[b], dr[b]) for b in range(dl.shape[0])]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


@pytest.mark.parametrize("H,W,D,win", [(12, 90, 70, 2), (36, 38, 5, 16)])
def test_flow_equals_single_calls_and_keeps_to_its_buffers(hooks, O, H, W, D, win):
    smt = hooks
    from stereo_match_traditional_amd._lib import lib
    Ls, Rs = _pairs(O, H, W)
    P = Ls.shape[0]
    flow = smt.NCCFlow(H, W, D, winSize=win)
    forms = [0, LOOP, BOX] + ([DOT4] if 2 * win + 1 <= 31 else [])
    for form in forms:
        for lr in (KEYS, COMPOSED):
            flow.set_form(form)
            smt.lrncc_set_impl(lr)
            dl, dr, last, cls = flow.run_both(T(Ls), T(Rs))
            ran, left = smt.lrncc_last_form(), smt.ncc_last_form()
            assert left == form or form == 0
            assert ran == (KEYS if left != LOOP and lr == KEYS else COMPOSED)
            want_l = flow.run(T(Ls), T(Rs))
            assert torch.equal(dl, want_l)
            for b in range(P):
                d1l, d1r, _, _, _ = both(smt, Ls[b], Rs[b], D, win, left, lr, want_cost=False)
                assert np.array_equal(dl[b].cpu().numpy(), d1l) and np.array_equal(dr[b].cpu().numpy(), d1r), (form, lr, b)
            wl, wc = _crosscheck(smt, dl, dr)
            assert torch.equal(last, wl) and torch.equal(cls, wc)
            dl, dr, last, cls = (t.cpu().numpy() for t in (dl, dr, last, cls))
            smt.lrncc_set_impl(lr)

            for outs in (LC.OUTS, ("dispR",), ("lastdisp",), ("dispL", "cls")):
                def make(A, outs=outs):
                    A.inp("L", Ls)
                    A.inp("R", Rs)
                    for nm in outs:
                        A.out(nm, (P, H, W), np.uint8 if nm == "cls" else np.int32)
                    st = smt.current_stream_ptr()
                    return lambda A: (lib().smt_ncc_flow_set_stream(flow._h, st) or
                                      lib().smt_lrncc_flow_run_batch(flow._h, A.ptr("L"), A.ptr("R"), P,
                                                                     *[A.ptr(nm if nm in outs else None) for nm in LC.OUTS]))

                def held(o, what, outs=outs):
                    for nm, ref in zip(LC.OUTS, (dl, dr, last, cls)):
                        if nm in outs:
                            assert np.array_equal(o[nm], ref), (form, lr, outs, nm, what)

                o, _ = arena.run_two_seeds(make, DEV, torch.cuda.synchronize)  # guards, inputs, both prefills, both seeds equal
                held(o, "warm")
                if outs in (LC.OUTS, ("lastdisp",)):
                    for byte in (0xFF, 0x00):
                        smt.scratch_poison(byte)
                        o, _ = arena.run_two_seeds(make, DEV, torch.cuda.synchronize)
                        held(o, f"scratch {byte:#x}")
    flow.close()


def test_flow_on_a_reused_handle_alternates_with_run_batch(hooks, O):
    smt = hooks
    H, W, D, win = 10, 80, 66, 2
    batches = [_pairs(O, H, W, P, 40 + P) for P in (2, 4, 1)]
    flow = smt.NCCFlow(H, W, D, winSize=win)
    smt.lrncc_set_impl(KEYS)
    first = None
    for k, (Ls, Rs) in enumerate(batches + batches[:1]):
        for form in (DOT4, BOX):
            flow.set_form(form)
            single_view = flow.run(T(Ls), T(Rs))                               # run_batch in between, on the same tables
            dl, dr, last, cls = flow.run_both(T(Ls), T(Rs))
            assert smt.lrncc_last_form() == KEYS
            assert torch.equal(dl, single_view)
            for b in range(Ls.shape[0]):
                dm, _ = mirrored(smt, Ls[b], Rs[b], D, win, form)
                assert np.array_equal(dr[b].cpu().numpy(), dm), (k, form, b)
            wl, wc = _crosscheck(smt, dl, dr)
            assert torch.equal(last, wl) and torch.equal(cls, wc)
            again = flow.run(T(Ls), T(Rs))
            assert torch.equal(again, single_view)
        if k == 0:
            first = (dl.clone(), dr.clone(), last.clone(), cls.clone())
    for a, b in zip(first, (dl, dr, last, cls)):                               # the first batch again: the same bits
        assert torch.equal(a, b)
    flow.close()


def test_flow_edges_and_rejections(hooks, O):
    smt = hooks
    from stereo_match_traditional_amd import _lib as Lb
    lib = Lb.lib()
    H, W, D, win = 12, 40, 20, 2
    Ls, Rs = _pairs(O, H, W)
    tl, tr = T(Ls), T(Rs)
    p = lambda t: C.c_void_p(t.data_ptr())
    flow = smt.NCCFlow(H, W, D, winSize=win)
    lib.smt_ncc_flow_set_stream(flow._h, smt.current_stream_ptr())
    maps = [torch.full((3, H, W), -5, dtype=torch.int32, device=DEV) for _ in range(3)]
    cls = torch.full((3, H, W), 77, dtype=torch.uint8, device=DEV)
    outs = [p(m) for m in maps] + [p(cls)]
    # pairs == 0 touches nothing
    assert lib.smt_lrncc_flow_run_batch(flow._h, p(tl), p(tr), 0, *outs) == 0
    assert lib.smt_lrncc_flow_run_batch(flow._h, None, None, 0, None, None, None, None) == 0
    # the rejections launch nothing
    assert lib.smt_lrncc_flow_run_batch(flow._h, p(tl), p(tr), -1, *outs) == SMT_ERR_ARG
    assert lib.smt_lrncc_flow_run_batch(flow._h, p(tl), p(tr), 32768, *outs) == SMT_ERR_ARG
    assert lib.smt_lrncc_flow_run_batch(flow._h, None, p(tr), 3, *outs) == SMT_ERR_ARG
    assert lib.smt_lrncc_flow_run_batch(flow._h, p(tl), None, 3, *outs) == SMT_ERR_ARG
    assert lib.smt_lrncc_flow_run_batch(None, p(tl), p(tr), 3, *outs) == SMT_ERR_ARG
    st = smt.current_stream_ptr()
    for hh, ww, dd, w_ in [(H, W, 0, win), (H, W, -1, win), (H, W, 513, win), (H, W, D, -1), (0, W, D, win), (H, 0, D, win)]:
        assert lib.smt_lrncc(p(tl), p(tr), hh, ww, dd, w_, outs[0], outs[1], None, None, st) == SMT_ERR_ARG, (hh, ww, dd, w_)
    assert lib.smt_lrncc(p(tl), p(tr), H, W, D, win, None, outs[1], None, None, st) == SMT_ERR_ARG
    assert lib.smt_lrncc(p(tl), p(tr), H, W, D, win, outs[0], None, None, None, st) == SMT_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((m == -5).all()) for m in maps) and bool((cls == 77).all())
    # every output NULL: nothing to do
    assert lib.smt_lrncc_flow_run_batch(flow._h, p(tl), p(tr), 3, None, None, None, None) == 0
    flow.close()
    # an empty interior: zero maps, and the cross-check of zero maps
    He, We, wine = 8, 40, 4
    Le, Re = _pairs(O, He, We)
    f = smt.NCCFlow(He, We, 5, winSize=wine)
    for form in (0, LOOP, DOT4, BOX):
        f.set_form(form)
        dl, dr, last, c = f.run_both(T(Le), T(Re))
        assert bool((dl == 0).all()) and bool((dr == 0).all())
        wl, wc = _crosscheck(smt, dl, dr)
        assert torch.equal(last, wl) and torch.equal(c, wc)
    f.close()
    dl, dr, cl, cr, _ = both(smt, Le[0], Re[0], 5, wine, 2, 0)
    assert (dl == 0).all() and (dr == 0).all() and (cl.view(np.uint64) == 0).all() and (cr.view(np.uint64) == 0).all()


# ------------------------------------------------------------------------------------------ the bounds suite's rows
@pytest.fixture(scope="module")
def BX(smt, O):
    return BC.Ctx(O, "cuda:0")


@pytest.mark.parametrize("params", LC.LRNCC_CASES, ids=[BC.case_id(p) for p in LC.LRNCC_CASES])
def test_lrncc_in_the_bounds_suite(BX, params):
    BC.run_case(BX, "smt_lrncc", params)


@pytest.mark.parametrize("params", LC.FLOW_CASES, ids=[BC.case_id(p) for p in LC.FLOW_CASES])
def test_flow_in_the_bounds_suite(BX, params):
    BC.run_case(BX, "smt_lrncc_flow_run_batch", params)


# ------------------------------------------------------------------------------------------ 6. the sharding unit
def test_shard_ncc_both_batch_under_a_world_size_1_group(hooks, O):
    import torch.distributed as dist
    from stereo_match_traditional_amd import shard
    smt = hooks
    H, W, D, win = 12, 40, 20, 2
    Ls, Rs = _pairs(O, H, W)
    flow = smt.NCCFlow(H, W, D, winSize=win)
    wl, wr, _, _ = flow.run_both(T(Ls), T(Rs))
    flow.close()
    assert not torch.equal(wl, wr)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        def compute(a, b, d):
            dl, dr = shard.ncc_both_batch(a, b, d, winSize=win)
            return dl.cpu(), dr.cpu()
        gl, gr = shard.run_sharded(T(Ls), T(Rs), D, compute)
        assert torch.equal(gl, wl.cpu()) and torch.equal(gr, wr.cpu())
    finally:
        dist.destroy_process_group()
    el, er = shard.ncc_both_batch(T(Ls)[:0], T(Rs)[:0], D, winSize=win)
    assert el.shape == (0, H, W) and er.shape == (0, H, W) and el.dtype == torch.int32
