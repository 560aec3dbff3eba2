"""smt_whole_ncc, smt_bgr_to_grey_batch and smt_whole_ncc_flow_run_batch on the device.

Costs: the integer form within 10 * 2^-53 relative of the exact rational function, the loop nest within
(12 N + 24) * 2^-53 / n absolute (both derived in tests/ncc_whole_cases.py, neither measured), NaN exactly where Ai Bi == 0.
Maps: the offset map is the sequential winner rule on the call's own costs, exactly; depth == (uint8)(3 * offset); the map
equals the reference's recorded one except where the exact values of the two choices lie closer than the sum of the two
bounds, at no more than 0.5 % of a case's pixels; pixels at which every offset is NaN are 0.
Everything else is bit for bit: both forms against their NumPy restatements (the same IEEE operations in the same
order), the flow against the single calls, lastdisp and cls against smt_sad_crosscheck of the flow's own offset maps.

Largest observed errors in units of the bounds on the six fixture pairs (MI355X): see DESIGN.md section 2; the test prints
them (pytest -s)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import bounds_cases as BC  # noqa: E402
import ncc_whole_cases as WC  # noqa: E402
import make_ncc_whole_golden as MG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K, O = 5, 79
TYPES = {WC.VL: "left", WC.VR: "right"}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def hooks(smt):
    yield smt
    smt.ncc_whole_set_impl(0)
    smt.ncc_whole_set_groups(0)


@pytest.fixture(scope="module")
def FX():
    return dict(np.load(MG.OUT))


@pytest.fixture(scope="module")
def PAIRS():
    return {n: (L, R) for n, L, R in WC.fixture_pairs()}


@pytest.fixture(scope="module")
def EXACT(PAIRS):
    """{(name, view): (exact, flat)} of the fixture pairs, computed once and left unchanged"""
    return {(n, v): WC.exact_ld(L, R, K, O, v) for n, (L, R) in PAIRS.items() for v in (WC.VL, WC.VR)}


def run(smt, L, R, k, o, view, impl, addc=False, want_cost=True):
    """-> (depth, offset, cost or None, form) as numpy"""
    smt.ncc_whole_set_impl(impl)
    out = smt.ncc(T(L), T(R), TYPES[view], add_constant=addc, kernel_size=k, max_offset=o, want_offset=True, want_cost=want_cost)
    form = smt.ncc_whole_last_form()
    out = [t.cpu().numpy() for t in out] + ([] if want_cost else [None])
    return (*out, form)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def hold_to_restatement(smt, L, R, k, o, view, impl, addc=False):
    """one call against the NumPy restatement of its form: costs bit for bit, maps exactly -> (depth, offset, cost)"""
    d, off, c, form = run(smt, L, R, k, o, view, impl, addc)
    assert form == WC.form_for(k, impl)
    rc, roff = WC.reference(L, R, k, o, view, form, addc)
    BC.nan_bits_eq(c, rc, f"cost, form {form}, view {view}")
    assert np.array_equal(off, WC.winner(c)), "offset != the sequential winner of the call's own costs"
    assert np.array_equal(off, roff)
    assert np.array_equal(d, (3 * off).astype(np.uint8)), "depth != (uint8)(3 * offset)"
    d2, off2, _, f2 = run(smt, L, R, k, o, view, impl, addc, want_cost=False)
    assert f2 == form and np.array_equal(d2, d) and np.array_equal(off2, off), "want_cost on and off"
    return d, off, c


# ------------------------------------------------------------------------------------------------- 1. the fixture pairs
@pytest.mark.parametrize("name", [n for n, _, _ in WC.fixture_pairs()])
def test_fixture_pairs(hooks, FX, PAIRS, EXACT, name):
    L, R = PAIRS[name]
    for view in (WC.VL, WC.VR):
        exact, flat = EXACT[name, view]
        want = FX[f"{name}_{TYPES[view]}"]
        bl = WC.bound_of(WC.LOOP, exact, K)                   # the recorded maps are a loop nest's
        offs = {}
        for form in (WC.INT, WC.LOOP):
            d, off, c, f = run(hooks, L, R, K, O, view, form)
            assert f == form
            worst = WC.check_costs(c, exact, flat, form, K)
            print(f"{name} {TYPES[view]} form {form}: largest error {worst:.3f} bounds")
            assert np.array_equal(off, WC.winner(c)), "offset != the sequential winner of the call's own costs"
            assert np.array_equal(d, (3 * off).astype(np.uint8))
            allnan = flat.all(axis=2)
            assert (d[allnan] == 0).all() and (off[allnan] == 0).all(), "a pixel with every offset NaN must be 0"
            assert ((off == 0) == allnan).all()
            # against the recorded map: where the depths differ the offsets do, and the excuse is stated on offsets
            ref_off = np.where(d == want, off, -1)
            bad = np.argwhere(d != want)
            for y, x in bad:
                cands = [o for o in range(1, O + 1) if (3 * o) % 256 == int(want[y, x])]
                assert len(cands) == 1 and not allnan[y, x], f"pixel ({y}, {x}): the recorded depth {want[y, x]} names no single offset"
                ref_off[y, x] = cands[0]
            need = WC.excused(off, ref_off.astype(np.int32), exact, WC.bound_of(form, exact, K), bl)
            if form == WC.INT:
                assert need == 0, f"{need} pixels needed the excuse; the integer form needed none when the fixture was made"
            d2, off2, _, _ = run(hooks, L, R, K, O, view, form, want_cost=False)
            assert np.array_equal(d2, d) and np.array_equal(off2, off), "want_cost on and off give the same maps"
            offs[form] = (off, c)
        WC.excused(offs[WC.INT][0], offs[WC.LOOP][0], exact, WC.bound_of(WC.INT, exact, K), bl)
        assert np.array_equal(np.isnan(offs[WC.INT][1]), np.isnan(offs[WC.LOOP][1])), "the two forms' NaN patterns"


def test_shared_cost_identity(hooks, PAIRS):
    """left cost at (y, x, o) == right cost at (y, x - o, o) word for word wherever x - k >= o and x + k <= W - 1"""
    words = 0
    for name in ("9x83_noise", "14x100_patches"):
        L, R = PAIRS[name]
        W = L.shape[1]
        cl, cr = run(hooks, L, R, K, O, WC.VL, WC.INT)[2], run(hooks, L, R, K, O, WC.VR, WC.INT)[2]
        for o in range(1, O + 1):
            xs = np.arange(o + K, W - K)
            if len(xs):
                a, b = np.ascontiguousarray(cl[:, xs, o - 1]), np.ascontiguousarray(cr[:, xs - o, o - 1])
                assert same_bits(a, b), (name, o)
                words += a.size
    assert words > 10000


# ---------------------------------------------------------------------------- 2. the smallest shapes that can go wrong
@pytest.mark.parametrize("H,W,k,o", WC.SHAPES, ids=[f"{h}x{w}-k{k}-O{o}" for h, w, k, o in WC.SHAPES])
def test_shapes_against_the_restatements(hooks, H, W, k, o):
    L, R = WC.pair(H, W, "noise", 40 + H + W)
    for view in (WC.VL, WC.VR):
        for impl in (2, 1):
            hold_to_restatement(hooks, L, R, k, o, view, impl)


@pytest.mark.parametrize("H,W,k,o,s", [(3, 100, 2, 90, 88), (2, 270, 1, 255, 200)])
def test_uchar_wrap(hooks, H, W, k, o, s):
    """(uchar)(3 o) wraps from o = 86 on: a pair whose true offset is s"""
    L = BC.rb((H, W), 3)
    R = BC.rb((H, W), 4)
    R[:, :W - s] = L[:, s:]
    for impl in (2, 1):
        d, off, _ = hold_to_restatement(hooks, L, R, k, o, WC.VL, impl)
        assert (off[:, s + k:W - k] == s).all() and (d[:, s + k:W - k] == (3 * s) % 256).all() and 3 * s > 255


@pytest.mark.parametrize("k,form", [(35, WC.INT), (36, WC.LOOP)])
def test_either_side_of_the_integer_limit(hooks, k, form):
    L, R = WC.pair(3, 80, "noise", 77)
    L[:, :40] = 255; R[:, :44] = 255                          # the largest sums the limit is derived for
    for impl in (0, 2):
        d, off, c, f = run(hooks, L, R, k, 3, WC.VL, impl)
        assert f == form, "kernel_size 35 is the last the integer form takes"
        rc, roff = WC.reference(L, R, k, 3, WC.VL, form)
        BC.nan_bits_eq(c, rc, "cost")
        assert np.array_equal(off, roff) and np.array_equal(d, (3 * off).astype(np.uint8))
    exact, flat = WC.exact_ld(L, R, k, 3, WC.VL)
    WC.check_costs(c, exact, flat, form, k)


def test_offset_rules(hooks):
    from stereo_match_traditional_amd import SmtError
    L, R = WC.pair(4, 20, "noise", 5)
    hold_to_restatement(hooks, L, R, 3, 20, WC.VR, 2)          # O == W is defined: every column is fill at o = W
    hold_to_restatement(hooks, L, R, 3, 1, WC.VL, 2)           # O == 1
    for view in (WC.VL, WC.VR):
        with pytest.raises(SmtError) as e:
            run(hooks, L, R, 3, 21, view, 0)
        assert e.value.status == BC.SMT_ERR_REF_UB
    for bad in (dict(k=0, o=3), dict(k=2, o=0), dict(k=2, o=513)):
        with pytest.raises(SmtError) as e:
            run(hooks, *WC.pair(4, 600, "noise", 5), bad["k"], bad["o"], WC.VL, 0)
        assert e.value.status == -1
    with pytest.raises(SmtError):
        run(hooks, L[:1], R[:1], 2, 3, WC.VL, 0)               # H < 2


@pytest.mark.parametrize("impl", [2, 1])
def test_hostile_images(hooks, impl):
    H, W, k, o = 9, 40, 2, 12
    zero = np.zeros((H, W), np.uint8)
    L, R = WC.pair(H, W, "noise", 9)
    for view, (a, b) in ((WC.VL, (zero, R)), (WC.VR, (L, zero)), (WC.VL, (zero, zero))):
        d, off, c, _ = run(hooks, a, b, k, o, view, impl)
        assert np.isnan(c).all() and (d == 0).all() and (off == 0).all(), "an all-zero image: every cost NaN, every pixel 0"
    const = np.full((H, W), 93, np.uint8)
    d, off, c = hold_to_restatement(hooks, const, np.full((H, W), 201, np.uint8), k, o, WC.VL, impl)
    h, w = WC.extents(H, W, k)
    assert (off == 1).all(), "constant windows tie at every offset: the first stays"
    assert np.allclose(c, (1.0 / ((h - 1) * (w - 1)))[:, :, None], rtol=1e-13, atol=0), "a constant window scores 1 / n"
    # the best offset in the fill region: R equals L on the first columns and is unrelated elsewhere, so a left pixel near
    # the left edge matches only at offsets that leave its whole window unshifted (o > x + k)
    Lf, Rf = WC.pair(H, W, "noise", 10)
    Rf = np.random.default_rng(2).integers(0, 256, (H, W)).astype(np.uint8)
    Rf[:, :8] = Lf[:, :8]
    d, off, c = hold_to_restatement(hooks, Lf, Rf, k, o, WC.VL, impl)
    assert (off[:, :4] == np.arange(4)[None, :] + k + 1).all(), "the first offset whose window is all fill wins"
    # add_constant: min(R + 10, 255) on a copy; the caller's image stays
    La, Ra = WC.pair(H, W, "noise", 11)
    Ra = (228 + Ra % 28).astype(np.uint8)                      # 228 .. 255: many bytes saturate
    assert (Ra > 245).sum() > 50
    Rt = T(Ra)
    hooks.ncc_whole_set_impl(impl)
    dd, oo = hooks.ncc(T(La), Rt, "right", add_constant=True, kernel_size=k, max_offset=o, want_offset=True)
    assert np.array_equal(Rt.cpu().numpy(), Ra), "add_constant must leave the caller's image alone"
    rc, roff = WC.reference(La, Ra, k, o, WC.VR, WC.form_for(k, impl), addc=True)
    assert np.array_equal(oo.cpu().numpy(), roff) and np.array_equal(dd.cpu().numpy(), (3 * roff).astype(np.uint8))
    assert not np.array_equal(roff, WC.reference(La, Ra, k, o, WC.VR, WC.form_for(k, impl))[1]), "the case must feel the constant"


def test_bgr_to_grey(smt, FX):
    bgr = WC.fixture_bgr()
    assert np.array_equal(smt.bgr_to_grey(T(bgr)).cpu().numpy(), FX["grey"])
    batch = BC.rb((3, 5, 65, 3), 4)
    assert np.array_equal(smt.bgr_to_grey(T(batch)).cpu().numpy(), WC.bgr_to_grey(batch))


# ------------------------------------------------------------------------------------------------------- 3. the flow
def flow_call(smt, h, L, R, outs):
    """the C entry on prefilled tensors `outs` ({name: tensor}; a name left out is passed as NULL)"""
    from stereo_match_traditional_amd._lib import lib, check
    P = L.shape[0]
    check(lib().smt_whole_ncc_flow_set_stream(h._h, smt.current_stream_ptr(DEV)), "set_stream")
    check(lib().smt_whole_ncc_flow_run_batch(h._h, C.c_void_p(L.data_ptr()), C.c_void_p(R.data_ptr()), P,
                                             *[C.c_void_p(outs[n].data_ptr()) if n in outs else None for n in WC.OUTS]), "run_batch")


def prefilled(P, H, W, names, fill):
    return {n: torch.full((P, H, W), fill, dtype=torch.int32 if n in ("offL", "offR", "lastdisp") else torch.uint8, device=DEV)
            for n in names}


def singles(smt, Ls, Rs, k, o, impl):
    """{name: [P][H][W]} from single-view calls and the device cross-check of their offset maps"""
    out = {n: [] for n in WC.OUTS}
    for L, R in zip(Ls, Rs):
        dl, ol, _, _ = run(smt, L, R, k, o, WC.VL, impl, want_cost=False)
        dr, orr, _, _ = run(smt, L, R, k, o, WC.VR, impl, want_cost=False)
        last, cls = smt.sad_CrossCheckDiaparity(T(ol), T(orr))
        for n, v in zip(WC.OUTS, (dl, dr, ol, orr, last.cpu().numpy(), cls.cpu().numpy())):
            out[n].append(v)
    return {n: np.stack(v) for n, v in out.items()}


@pytest.mark.parametrize("form", [WC.INT, WC.LOOP])
@pytest.mark.parametrize("H,W,k,o", [(9, 83, 5, 79), (5, 33, 1, 12), (19, 21, 5, 10)])
def test_flow_equals_the_single_calls(hooks, H, W, k, o, form):
    sets = {P: ([WC.pair(H, W, "noise", 60 + 5 * P + b)[0] for b in range(P)], [WC.pair(H, W, "noise", 60 + 5 * P + b)[1] for b in range(P)])
            for P in (3, 1, 2)}
    want = {P: singles(hooks, *sets[P], k, o, form) for P in sets}
    hooks.ncc_whole_set_impl(0)
    h = hooks.NCCWholeFlow(H, W, DEV, kernel_size=k, max_offset=o).set_form(form)
    try:
        # a reused handle: three batches with different pair counts, then the first again, into prefilled outputs
        for fill, P in enumerate((3, 1, 2, 3)):
            outs = prefilled(P, H, W, WC.OUTS, 7 + 50 * fill)
            flow_call(hooks, h, T(np.stack(sets[P][0])), T(np.stack(sets[P][1])), outs)
            assert hooks.ncc_whole_last_form() == form
            for n in WC.OUTS:
                assert np.array_equal(outs[n].cpu().numpy(), want[P][n]), (n, P)
            last, cls = [], []
            for b in range(P):                                 # lastdisp, cls == smt_sad_crosscheck of the flow's own maps
                l, c = hooks.sad_CrossCheckDiaparity(outs["offL"][b].contiguous(), outs["offR"][b].contiguous())
                last.append(l); cls.append(c)
            assert torch.equal(torch.stack(last), outs["lastdisp"]) and torch.equal(torch.stack(cls), outs["cls"])
        # optional outputs: what is not asked for stays as it was; the others do not change
        part = prefilled(3, H, W, ("depthR", "cls"), 9)
        flow_call(hooks, h, T(np.stack(sets[3][0])), T(np.stack(sets[3][1])), part)
        assert np.array_equal(part["depthR"].cpu().numpy(), want[3]["depthR"]) and np.array_equal(part["cls"].cpu().numpy(), want[3]["cls"])
        got = h.run(T(np.stack(sets[2][0])), T(np.stack(sets[2][1])), want=("offL", "lastdisp"))
        assert [g is None for g in got] == [True, True, False, True, False, True]
        assert np.array_equal(got[2].cpu().numpy(), want[2]["offL"]) and np.array_equal(got[4].cpu().numpy(), want[2]["lastdisp"])
    finally:
        h.close()


def test_flow_rejects_and_noops(hooks):
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import lib
    with pytest.raises(SmtError) as e:
        hooks.NCCWholeFlow(4, 20, DEV, kernel_size=3, max_offset=21)
    assert e.value.status == BC.SMT_ERR_REF_UB
    h = hooks.NCCWholeFlow(3, 80, DEV, kernel_size=36, max_offset=3)
    try:
        with pytest.raises(SmtError):
            h.set_form(WC.INT)                                 # beyond the integer limit
        outs = prefilled(1, 3, 80, WC.OUTS, 5)
        L = T(np.zeros((1, 3, 80), np.uint8))
        assert lib().smt_whole_ncc_flow_run_batch(h._h, C.c_void_p(L.data_ptr()), C.c_void_p(L.data_ptr()), 0,
                                                  *[C.c_void_p(outs[n].data_ptr()) for n in WC.OUTS]) == 0
        torch.cuda.synchronize()
        assert all((outs[n] == 5).all() for n in WC.OUTS), "pairs == 0 is a no-op"
    finally:
        h.close()


def test_shard_batch_equals_the_flow(hooks):
    from stereo_match_traditional_amd import shard
    H, W, k, o = 6, 50, 2, 15
    Ls = np.stack([WC.pair(H, W, "smooth", 80 + b)[0] for b in range(3)])
    Rs = np.stack([WC.pair(H, W, "smooth", 80 + b)[1] for b in range(3)])
    ol, orr = shard.ncc_whole_batch(T(Ls), T(Rs), o, kernel_size=k)
    h = hooks.NCCWholeFlow(H, W, DEV, kernel_size=k, max_offset=o)
    try:
        got = h.run(T(Ls), T(Rs))
    finally:
        h.close()
    assert torch.equal(ol, got[2]) and torch.equal(orr, got[3])
    z = shard.ncc_whole_batch(T(Ls[:0]), T(Rs[:0]), o, kernel_size=k)
    assert z[0].shape == (0, H, W)


# ---------------------------------------------------------------------------------- 4. the rows of the bounds table
_ROWS = [(n, p) for n in ("smt_whole_ncc", "smt_bgr_to_grey_batch", "smt_whole_ncc_flow_run_batch") for p in BC.CASES[n]]


@pytest.fixture(scope="module")
def X(smt, O):
    return BC.Ctx(O, "cuda:0")


@pytest.mark.parametrize("name,params", _ROWS, ids=[f"{n}-{BC.case_id(p)}" for n, p in _ROWS])
def test_guards_prefill_inputs_and_restatement(X, name, params):
    """pairs = 1 and 3 in an arena with guards on both sides of every tensor, under both fill seeds"""
    BC.run_case(X, name, params)


# ------------------------------------------------------------------------------------------------ 5. the C++ driver
def test_ncc_main_counterpart(smt, O, X):
    """host/ncc_main.cpp (NCC_main.cpp with :24 enabled, both types): its FNV-1a hashes against the restatement"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo_match_traditional_amd", "lib", "ncc_main")
    assert os.path.exists(exe), "run stereo_match_traditional_amd/build.py"
    H, W, seed, k, o = 20, 90, 3, 3, 30
    r = subprocess.run([exe, str(H), str(W), str(seed), str(k), str(o)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    L, R = O.synth_pair(H, W, o, seed)
    ref = WC.flow_reference(X, L, R, k, o, WC.INT)
    for name, key in (("left_disp", "depthL"), ("right_disp", "depthR"), ("offleft", "offL"), ("offright", "offR"), ("lastdisp", "lastdisp")):
        assert got[name] == f"{O.fnv1a(np.ascontiguousarray(ref[key])):016x}", name


# ----------------------------------------------------------------------------------- 6. runs of more than one offset
# Small images launch few workgroups, so a cost launch splits the offsets into G == O runs of one offset each.  Real sizes
# do not (450x375: 22 runs of 4): these cases run workgroups over several offsets -- the per-offset rebuild of the running
# sums, the LDS halves carried across offsets, ties and NaN inside a run, short and empty trailing runs, the finishing
# combine -- through the hook and at sizes that choose such a G by themselves.
_FLOW_REF = {}                    # the restatements of test_flow_in_runs, computed once
RUNS = [1, 3, 7, 40, 60]          # O = 79: one run; 27 + 27 + 25; 6 x 12 + 7; 39 x 2 + 1; 40 runs and 20 empty ones


@pytest.fixture(scope="module")
def PATCH_REFS(PAIRS):
    """{(name, view, form): (cost, offsets)} of the two 'patches' pairs (exact ties and NaN at consecutive offsets)"""
    return {(n, v, f): WC.reference(*PAIRS[n], K, O, v, f) for n in ("9x83_patches", "14x100_patches") for v in (WC.VL, WC.VR)
            for f in (WC.INT, WC.LOOP)}


@pytest.mark.parametrize("G", RUNS)
@pytest.mark.parametrize("name", ["9x83_patches", "14x100_patches"])
def test_patches_pairs_in_runs(hooks, FX, PAIRS, PATCH_REFS, name, G):
    L, R = PAIRS[name]
    hooks.ncc_whole_set_groups(G)
    for view in (WC.VL, WC.VR):
        for form in (WC.INT, WC.LOOP):
            d, off, c, f = run(hooks, L, R, K, O, view, form)
            assert f == form and hooks.ncc_whole_last_groups() == G
            rc, roff = PATCH_REFS[name, view, form]
            BC.nan_bits_eq(c, rc, f"cost, form {form}, view {view}, G {G}")
            assert np.array_equal(off, roff) and np.array_equal(d, (3 * roff).astype(np.uint8))
            d2, off2, _, _ = run(hooks, L, R, K, O, view, form, want_cost=False)
            assert np.array_equal(d2, d) and np.array_equal(off2, off), "want_cost on and off"
            if form == WC.INT:
                assert np.array_equal(d, FX[f"{name}_{TYPES[view]}"]), "the recorded map"
    ties = np.isnan(PATCH_REFS[name, WC.VL, WC.INT][0])
    assert (ties[:, :, :-1] & ~ties[:, :, 1:]).any() and (PATCH_REFS[name, WC.VL, WC.INT][0][:, :, 1:] == PATCH_REFS[name, WC.VL, WC.INT][0][:, :, :-1]).any()


@pytest.mark.parametrize("H,W,k,o,G", [(7, 9, 5, 9, 4), (5, 33, 1, 12, 5), (19, 21, 5, 10, 3), (2, 260, 1, 255, 2), (3, 65, 5, 7, 1)])
def test_shapes_in_runs(hooks, H, W, k, o, G):
    """run lengths that do not divide O (9 = 3 + 3 + 3 + 0, 12 = 3 x 4 + 0, 10 = 4 + 4 + 2, 255 = 128 + 127) and G == 1"""
    L, R = WC.pair(H, W, "noise", 40 + H + W)
    hooks.ncc_whole_set_groups(G)
    for view in (WC.VL, WC.VR):
        for impl in (2, 1):
            hold_to_restatement(hooks, L, R, k, o, view, impl)
            assert hooks.ncc_whole_last_groups() == G


def test_sizes_that_choose_several_offsets_per_run(hooks):
    """no hook: 200x300 k = 5 O = 79 under INT launches 2 x 25 workgroups per run and takes G = 41, per = 2 (39 runs of 2,
    one of 1, one empty); 300x400 k = 1 O = 12 under LOOP launches 469 and takes G = 5, per = 3 (4 runs of 3, one empty)"""
    L, R = WC.pair(200, 300, "smooth", 21)
    for view in (WC.VL, WC.VR):
        d, off, _, f = run(hooks, L, R, 5, 79, view, 2, want_cost=False)
        assert f == WC.INT and hooks.ncc_whole_last_groups() == 41
        roff = WC.ref_int(L, R, 5, 79, view)[1]
        assert np.array_equal(off, roff) and np.array_equal(d, (3 * roff).astype(np.uint8))
    L, R = WC.pair(300, 400, "noise", 22)
    d, off, c, f = run(hooks, L, R, 1, 12, WC.VR, 1)
    assert f == WC.LOOP and hooks.ncc_whole_last_groups() == 5
    rc, roff = WC.ref_loops(L, R, 1, 12, WC.VR)
    BC.nan_bits_eq(c, rc, "cost")
    assert np.array_equal(off, roff) and np.array_equal(d, (3 * roff).astype(np.uint8))


@pytest.mark.parametrize("form", [WC.INT, WC.LOOP])
@pytest.mark.parametrize("G", [1, 3, 60])
def test_flow_in_runs(hooks, X, PAIRS, PATCH_REFS, form, G):
    """the flow under the hook, three pairs (one of them the 'patches' pair), against the restatements"""
    H, W = 9, 83
    imgs = [PAIRS["9x83_patches"], PAIRS["9x83_noise"], PAIRS["9x83_smooth"]]
    hooks.ncc_whole_set_groups(G)
    h = hooks.NCCWholeFlow(H, W, DEV, kernel_size=K, max_offset=O).set_form(form)
    try:
        got = dict(zip(WC.OUTS, h.run(T(np.stack([i[0] for i in imgs])), T(np.stack([i[1] for i in imgs])))))
        assert hooks.ncc_whole_last_groups() == G and hooks.ncc_whole_last_form() == form
    finally:
        h.close()
    for b, (L, R) in enumerate(imgs):
        if (form, b) not in _FLOW_REF:
            _FLOW_REF[form, b] = WC.flow_reference(X, L, R, K, O, form)
        for n in WC.OUTS:
            assert np.array_equal(got[n][b].cpu().numpy(), _FLOW_REF[form, b][n]), (n, b)
