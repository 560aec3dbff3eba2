"""The C++ host mirror (host/smt_host.hpp) on the device, entry by entry, against the oracle, bit for bit.

host/mirror_main.cpp reads raw input files, calls one mirror entry with host buffers carved out of guard bands, runs
the case under two prefills of its outputs (an element left unwritten differs between them: exit 4; a changed band:
exit 3) and writes every buffer back.  The references are the ones the parity tests of the C entries beneath use
(tests/bounds_cases.py and the per-family *_cases.py); none is restated here.  No tolerance appears: every entry
has a bit-exact reference, except the ASW maps, held by bounds_cases' own rule for them.

One test is one subprocess, one GPU process.  After a subprocess that died (time limit, abort, segmentation fault,
kill) nothing else of this module starts on the device."""
import os
import subprocess

import numpy as np
import pytest

import asw_tail_cases as ATC
import bounds_cases as BC
import cblsm_v4_cases as VC
import cblsm_window_cases as CW
import median_inplace_cases as MC
import ncc_whole_cases as NW
import subpixel_cases as SP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "mirror_main")
INT_MIN = -(2 ** 31)

_died = []      # set once: the first subprocess that did not end by itself


class Result:
    def __init__(self, d):
        self.d = d
        self.status = open(os.path.join(d, "status.txt")).read().splitlines()

    def out(self, name, dtype, shape):
        return np.fromfile(os.path.join(self.d, f"out_{name}.bin"), dtype=dtype).reshape(shape)

    def value(self, key):
        return [int(l.split()[1]) for l in self.status if l.split()[0] == key]


def mirror(smt, tmp_path, case, ints, inputs, expect=0):
    """write in_<name>.bin, run the case, check that the inputs came back as they went"""
    if _died:
        pytest.skip(f"an earlier mirror_main did not end by itself ({_died[0]}): nothing else starts on this device")
    assert os.path.exists(EXE), "run stereo_match_traditional_amd/build.py"
    for name, a in inputs.items():
        np.ascontiguousarray(a).tofile(tmp_path / f"in_{name}.bin")
    try:
        r = subprocess.run([EXE, case, str(tmp_path)] + [str(int(i)) for i in ints], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _died.append(f"{case}: time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _died.append(f"{case}: exit {r.returncode}")
    assert r.returncode == expect, (r.returncode, r.stderr)
    return Result(str(tmp_path))


def unchanged(res, inputs, skip=()):
    for name, a in inputs.items():
        if name not in skip:
            a = np.ascontiguousarray(a)
            BC.bits_eq(res.out(name, a.dtype, a.shape), a, f"input {name} was modified")


SMALL = [(5, 67), (1, 63)]


@pytest.mark.parametrize("H,W", SMALL)
def test_left_and_right_consistency_appends(smt, O, tmp_path, H, W):
    dL, dR = BC._lr_maps(H, W, 91)
    dL[0, ::7] = np.nan; dR[0, 3::11] = -4e9; dL[H - 1, 1::5] += 0.5          # bounds_cases._lrvariant's hostile entries
    pre_occ, pre_mis = np.array([[7, 7], [0, 0]], np.int32), np.array([[9, 1]], np.int32)
    inputs = dict(dispL=dL, dispR=dR, occ=pre_occ, mis=pre_mis)
    res = mirror(smt, tmp_path, "lar", (H, W, 1500), inputs)
    assert res.status[0] == "LeftAndRightConsistency ok"
    ref, cls, no, nm = O.lrcheck_variant(dL, dR, 1.5)
    BC.bits_eq(res.out("last", np.float32, (H, W)), ref, "lastDisp")
    assert res.value("len_occ") == [2 + no] and res.value("len_mis") == [1 + nm]
    BC.bits_eq(res.out("occ", np.int32, (-1, 2)), np.concatenate([pre_occ, np.argwhere(cls == 1).astype(np.int32)]), "occlusion list")
    BC.bits_eq(res.out("mis", np.int32, (-1, 2)), np.concatenate([pre_mis, np.argwhere(cls == 2).astype(np.int32)]), "mismatch list")
    unchanged(res, inputs, skip=("occ", "mis"))


@pytest.mark.parametrize("fix", [0, ATC.FIX_ROW_END])
@pytest.mark.parametrize("H,W", SMALL)
def test_fill_image_new(smt, tmp_path, H, W, fix):
    m = ATC._holey(H, W, 320, 1)[0]
    res = mirror(smt, tmp_path, "fill_image", (H, W, fix), dict(map=m, map_nocounts=m))
    assert res.status == ["FillImageNew ok"] * 2
    ref, counts, _ = ATC.ref_fill(m, fix)
    BC.bits_eq(res.out("map", np.uint8, (H, W)), ref, "map")
    BC.bits_eq(res.out("map_nocounts", np.uint8, (H, W)), ref, "map without counts")
    assert tuple(res.out("counts", np.int32, (2,))) == tuple(counts)


@pytest.mark.parametrize("wnd", [3, 5])
@pytest.mark.parametrize("H,W", SMALL)
def test_median_filter_in_place_and_aliased(smt, tmp_path, H, W, wnd):
    m = MC.rand_map(H, W, 5)
    res = mirror(smt, tmp_path, "median", (H, W, wnd), dict(map=m, aliased=m))
    assert res.status == ["MedianFilterInPlace ok", "MedianFilter ok"]
    ref = MC.oracle_inplace(m, wnd)
    assert H == 1 or MC.discriminates(m, wnd), "the recurrence must differ from the out-of-place filter on this map"
    BC.bits_eq(res.out("map", np.float32, (H, W)), ref, "MedianFilterInPlace")
    BC.bits_eq(res.out("aliased", np.float32, (H, W)), ref, "MedianFilter(d, d)")


@pytest.mark.parametrize("H,W", SMALL)
def test_bgr_to_grey(smt, tmp_path, H, W):
    bgr = BC.rb((H, W, 3), 340)
    res = mirror(smt, tmp_path, "grey", (H, W), dict(bgr=bgr))
    BC.bits_eq(res.out("grey", np.uint8, (H, W)), NW.bgr_to_grey(bgr), "grey")
    unchanged(res, dict(bgr=bgr))


@pytest.mark.parametrize("H,W,D", [(5, 33, 8), (5, 33, 65)])
def test_choose_arm_length(smt, O, tmp_path, H, W, D):
    _, _, aL, aR = BC._cblsm_arms(BC.Ctx(O), H, W, 42)
    inputs = dict(zip(("LL", "LR", "LUp", "LDown", "RL", "RR", "RUp", "RDown"), aL + aR))
    res = mirror(smt, tmp_path, "choose", (H, W, D), inputs)
    assert [l.split()[1] for l in res.status] == ["ok"] * 4
    for k, name in enumerate(("volL", "volR", "volUp", "volDown")):
        BC.bits_eq(res.out(name, np.int32, (H, W, D)), O.choose_arm_length(k, aL[k], aR[k] if k >= 2 else None, aR[0], aR[1], D).astype(np.int32), name)
    unchanged(res, inputs)


def _v4_inputs(H, W, D):
    vol = (np.random.default_rng(H * 100 + D).standard_normal((H, W, D)) * 37.0).astype(np.float32)
    return vol, VC.random_arm_volumes(H, W, D, seed=D)


@pytest.mark.parametrize("H,W,D", [(5, 33, 8), (5, 33, 65)])
def test_cost_aggregation_v4(smt, tmp_path, H, W, D):
    vol, arms = _v4_inputs(H, W, D)
    inputs = dict(vol=vol, aL=arms[0], aR=arms[1], aUp=arms[2], aDown=arms[3])
    res = mirror(smt, tmp_path, "v4", (H, W, D), inputs)
    assert res.status == ["costAggregationV4 ok"]
    ref = VC.v4_numpy(vol, *arms)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert VC.same_volume(res.out("out", np.float32, (H, W, D)), ref), "CostVolume"
    unchanged(res, inputs)


def test_cost_aggregation_v4_rectangle_leaves_the_plane(smt, tmp_path):
    """the reference reads out of bounds there: the mirror throws, and CostVolume is written all the same"""
    H, W, D = 5, 33, 8
    vol, arms = _v4_inputs(H, W, D)
    inside = [a.copy() for a in arms]
    for v, (at, val) in enumerate(((2, 0), (1, 1), (0, 0), (1, 1))):       # L, R, up, down at (2, 0, 3): one row, columns [-2, 1)
        arms[v][2, 0, 3], inside[v][2, 0, 3] = at, val
    res = mirror(smt, tmp_path, "v4", (H, W, D), dict(vol=vol, aL=arms[0], aR=arms[1], aUp=arms[2], aDown=arms[3]))
    assert len(res.status) == 1 and res.status[0].startswith("costAggregationV4 threw")
    got, ref = res.out("out", np.float32, (H, W, D)).copy(), VC.v4_numpy(vol, *inside).copy()
    got[2, 0, 3] = ref[2, 0, 3] = 0                      # the clipped hypothesis is unspecified
    assert VC.same_volume(got, ref), "CostVolume of the hypotheses that stay inside"


@pytest.mark.parametrize("H,W,D,ws", [(3, 33, 65, 0), (5, 65, 8, 1)])
def test_compute_disp_v4(smt, tmp_path, H, W, D, ws):
    Lp, Rp = CW.pair(H, W, ws, 7, channels=3)
    res = mirror(smt, tmp_path, "dispv4", (H, W, D, ws), dict(Lp=Lp, Rp=Rp))
    assert res.status == ["ComputeDispV4 ok"]
    BC.bits_eq(res.out("vol", np.float32, (H, W, D)), CW.ref_volume(Lp, Rp, D, ws, 3), "dispVolume")
    unchanged(res, dict(Lp=Lp, Rp=Rp))


@pytest.mark.parametrize("H,W,D,ws", [(5, 33, 8, 2), (5, 33, 65, 1)])         # padded widths 39 and 37: (W + 2w) % 4 != 0
def test_get_point_depth_both(smt, O, tmp_path, H, W, D, ws):
    assert (W + 2 * (ws + 1)) % 4 != 0
    _, _, Lp, Rp = BC._padded(H, W, ws + 1, 100)
    res = mirror(smt, tmp_path, "sad", (H, W, D, ws), dict(Lp=Lp, Rp=Rp))
    assert [l.split()[1] for l in res.status] == ["ok"] * 3
    for view, single, both in ((0, "left", "bothL"), (1, "right", "bothR")):
        ref = O.sad(Lp, Rp, D, ws, view).astype(np.int32)
        BC.bits_eq(res.out(single, np.int32, (H, W)), ref, single)
        BC.bits_eq(res.out(both, np.int32, (H, W)), ref, both)
    unchanged(res, dict(Lp=Lp, Rp=Rp))


@pytest.mark.parametrize("H,W,D,ws", [(5, 33, 8, 2), (5, 33, 65, 1)])
def test_adaptive_support_weight_single_view(smt, O, tmp_path, H, W, D, ws):
    assert (W + 2 * (ws + 1)) % 4 != 0
    _, _, Lp, Rp = BC._padded(H, W, ws + 1, 160)
    sp, cm = O.asw_masks(ws, 50.0, 30.0)
    res = mirror(smt, tmp_path, "asw", (H, W, D, ws, 40), dict(Lp=Lp, Rp=Rp))
    assert res.status == ["AdaptiveSupportWeight ok"] * 2
    for view, name in ((0, "left"), (1, "right")):
        BC._asw_map_check(BC.Ctx(O), res.out(name, np.float32, (H, W)), Lp, Rp, D, ws, sp, cm, view, name)
    unchanged(res, dict(Lp=Lp, Rp=Rp))


@pytest.mark.parametrize("iters", [1, 4])
def test_cross_aggregator(smt, O, tmp_path, iters):
    H, W, D = 5, 33, 8
    bgr = BC._bgr_of(VC.noisy_pair(H, W, 70)[0], 71)
    cost = BC.rf((H, W, D), 72)
    res = mirror(smt, tmp_path, "crossagg", (W, H, D, iters), dict(img=bgr, cost=cost))
    assert res.status == ["initialize 1", "cost_before_aggregate 1", "CrossAggregator ok"]
    a_ref, c_ref = O.crossagg(bgr, cost, iters=iters)
    BC.bits_eq(res.out("arms", np.uint8, (H, W, 4)), a_ref, "arms")
    BC.bits_eq(res.out("agg", np.float32, (H, W, D)), c_ref, "aggregated volume")
    unchanged(res, dict(img=bgr, cost=cost))


@pytest.mark.parametrize("D", [1, 2, 65])
def test_wta_subpixel(smt, O, tmp_path, D):
    H, W = 3, 65
    vol = SP.volume(D, (H, W))
    md = 2.0 ** -20
    res = mirror(smt, tmp_path, "subpixel", (H, W, D, int(np.float32(md).view(np.uint32))), dict(vol=vol))
    assert res.status == ["WTASubpixel ok"] * 2
    BC.nan_bits_eq(res.out("disp", np.float32, (H, W)), SP.restate(O, vol, md), "disp")
    BC.nan_bits_eq(res.out("disp_default", np.float32, (H, W)), SP.restate(O, vol, 1.0), "disp at the default min_den")
    unchanged(res, dict(vol=vol))


def test_pipeline_one_handle_three_batches(smt, O, tmp_path):
    """RunBatch with 2, 1 and 3 pairs on one handle: integer maps, setSubpixel(1.0f), setSubpixel(0) again, against the
    composition from the oracle that test_subpixel_gpu.py builds"""
    H, W, D = 9, 65, 8
    pairs = []
    for b in range(3):
        L, R = O.synth_pair(H, W, D, 30 + b)
        al, oob_l = O.aggregate_rect(O.adcensus_view(L, R, D, 10.0, 30.0, 0), O.arms_all(L, right_row_bug=False), 0)
        ar, oob_r = O.aggregate_rect(O.adcensus_view(L, R, D, 10.0, 30.0, 1), O.arms_all(R, right_row_bug=False), 0)
        assert oob_l == 0 and oob_r == 0
        pairs.append((L, R, O.scanline(al, L.astype(np.float32), 10, 150), ar))
    Lb, Rb = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    # at 9 x 65 the reference's right-arm stride defect sends rectangles out of the plane (SMT_ERR_REF_UB): setQuirks undoes it
    res = mirror(smt, tmp_path, "pipeline", (H, W, D, 0x1), dict(L=Lb, R=Rb))
    assert res.status == ["Pipeline ok"]
    for state, min_den in (("int", None), ("sub", 1.0), ("again", None)):
        pick = O.wta if min_den is None else (lambda v: SP.restate(O, v, min_den))
        for n in (2, 1, 3):
            t = f"{state}{n}"
            dl, dr, cls = res.out("dl_" + t, np.float32, (n, H, W)), res.out("dr_" + t, np.float32, (n, H, W)), res.out("cls_" + t, np.uint8, (n, H, W))
            for b in range(n):
                d_so, d_r = pick(pairs[b][2]), pick(pairs[b][3])
                lr, c_ref, _, _ = O.lrcheck(d_so, d_r, 2)
                BC.bits_eq(dl[b], lr.astype(np.float32), ("dispL", t, b))
                BC.bits_eq(dr[b], d_r.astype(np.float32), ("dispR", t, b))
                BC.bits_eq(cls[b], c_ref, ("cls", t, b))
    unchanged(res, dict(L=Lb, R=Rb))


def test_crossarm_class_methods(smt, O, tmp_path):
    """Aggregation (exclusive bounds), AggregationVertical, setSubpixel and WTA of CrossArmAggregation, at a shape of
    bounds_cases' smt_crossarm_aggregate"""
    H, W, D, md = 5, 65, 65, 0.5
    img = VC.noisy_pair(H, W, 33)[0]
    vol = BC.rf((H, W, D), 34)
    res = mirror(smt, tmp_path, "crossarm", (H, W, D, int(md * 1000)), dict(img=img, vol=vol))
    arms = O.arms_all(img)
    ref, oob = O.aggregate_rect(vol, arms, 0)
    assert oob == 0 and res.status[0] == "CrossArmAggregation ok"
    BC.bits_eq(res.out("vertical", np.float32, (H, W, D)), ref, "AggregationVertical")
    BC.bits_eq(res.out("wta", np.float32, (H, W)), O.wta(ref).astype(np.float32), "WTA")
    BC.bits_eq(res.out("wta_sub", np.float32, (H, W)), SP.restate(O, ref, md), "WTA after setSubpixel")
    BC.bits_eq(res.out("wta_again", np.float32, (H, W)), O.wta(ref).astype(np.float32), "WTA after setSubpixel(0)")
    ref2, bad = O.aggregate_rect(vol, arms, 2)
    assert res.status[1].split()[1] == ("threw" if bad else "ok")              # an empty rectangle is the reference's 0 / 0
    BC.nan_bits_eq(res.out("exclusive", np.float32, (H, W, D)), ref2, "Aggregation")
    unchanged(res, dict(img=img, vol=vol))


def test_scanline_class_methods(smt, O, tmp_path):
    """setSubpixel and WTA of ScanlineOptimizer at a shape of bounds_cases' smt_scanline_run"""
    H, W, D, md = 3, 6, 65, 0.5
    vol = BC.rf((H, W, D), 50)
    gray = BC.rb((H, W), 51).astype(np.float32)
    res = mirror(smt, tmp_path, "scanline", (H, W, D, int(md * 1000)), dict(vol=vol, gray=gray))
    assert res.status == ["ScanlineOptimizer ok"]
    ref = O.scanline(vol, gray, 10, 150)
    BC.bits_eq(res.out("wta", np.float32, (H, W)), O.wta(ref).astype(np.float32), "WTA")
    BC.bits_eq(res.out("wta_sub", np.float32, (H, W)), SP.restate(O, ref, md), "WTA after setSubpixel")
    BC.bits_eq(res.out("wta_again", np.float32, (H, W)), O.wta(ref).astype(np.float32), "WTA after setSubpixel(0)")
    unchanged(res, dict(vol=vol, gray=gray))


def test_adcensus_right_view_and_second_initialize(smt, O, tmp_path):
    """ComputeADcensusRight and GetPtrRight, then Initialize with other images on the live object: the host copies of
    the first pair must not be served again"""
    H, W, D = 5, 65, 8
    (L0, R0), (L1, R1) = O.synth_pair(H, W, D, 3), O.synth_pair(H, W, D, 4)
    inputs = dict(L0=L0.astype(np.float32), R0=R0.astype(np.float32), L1=L1.astype(np.float32), R1=R1.astype(np.float32))
    res = mirror(smt, tmp_path, "adcensus", (H, W, D), inputs)
    assert res.status == ["AD_Census ok"]
    for k, (L, R) in enumerate(((L0, R0), (L1, R1))):
        BC.bits_eq(res.out(f"left{k}", np.float32, (H, W, D)), O.adcensus_view(L, R, D, 10.0, 30.0, 0), f"left volume {k}")
        BC.bits_eq(res.out(f"right{k}", np.float32, (H, W, D)), O.adcensus_view(L, R, D, 10.0, 30.0, 1), f"right volume {k}")
    assert not np.array_equal(res.out("right0", np.float32, (H, W, D)), res.out("right1", np.float32, (H, W, D)))
    unchanged(res, inputs)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_ncc_flow_set_form(smt, O, tmp_path, form):
    """NCCFlow::set_form selects the cost kernel (smt_ncc_last_form) and every form gives the oracle's maps; runBoth's
    right view is the mirrored single view (include/smt.h: smt_lrncc), its cross-check the oracle's Sad.h:184-222"""
    H, W, D, win, P = 7, 37, 65, 2, 2
    imgs = [BC._padded(H, W, 0, 170 + 3 * b)[:2] for b in range(P)]
    Lb, Rb = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    res = mirror(smt, tmp_path, "ncc_form", (H, W, D, win, form, P), dict(L=Lb, R=Rb))
    assert res.status == [f"form {form}", "NCCFlow ok"]
    for b, (L, R) in enumerate(imgs):
        dl = O.ncc(L, R, D, win).astype(np.int32)
        dr = np.ascontiguousarray(O.ncc(R[:, ::-1].copy(), L[:, ::-1].copy(), D, win)[:, ::-1]).astype(np.int32)
        last, cls = O.sad_crosscheck(dl, dr)
        BC.bits_eq(res.out("disp", np.int32, (P, H, W))[b], dl, ("disp", b))
        BC.bits_eq(res.out("bothL", np.int32, (P, H, W))[b], dl, ("dispLeft", b))
        BC.bits_eq(res.out("bothR", np.int32, (P, H, W))[b], dr, ("dispRight", b))
        BC.bits_eq(res.out("last", np.int32, (P, H, W))[b], last.astype(np.int32), ("lastdisp", b))
        BC.bits_eq(res.out("cls", np.uint8, (P, H, W))[b], cls.astype(np.uint8), ("cls", b))
    unchanged(res, dict(L=Lb, R=Rb))


@pytest.mark.parametrize("form", [NW.LOOP, NW.INT])
def test_ncc_whole_flow_set_form(smt, O, tmp_path, form):
    H, W, k, Off, P = 5, 33, 1, 12, 3                      # a shape of ncc_whole_cases.FLOW_CASES
    imgs = NW.flow_pairs(H, W, P)
    Lb, Rb = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    res = mirror(smt, tmp_path, "whole_form", (H, W, k, Off, form, P), dict(L=Lb, R=Rb))
    assert res.status == [f"form {form}", "NCCWholeFlow ok"]
    for b, (L, R) in enumerate(imgs):
        ref = NW.flow_reference(BC.Ctx(O), L, R, k, Off, form)
        for nm in ("depthL", "depthR", "offL", "offR", "lastdisp"):
            BC.bits_eq(res.out(nm, ref[nm].dtype, (P, H, W))[b], ref[nm], (nm, b))
    unchanged(res, dict(L=Lb, R=Rb))


@pytest.mark.parametrize("H,W,D,ws,P", [(5, 65, 64, 1, 2), (3, 33, 65, 0, 1)])       # bounds_cases' smt_cblsm_flow_run_batch_window
def test_cblsm_flow_run_window(smt, O, tmp_path, H, W, D, ws, P):
    Ls = np.stack([VC.noisy_pair(H, W, 70 + b)[0] for b in range(P)])
    Rs = np.stack([VC.noisy_pair(H, W, 70 + b)[1] for b in range(P)])
    res = mirror(smt, tmp_path, "window_flow", (H, W, D, ws, P), dict(L=Ls, R=Rs))
    assert res.status == ["CBLSMFlow ok"]
    for b in range(P):
        _, _, dl, dr = CW.flow_oracle(O, Ls[b], Rs[b], D, ws)
        BC.bits_eq(res.out("dispL", np.float32, (P, H, W))[b], dl.astype(np.float32), ("dispLeft", b))
        BC.bits_eq(res.out("dispR", np.float32, (P, H, W))[b], dr.astype(np.float32), ("dispRight", b))
    unchanged(res, dict(L=Ls, R=Rs))
