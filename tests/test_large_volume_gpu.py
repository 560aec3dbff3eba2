"""Every volume stage at 4 GiB to 8 GiB against the oracle, through periodic inputs (large_volume_cases.py holds the method,
the table and the helpers; test_large_volume_cpu.py proves the method on the oracle alone).  Three regimes: A, the largest
volume under 2^32 bytes (the tuned aggregation kernels with the top bit of their 32-bit tap offsets set); B, the smallest
at 2^32 bytes (the plain walk, whatever variant was asked for); C, just above 2^31 elements (element indices past int,
byte offsets past 2^32).  Every output is prefilled with 0xFF bytes; every element is compared on the device, the first,
second and last block with the oracle bit for bit (NCC costs by the bounds of exact_matchers.py).

A case frees its tensors and closes its handle before the next one.  It skips only when the device reports less free memory
than the table's figure plus 2 GiB; the last test prints every case as run or skipped, with its wall time."""
import ctypes as C
import functools
import gc
import time

import numpy as np
import pytest
import torch

import exact_matchers as X
import large_volume_cases as LV

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RESULTS = {}                    # case id -> "run <seconds>" / "skipped: ..." / "FAILED"
_O = None


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tile_dev(block, *reps):
    """the block repeated on the device: the full-size input never exists on the host"""
    return T(block).repeat(*reps)


def out_like(shape, dtype=torch.float32):
    return LV.prefilled(shape, dtype, DEV)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def call(status, what):
    from stereo_match_traditional_amd._lib import check
    check(status, what)


def L():
    from stereo_match_traditional_amd._lib import lib
    return lib()


@pytest.fixture(autouse=True)
def _oracle(O):
    global _O
    _O = O


# ------------------------------------------------------------------------------------------- inputs and oracle results, once
@functools.lru_cache(maxsize=None)
def agg_inputs(D):
    return LV.cost_block((LV.H0, LV.W, D), 100 + D), tuple(LV.arm_block(LV.H0, LV.W, 101))


@functools.lru_cache(maxsize=None)
def agg_expected(D, order):
    vb, ab = agg_inputs(D)
    return LV.aggregate_expected(_O, vb, list(ab), order)


@functools.lru_cache(maxsize=None)
def adc_images(seed):
    return LV.image_block(LV.H0, LV.W, seed), LV.image_block(LV.H0, LV.W, seed + 1)


@functools.lru_cache(maxsize=None)
def adc_expected(seed, K, D, view):
    vols = LV.adcensus_expected(_O, *adc_images(seed), K, D, view)
    return vols, tuple(_O.wta(v) for v in vols)


@functools.lru_cache(maxsize=None)
def scan_strip(H, D, fixed):
    strip = LV.cost_block((H, LV.W0, D), 400)
    gstrip = LV.column_guide(H, LV.W0, 401) if fixed else LV.flat_guide(H, LV.W0, LV.W0, 402)
    return strip, gstrip


@functools.lru_cache(maxsize=None)
def ncc_images():
    return LV.image_block(LV.H0, LV.W, 500), LV.image_block(LV.H0, LV.W, 501)


@functools.lru_cache(maxsize=None)
def ncc_expected(D, win):
    Lb, Rb = ncc_images()
    return X.ncc_exact(LV.tile_rows(Lb, 3), LV.tile_rows(Rb, 3), D, win)


# --------------------------------------------------------------------------------------------------------------- the stages
def run_agg(smt, c):
    K, order, variant = c.H // c.h0, c.params["order"], c.params["variant"]
    vb, ab = agg_inputs(c.D)
    vols, maps = agg_expected(c.D, order)
    vin = tile_dev(vb, K, 1, 1)
    arms = [T(a) for a in LV.full_arms(list(ab), K)]
    vout, disp = out_like((c.H, c.W, c.D)), out_like((c.H, c.W))
    ca = smt.CrossArmAggregation().Initialize(c.H, c.W, 30, c.D, DEV)
    try:
        ca.load_arm_maps(*arms)
        if variant is not None:
            ca.set_variant(variant)
        ca._agg(vin, vout, order, disp)
        ca.status()                                          # no rectangle leaves the plane: no SMT_ERR_REF_UB
    finally:
        ca.close()
    LV.check_rows(vout, c.h0, *vols, c.id + " volume")
    LV.check_rows(disp, c.h0, *maps, c.id + " map")
    assert not LV.differing_blocks(vin, c.h0, first=0, last=K - 1), "the input volume changed"


def run_adc(smt, c):
    K, mode = c.H // c.h0, c.params["mode"]
    seeds = (310,) if mode == "compute" else (330, 310)      # the last pair of a batch is the single call's pair
    Ls = [T(LV.tile_rows(adc_images(s)[0], K).astype(np.float32)) for s in seeds]
    Rs = [T(LV.tile_rows(adc_images(s)[1], K).astype(np.float32)) for s in seeds]
    adc = smt.AD_Census().Initialize(Ls[-1], Rs[-1], c.D, c.H, c.W, LV.SIGMA_C, LV.SIGMA_S, placement_search=False,
                                     store_calibration=False)
    try:
        if mode != "deferred":                               # lent beforehand: the call itself writes the volumes
            vl, vr = adc.GetPtrLeft(), adc.GetPtrRight()
            LV.bits(vl).fill_(-1)
            LV.bits(vr).fill_(-1)
        if mode == "compute":
            dl, dr = out_like((1, c.H, c.W)), out_like((1, c.H, c.W))
            adc.ComputeBoth(dl[0], dr[0])
        else:
            dl, dr = out_like((2, c.H, c.W)), out_like((2, c.H, c.W))
            adc.ComputeBatch(torch.stack(Ls), torch.stack(Rs), dl, dr)
        adc.status()
        if mode == "deferred":                               # smt_adcensus_volume writes the last pair's volumes now
            vl, vr = adc.GetPtrLeft(), adc.GetPtrRight()
        torch.cuda.synchronize()
        for view, vol, d in ((0, vl, dl), (1, vr, dr)):
            LV.check_rows(vol, c.h0, *adc_expected(seeds[-1], K, c.D, view)[0], f"{c.id} volume of view {view}")
            for p, s in enumerate(seeds):
                LV.check_rows(d[p], c.h0, *adc_expected(s, K, c.D, view)[1], f"{c.id} map of view {view}, pair {p}")
        del vl, vr
    finally:
        adc.close()


def run_wta(smt, c):
    K = c.H // c.h0
    vb = LV.cost_block((c.h0, c.W, c.D), 200 + c.D, levels=64)           # a tie in most pixels
    want = _O.wta(vb)
    assert (np.sort(vb, -1)[..., 0] == np.sort(vb, -1)[..., 1]).mean() > 0.5
    assert torch.equal(LV.first_min(T(vb)), T(want)), "the torch first minimum is not the oracle's"
    vol = tile_dev(vb, K, 1, 1)
    disp = out_like((c.H, c.W))
    smt.wta(vol, disp)
    LV.check_rows(disp, c.h0, want, want, want, c.id)
    LV.check_pieces(disp, c.h0, lambda r0, r1: LV.first_min(vol[r0:r1]), c.id + " against the torch first minimum",
                    row_bytes=c.W * c.D * 4)


def _scan_handle(smt, c, quirks=0):
    so = smt.ScanlineOptimizer().Initialize(c.H, c.W, c.D, LV.P1, LV.P2, DEV, quirks=quirks)
    call(L().smt_scanline_set_stream(so._h, stream()), "smt_scanline_set_stream")
    return so


def run_scan_rows(smt, c):
    K, p = c.H // c.h0, c.params["scan_pass"]
    cb = LV.cost_block((c.h0, c.W, c.D), 300)
    gb = LV.image_block(c.h0, c.W, 301).astype(np.float32)
    want = LV.scan_rows_expected(_O, cb, gb, ("left", "right")[p])
    cost, gray = tile_dev(cb, K, 1, 1), tile_dev(gb, K, 1)
    out = out_like((c.H, c.W, c.D))
    so = _scan_handle(smt, c)
    try:
        call(L().smt_scanline_pass(so._h, ptr(cost), ptr(gray), p, ptr(out)), "smt_scanline_pass")
        torch.cuda.synchronize()
    finally:
        so.close()
    LV.check_rows(out, c.h0, want, want, want, c.id)


def run_scan_cols(smt, c):
    from stereo_match_traditional_amd._lib import QUIRK_FIX_SCAN_VERTICAL
    kc, p, fixed = c.W // c.w0, c.params["scan_pass"], c.params["fixed"]
    strip, gstrip = scan_strip(c.H, c.D, fixed)
    want = LV.scan_cols_expected(_O, strip, gstrip, ("up", "down")[p - 2], fixed)
    cost, gray = tile_dev(strip, 1, kc, 1), tile_dev(gstrip, 1, kc)
    out = out_like((c.H, c.W, c.D))
    so = _scan_handle(smt, c, QUIRK_FIX_SCAN_VERTICAL if fixed else 0)
    try:
        call(L().smt_scanline_pass(so._h, ptr(cost), ptr(gray), p, ptr(out)), "smt_scanline_pass")
        torch.cuda.synchronize()
    finally:
        so.close()
    LV.check_cols(out, c.w0, want, c.id)


def run_scan_run(smt, c):
    K, kc = c.H // c.h0, c.W // c.w0
    cb = LV.cost_block((c.h0, c.w0, c.D), 410)
    guide = LV.flat_guide(c.H, c.W, c.w0, 411)
    l, r, u, d = [T(a) for a in LV.scan_run_parts(_O, cb, guide[0], c.H, c.W)]
    lr = l + r
    del l, r
    cost, gray = tile_dev(cb, K, kc, 1), T(guide)
    out, disp = out_like((c.H, c.W, c.D)), out_like((c.H, c.W))
    so = _scan_handle(smt, c)
    try:
        call(L().smt_scanline_run(so._h, ptr(cost), ptr(gray), ptr(out), ptr(disp)), "smt_scanline_run")
        torch.cuda.synchronize()
    finally:
        so.close()                                           # frees the handle's scratch volume
    del cost
    LV.check_pieces(out, c.h0, lambda r0, r1: LV.compose_scan_run(lr, u, d, r0, r1, kc), c.id + " volume")
    LV.check_pieces(disp, c.h0, lambda r0, r1: LV.first_min(out[r0:r1]), c.id + " map", row_bytes=c.W * c.D * 4)


def run_cblsm_ad(smt, c):
    K, view = c.H // c.h0, c.params["view"]
    Lb, Rb = LV.image_block(c.h0, c.W, 600), LV.image_block(c.h0, c.W, 601)
    want = LV.split3(_O.cblsm_ad(LV.tile_rows(Lb, 3), LV.tile_rows(Rb, 3), c.D, view), c.h0)
    out = out_like((c.H, c.W, c.D))
    smt.cblsm_ComputeAD(tile_dev(Lb, K, 1), tile_dev(Rb, K, 1), c.D, (smt.VIEW_LEFT, smt.VIEW_RIGHT)[view], out)
    LV.check_rows(out, c.h0, *want, c.id)


def run_ncc(smt, c):
    K, impl, win = c.H // c.h0, c.params["impl"], c.params["win"]
    Lb, Rb = ncc_images()
    exact, flat, sentinel = ncc_expected(c.D, win)
    Lt, Rt = tile_dev(Lb, K, 1), tile_dev(Rb, K, 1)
    cost, disp = out_like((c.H, c.W, c.D), torch.float64), out_like((c.H, c.W), torch.int32)
    smt.ncc_set_impl(impl)
    try:
        call(L().smt_ncc(ptr(Lt), ptr(Rt), c.H, c.W, c.D, win, ptr(disp), ptr(cost), stream()), "smt_ncc")
        torch.cuda.synchronize()
        assert smt.ncc_last_form() == impl                   # NCC_FORM_DOT4 = 2, NCC_FORM_BOX = 3: no loop-nest fallback
    finally:
        smt.ncc_set_impl(2)
    # blocks bit-identical among themselves; the first, second and last by the project's own bound; maps = WinTakeAll of
    # the call's own costs
    assert not LV.differing_blocks(cost, c.h0), "cost blocks differ"
    assert not LV.differing_blocks(disp, c.h0), "map blocks differ"
    three = lambda t: torch.cat([t[:c.h0], t[c.h0:2 * c.h0], t[-c.h0:]]).cpu().numpy()      # noqa: E731
    got = three(cost)
    worst = X.check_ncc(got, exact, flat, sentinel, win, "int")
    print(f"{c.id}: largest |cost - exact| = {worst:.3g} x bound (2^-50 |exact|)")
    assert np.array_equal(three(disp), X.ncc_wta(got, win))


def run_sad(smt, c):
    K, ws = c.H // c.h0, c.params["winsize"]
    Lb, Rb = LV.image_block(c.h0, c.W, 700), LV.image_block(c.h0, c.W, 701)
    Lp3, Rp3 = [_O.pad_replicate(LV.tile_rows(b, 3), ws + 1) for b in (Lb, Rb)]
    vol3 = LV.left_costs_fn()(Lp3, Rp3, c.D, ws)
    assert int(vol3.max()) < 1 << 24                         # integers a float32 holds exactly
    want_l, want_r = _O.sad(Lp3, Rp3, c.D, ws, 0), _O.sad(Lp3, Rp3, c.D, ws, 1)
    Lp, Rp = [T(_O.pad_replicate(LV.tile_rows(b, K), ws + 1)) for b in (Lb, Rb)]
    dl, dr = out_like((c.H, c.W), torch.int32), out_like((c.H, c.W), torch.int32)
    cl = out_like((c.H, c.W, c.D))
    call(L().smt_sad_both(ptr(Lp), ptr(Rp), c.H, c.W, c.D, ws, ptr(dl), ptr(dr), ptr(cl), stream()), "smt_sad_both")
    torch.cuda.synchronize()
    LV.check_rows(cl, c.h0, *LV.split3(vol3.astype(np.float32), c.h0), c.id + " costL")
    LV.check_rows(dl, c.h0, *LV.split3(want_l, c.h0), c.id + " left map")
    LV.check_rows(dr, c.h0, *LV.split3(want_r, c.h0), c.id + " right map")


RUN = dict(agg=run_agg, adc=run_adc, wta=run_wta, scan_rows=run_scan_rows, scan_cols=run_scan_cols, scan_run=run_scan_run,
           cblsm_ad=run_cblsm_ad, ncc=run_ncc, sad=run_sad)


@pytest.mark.parametrize("c", LV.CASES, ids=[c.id for c in LV.CASES])
def test_large_volume(smt, c):
    gc.collect()
    torch.cuda.empty_cache()
    need = LV.device_bytes(c)
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < need + LV.HEADROOM:
        msg = (f"{c.id} needs {need} bytes ({need / LV.GiB:.2f} GiB) plus {LV.HEADROOM} of headroom; "
               f"the device reports {free} bytes free ({free / LV.GiB:.2f} GiB)")
        RESULTS[c.id] = "skipped: " + msg
        pytest.skip(msg)
    RESULTS[c.id] = "FAILED"
    t0 = time.perf_counter()
    try:
        RUN[c.stage](smt, c)
        torch.cuda.synchronize()
    finally:
        gc.collect()
        torch.cuda.empty_cache()
    RESULTS[c.id] = f"run {time.perf_counter() - t0:6.2f} s   {LV.elements(c) * c.itemsize / LV.GiB:.4f} GiB per volume"


def test_summary_lists_every_case_as_run_or_skipped(capsys):
    with capsys.disabled():
        print()
        for c in LV.CASES:
            print(f"  large volume  {c.id:28s} {RESULTS.get(c.id, 'not selected')}")
    assert all(r.startswith(("run", "skipped: ")) for r in RESULTS.values()), [k for k, r in RESULTS.items() if r == "FAILED"]
