"""BASELINE.json configs 2, 3 and 5 at FULL size: every volume and map of the HIP path (through the
C ABI) hashed on the host (D2H + the oracle's FNV-1a) and compared with tests/golden/config_hashes.json,
which the CPU oracle produced in the build container (tests/golden/make_config_hashes.py) on the same
SURVEY 8(d) synthetic pairs.  This is where the up/down scanline passes (ScanlineOptimizer.h:194-253, with
their three quirks), the ((left+right)+up)+down sum (:124), the right-view aggregation (stride-bug arms,
CrossArm.cpp:60-102, :265) and the LR check (PostProcessing.h:72-135) are compared at 1920x1080x192.

The fixtures pin the HIP path to the oracle at full size; the oracle is pinned to the reference's own compiled code
at small sizes (oracle/smt_oracle.c header, tests/test_ref_pin_cpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_hashes.json")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def gold():
    assert os.path.exists(GOLD), "tests/golden/config_hashes.json missing (tests/golden/make_config_hashes.py)"
    return json.load(open(GOLD))


def hx(O, t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return "%016x" % O.fnv1a(a)


def check(O, rec, key, t):
    got = hx(O, t)
    assert got == rec[key], f"{key}: device {got} != oracle fixture {rec[key]}"


def test_config2_full_size_hashes(smt, O, gold):
    from stereo_match_traditional_amd import synth
    rec = gold["cfg2_adcensus_720p_d128"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    L, R = synth.synth_pair(H, W, D, rec["seed"])
    adc = smt.AD_Census().Initialize(T(L.astype(np.float32)), T(R.astype(np.float32)), D, H, W, rec["sigmaC"],
                                     rec["sigmaS"])
    dl = torch.empty((H, W), device=DEV)
    dr = torch.empty((H, W), device=DEV)
    adc.ComputeBoth(dl, dr)
    adc.status()
    check(O, rec, "adcensus_vol_left", adc.GetPtrLeft())
    check(O, rec, "adcensus_vol_right", adc.GetPtrRight())
    check(O, rec, "adcensus_disp_left", dl)
    check(O, rec, "adcensus_disp_right", dr)
    adc.close()


def test_config3_full_size_hashes(smt, O, gold):
    """The north-star pipeline in main.cpp's order (AD-CensusV1/main.cpp:59-92), every stage's output."""
    from stereo_match_traditional_amd import synth
    rec = gold["cfg3_pipeline_1080p_d192"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    L, R = synth.synth_pair(H, W, D, rec["seed"])
    Lf, Rf = T(L.astype(np.float32)), T(R.astype(np.float32))
    adc = smt.AD_Census().Initialize(Lf, Rf, D, H, W, rec["sigmaC"], rec["sigmaS"])
    dl = torch.empty((H, W), device=DEV)
    dr = torch.empty((H, W), device=DEV)
    adc.ComputeBoth(dl, dr)
    adc.status()
    check(O, rec, "adcensus_vol_left", adc.GetPtrLeft())
    check(O, rec, "adcensus_vol_right", adc.GetPtrRight())
    check(O, rec, "adcensus_disp_left", dl)
    check(O, rec, "adcensus_disp_right", dr)

    agg = {}
    disp = {}
    for view, img, vol in (("left", L, adc.GetPtrLeft()), ("right", R, adc.GetPtrRight())):
        ca = smt.CrossArmAggregation().Initialize(H, W, rec["tau"], D, DEV)
        ca.ComputeArmLengths(T(img))
        for nm, a in zip(("left", "right", "top", "bottom"), ca.arm_maps()):
            check(O, rec, f"arms_{view}img_{nm}", a)
        agg[view] = torch.empty((H, W, D), device=DEV)
        disp[view] = torch.empty((H, W), device=DEV)
        ca.AggregationVertical(vol, agg[view], disp[view])
        ca.status()
        check(O, rec, f"agg_vol_{view}", agg[view])
        check(O, rec, f"agg_disp_{view}", disp[view])
        ca.close()
    del agg["right"]
    adc.close()

    so = smt.ScanlineOptimizer().Initialize(H, W, D, rec["p1"], rec["p2"], DEV)
    for which in ("left", "right", "up", "down"):
        pv = so.ScanPass(agg["left"], Lf, which)
        check(O, rec, "scan_path_" + which, pv)
        del pv
    out = torch.empty((H, W, D), device=DEV)
    dso = torch.empty((H, W), device=DEV)
    so.ScanLine(agg["left"], Lf, out, dso)
    check(O, rec, "scan_sum", out)
    check(O, rec, "scan_disp", dso)
    so.close()

    cls, nocc, nmis = smt.LeftRightConsistency(W, H, rec["gate"], dso, disp["right"])
    check(O, rec, "lr_disp", dso)
    check(O, rec, "lr_cls", cls)
    assert (nocc, nmis) == (rec["lr_n_occlusion"], rec["lr_n_mismatch"])


def test_config5_batch_hashes(smt, O, gold):
    """configs[4]: the whole 256-pair KITTI-size batch through smt_adcensus_compute_batch; every pair's
    two WTA maps against the oracle's, plus the last pair's volumes (the handle keeps only those)."""
    from stereo_match_traditional_amd import synth
    rec = gold["cfg5_kitti_d256_batch"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    P = len(rec["pairs"])
    assert P >= 1
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, rec["seed0"] + b) for b in range(P)])
    Lb = T(np.stack(Ls).astype(np.float32))
    Rb = T(np.stack(Rs).astype(np.float32))
    dl = torch.empty((P, H, W), device=DEV)
    dr = torch.empty((P, H, W), device=DEV)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, rec["sigmaC"], rec["sigmaS"])
    adc.ComputeBatch(Lb, Rb, dl, dr)
    adc.status()
    dlh, drh = dl.cpu().numpy(), dr.cpu().numpy()
    for b in range(P):
        r = rec["pairs"][str(b)]
        assert hx(O, dlh[b]) == r["adcensus_disp_left"], b
        assert hx(O, drh[b]) == r["adcensus_disp_right"], b
    last = rec["pairs"][str(P - 1)]
    check(O, last, "adcensus_vol_left", adc.GetPtrLeft())
    check(O, last, "adcensus_vol_right", adc.GetPtrRight())
    adc.close()


def test_config3_through_the_batched_pipeline_entry(smt, O, gold):
    """smt_pipeline_run_batch (the sharding unit of config 3): a batch of 2 x the config-3 pair -- both pairs'
    maps, class maps and counts and the last pair's five volumes against the oracle fixtures."""
    from stereo_match_traditional_amd import synth
    rec = gold["cfg3_pipeline_1080p_d192"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    L, R = synth.synth_pair(H, W, D, rec["seed"])
    Lb = T(np.stack([L, L]))
    Rb = T(np.stack([R, R]))
    pipe = smt.Pipeline(H, W, D, DEV)
    dl, dr, cls, counts = pipe.run(Lb, Rb)
    pipe.status()
    for b in range(2):
        check(O, rec, "lr_disp", dl[b])
        check(O, rec, "agg_disp_right", dr[b])
        check(O, rec, "lr_cls", cls[b])
        assert tuple(counts[b].cpu().tolist()) == (rec["lr_n_occlusion"], rec["lr_n_mismatch"])
    for key, v in zip(("adcensus_vol_left", "adcensus_vol_right", "agg_vol_left", "agg_vol_right", "scan_sum"), pipe.volumes()):
        check(O, rec, key, v)
    pipe.close()


@pytest.mark.parametrize("schedule", ["default", "0", "1", "2"])
def test_pipeline_batch_small_pairs_vs_oracle(smt, O, schedule, monkeypatch):
    """Different pairs in one batch, every map against the oracle pipeline run pair by pair -- under each stream
    schedule of smt_pipeline_run_batch (SMT_PIPE_SCHEDULE, read at create: 0 one stream, 1 right view beside the
    scanline, 2 three streams with double-buffered front-end state; 5 pairs so that every event edge of 2 is used)."""
    if schedule != "default":
        monkeypatch.setenv("SMT_PIPE_SCHEDULE", schedule)
    H, W, D, P = 40, 96, 32, 5
    pairs = [O.synth_pair(H, W, D, 20 + b, b == 1) for b in range(P)]
    Lb = T(np.stack([p[0] for p in pairs]))
    Rb = T(np.stack([p[1] for p in pairs]))
    pipe = smt.Pipeline(H, W, D, DEV)
    dl, dr, cls, counts = pipe.run(Lb, Rb)
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
    try:
        pipe.status()
    except SmtError as e:
        # small images + stride bug: out-of-plane taps are flagged (the reference is undefined there), results defined.
        # Nothing else may hide here: a HIP error or a domain error fails the test.
        assert e.status == SMT_ERR_REF_UB, e
    for b, (L, R) in enumerate(pairs):
        cl = O.adcensus_view(L, R, D, 10.0, 30.0, 0)
        cr = O.adcensus_view(L, R, D, 10.0, 30.0, 1)
        al, _ = O.aggregate_rect(cl, O.arms_all(L), 0)
        ar, _ = O.aggregate_rect(cr, O.arms_all(R), 0)
        d_so, d_r = O.wta(O.scanline(al, L.astype(np.float32), 10, 150)), O.wta(ar)
        lr, c, no, nm = O.lrcheck(d_so, d_r, 2)
        assert np.array_equal(dl[b].cpu().numpy().view(np.uint32), lr.view(np.uint32)), b
        assert np.array_equal(dr[b].cpu().numpy(), d_r) and np.array_equal(cls[b].cpu().numpy(), c)
        assert tuple(counts[b].cpu().tolist()) == (no, nm)
    pipe.close()


def test_a18_crossaggregator_full_size_vs_reference_build(smt, O, gold):
    """CrossAggregator at 1280x720 D=128, ADCensusOption's parameters, 4 iterations, fed with config 2's left AD-Census
    volume computed on the device: arms, aggregated volume and WTA map against hashes produced by the REFERENCE's own
    cross_aggregator.cpp (oracle/_ref, tests/golden/make_config_hashes.py a18) -- the pinned stage at its benchmark size.
    Both HIP formulations (shared-tap passes, one pixel per wave)."""
    from stereo_match_traditional_amd import synth
    rec = gold["a18_crossaggregator_720p_d128"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    L, R = synth.synth_pair(H, W, D, rec["seed"])
    bgr = np.clip(L.astype(np.int32)[..., None] + (synth.lcg_bytes(rec["bgr_seed"], H * W * 3)[0] % 3).reshape(H, W, 3), 0, 255).astype(np.uint8)
    adc = smt.AD_Census().Initialize(T(L.astype(np.float32)), T(R.astype(np.float32)), D, H, W, 10.0, 30.0)
    adc.ComputeBoth()
    cost = adc.GetPtrLeft().clone()
    adc.close()
    assert hx(O, cost) == rec["cost_init_hash"]
    b = T(bgr)
    for impl in (2, 1):
        ca = smt.CrossAggregator()
        ca.Initialize(W, H, 0, D, DEV)
        ca.set_impl(impl)
        ca.SetData(b, b, cost)
        ca.SetParams(rec["L1"], rec["L2"], rec["t1"], rec["t2"])
        ca.Aggregate(rec["iters"])
        check(O, rec, "arms", ca.get_arms_ptr())
        out = ca.get_cost_ptr()
        check(O, rec, "cost", out)
        check(O, rec, "disp", smt.wta(out))
        ca.close()


@pytest.mark.parametrize("D", [320, 257, 512])
def test_disparity_range_above_256(smt, O, D):
    """AD_Census::Initialize takes any `int dispRange` (AD-Census.h:322); the C ABI covers D <= SMT_MAX_DISPARITY = 512
    on rows a1-a15 (beyond 256 a lane owns 5..8 hypotheses and the first-version kernels run).  AD-Census volumes + WTA,
    arms + both aggregation orders + fused WTA, the four scanline passes + sum + WTA, the LR check and the batched
    pipeline entry against the oracle, bit for bit, on a pair wider than D and on one narrower."""
    for H, W, seed in ((12, D + 37, 5), (9, 150, 6)):
        L, R = O.synth_pair(H, W, min(D, 64), seed)
        Lf, Rf = T(L.astype(np.float32)), T(R.astype(np.float32))
        adc = smt.AD_Census().Initialize(Lf, Rf, D, H, W, 10.0, 30.0)
        dl, dr = torch.empty((H, W), device=DEV), torch.empty((H, W), device=DEV)
        adc.ComputeBoth(dl, dr)
        adc.status()
        cl, cr = O.adcensus_view(L, R, D, 10.0, 30.0, 0), O.adcensus_view(L, R, D, 10.0, 30.0, 1)
        assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), cl.view(np.uint32))
        assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), cr.view(np.uint32))
        assert np.array_equal(dl.cpu().numpy(), O.wta(cl)) and np.array_equal(dr.cpu().numpy(), O.wta(cr))
        assert np.array_equal(smt.wta(adc.GetPtrLeft()).cpu().numpy(), O.wta(cl))
        ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, DEV)
        ca.ComputeArmLengths(T(L))
        arms = O.arms_all(L)
        agg = torch.empty((H, W, D), device=DEV)
        for order, fn in ((0, ca.AggregationVertical), (1, ca.costAggregationV5)):
            fn(adc.GetPtrLeft(), agg, dl)
            ref, _ = O.aggregate_rect(cl, arms, order)
            assert np.array_equal(agg.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (D, order)
            assert np.array_equal(dl.cpu().numpy(), O.wta(ref))
        ca.AggregationVertical(adc.GetPtrLeft(), agg)
        al, _ = O.aggregate_rect(cl, arms, 0)
        so = smt.ScanlineOptimizer().Initialize(H, W, D, 10, 150, DEV)
        out = torch.empty((H, W, D), device=DEV)
        so.ScanLine(agg, Lf, out, dl)
        ref = O.scanline(al, L.astype(np.float32), 10, 150)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), D
        assert np.array_equal(dl.cpu().numpy(), O.wta(ref))
        for o in (adc, ca, so):
            o.close()
        pipe = smt.Pipeline(H, W, D, DEV)
        pdl, pdr, cls, counts = pipe.run(T(L), T(R))
        from stereo_match_traditional_amd import SmtError
        from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
        try:
            pipe.status()
        except SmtError as e:
            assert e.status == SMT_ERR_REF_UB, e
        ar, _ = O.aggregate_rect(cr, O.arms_all(R), 0)
        lr, c, no, nm = O.lrcheck(O.wta(ref), O.wta(ar), 2)
        assert np.array_equal(pdl[0].cpu().numpy().view(np.uint32), lr.view(np.uint32))
        assert np.array_equal(pdr[0].cpu().numpy(), O.wta(ar)) and np.array_equal(cls[0].cpu().numpy(), c)
        pipe.close()
    # and one past the limit is refused
    with pytest.raises(SmtError):
        smt.AD_Census().Initialize(Lf, Rf, 513, H, W, 10.0, 30.0)
