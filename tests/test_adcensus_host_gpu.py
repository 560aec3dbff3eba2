"""Host-fed AD-Census batches (ADCensusHostBatch / smt_adcensus_host_*): uint8 images in host memory in, both views'
maps in host memory out.  The maps must equal smt_adcensus_compute_batch's on the same pairs staged by hand, bit for
bit, for every chunking, map format and input format, across reuse of the handle's slots; and the oracle's at the edge
shapes of the staging and packing kernels."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_hashes.json")
SC, SS = 10.0, 30.0


def pairs_u8(H, W, D, P, seed0):
    from stereo_match_traditional_amd import synth
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, seed0 + 7 * b) for b in range(P)])
    return np.stack(Ls), np.stack(Rs)


def device_batch(smt, L, R, D):
    """smt_adcensus_compute_batch on the pairs staged by hand (uint8 -> float32 on the host)."""
    P, H, W = L.shape
    Lf = torch.from_numpy(L.astype(np.float32)).to(DEV)
    Rf = torch.from_numpy(R.astype(np.float32)).to(DEV)
    dl = torch.empty((P, H, W), device=DEV)
    dr = torch.empty((P, H, W), device=DEV)
    adc = smt.AD_Census().Initialize(Lf[0], Rf[0], D, H, W, SC, SS, placement_search=False, store_calibration=False)
    adc.ComputeBatch(Lf, Rf, dl, dr)
    adc.status()
    adc.close()
    return dl.cpu().numpy(), dr.cpu().numpy()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SHAPES = [(24, 130, 64), (33, 97, 128), (18, 100, 192), (9, 70, 256), (12, 90, 320)]


@pytest.mark.parametrize("H,W,D", SHAPES)
def test_equal_to_the_device_batch(smt, O, H, W, D):
    L, R = pairs_u8(H, W, D, 13, 100 + D)
    for P in (1, 5, 13):
        refl, refr = device_batch(smt, L[:P], R[:P], D)
        for chunk in (1, 4, 8):
            hb = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=chunk)
            dl, dr = hb.run(torch.from_numpy(L[:P].copy()).pin_memory(), torch.from_numpy(R[:P].copy()).pin_memory())
            assert same(dl.numpy(), refl) and same(dr.numpy(), refr), (P, chunk)
            hb.close()
    if (H, W, D) == SHAPES[0]:
        hb = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=4)
        dl, dr = hb.run(torch.from_numpy(L), torch.from_numpy(R))
        for b in range(L.shape[0]):
            assert np.array_equal(dl[b].numpy(), O.wta(O.adcensus_view(L[b], R[b], D, SC, SS, 0))), b
            assert np.array_equal(dr[b].numpy(), O.wta(O.adcensus_view(L[b], R[b], D, SC, SS, 1))), b
        hb.close()


@pytest.mark.parametrize("H,W,D", SHAPES[:4])
def test_u8_maps_are_the_f32_maps_cast(smt, H, W, D):
    L, R = pairs_u8(H, W, D, 9, 300 + D)
    Lt, Rt = torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory()
    f = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=4)
    u = smt.ADCensusHostBatch(H, W, D, SC, SS, out_dtype=torch.uint8, chunk=4)
    fl, fr = f.run(Lt, Rt)
    ul, ur = u.run(Lt, Rt)
    assert ul.dtype == torch.uint8
    assert np.array_equal(ul.numpy(), fl.numpy().astype(np.uint8)) and np.array_equal(fl.numpy(), ul.numpy().astype(np.float32))
    assert np.array_equal(ur.numpy(), fr.numpy().astype(np.uint8)) and np.array_equal(fr.numpy(), ur.numpy().astype(np.float32))
    f.close()
    u.close()


def test_u8_maps_need_d_at_most_256(smt):
    from stereo_match_traditional_amd._lib import SmtError, SMT_ERR_ARG
    with pytest.raises(SmtError) as e:
        smt.ADCensusHostBatch(12, 90, 320, out_dtype=torch.uint8)
    assert e.value.status == SMT_ERR_ARG


@pytest.mark.parametrize("H,W,D", [(24, 130, 64), (33, 97, 128)])
def test_bgr_input(smt, H, W, D):
    """channels=3 equals gray input made by smt_bgr2gray on the device and by the numpy restatement of its rule."""
    P = 6
    rng = np.random.default_rng(D)
    Lb = rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)
    Rb = Lb.copy()
    Rb[:, :, : W - 5] = Lb[:, :, 5:]                      # a shifted view, so the maps are not noise alone
    Rb[:, :, W - 5:] = rng.integers(0, 256, (P, H, 5, 3), dtype=np.uint8)

    def np_gray(x):
        x = x.astype(np.int64)
        return ((1868 * x[..., 0] + 9617 * x[..., 1] + 4899 * x[..., 2] + (1 << 13)) >> 14).astype(np.uint8)

    dev_gray = lambda x: np.stack([smt.cvtColor_BGR2GRAY(torch.from_numpy(x[b]).to(DEV)).cpu().numpy() for b in range(P)])
    Lg, Rg = dev_gray(Lb), dev_gray(Rb)
    assert np.array_equal(Lg, np_gray(Lb)) and np.array_equal(Rg, np_gray(Rb))
    c = smt.ADCensusHostBatch(H, W, D, SC, SS, channels=3, chunk=4)
    g = smt.ADCensusHostBatch(H, W, D, SC, SS, channels=1, chunk=4)
    cl, cr = c.run(torch.from_numpy(Lb).pin_memory(), torch.from_numpy(Rb).pin_memory())
    gl, gr = g.run(torch.from_numpy(Lg).pin_memory(), torch.from_numpy(Rg).pin_memory())
    assert same(cl.numpy(), gl.numpy()) and same(cr.numpy(), gr.numpy())
    refl, refr = device_batch(smt, np_gray(Lb), np_gray(Rb), D)
    assert same(cl.numpy(), refl) and same(cr.numpy(), refr)
    assert c.stats()["h2d_bytes"] == 2 * P * H * W * 3
    c.close()
    g.close()


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32])
def test_config5_full_size_hashes(smt, O, out_dtype):
    """All 256 KITTI-size pairs of config 5, gray pinned in: every map, as float32, hashes to the oracle's fixture."""
    from stereo_match_traditional_amd import synth
    rec = json.load(open(GOLD))["cfg5_kitti_d256_batch"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    P = len(rec["pairs"])
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, rec["seed0"] + b) for b in range(P)])
    L, R = torch.from_numpy(np.stack(Ls)).pin_memory(), torch.from_numpy(np.stack(Rs)).pin_memory()
    hb = smt.ADCensusHostBatch(H, W, D, rec["sigmaC"], rec["sigmaS"], out_dtype=out_dtype)
    dl, dr = hb.run(L, R)
    st = hb.stats()
    assert st["pinned_in"] == 1 and st["pinned_out"] == 1
    dl, dr = dl.numpy().astype(np.float32), dr.numpy().astype(np.float32)
    for b in range(P):
        r = rec["pairs"][str(b)]
        assert "%016x" % O.fnv1a(dl[b]) == r["adcensus_disp_left"], b
        assert "%016x" % O.fnv1a(dr[b]) == r["adcensus_disp_right"], b
    hb.close()


# A chunk of c pairs is one flat array of n = 2 * c * H * W pixels for k_stage_pairs and k_pack_maps, whose 16-pixel
# vector body leaves n % 16 pixels to a one-by-one tail.  Across their chunks these shapes give every residue n can have
# (n is even), n < 16 (tail only), W = 1, H = 1 and a partial last chunk (chunk does not divide P).
EDGES = [  # H, W, D, P, chunk            n of the full / the last chunk (n % 16)
    (1, 1, 1, 1, 1),                    # 2 (2)
    (1, 3, 63, 7, 3),                   # 18 (2), 6 (6)
    (5, 1, 255, 4, 3),                  # 30 (14), 10 (10)
    (1, 77, 256, 7, 2),                 # 308 (4), 154 (10)
    (3, 6, 320, 7, 3),                  # 108 (12), 36 (4)
    (9, 31, 255, 1, 2),                 # 558 (14)
    (8, 33, 256, 4, 3),                 # 1584 (0), 528 (0)
    (4, 65, 63, 4, 1),                  # 520 (8)
]


@pytest.mark.parametrize("H,W,D,P,chunk", EDGES)
def test_edges_against_the_oracle(smt, O, H, W, D, P, chunk):
    """Gray and BGR input, float32 and uint8 maps: every map equals the oracle's (BGR through O.bgr2gray, uint8 maps
    the oracle's cast).  The BGR images are low-contrast, so a gray value off by one moves census bits."""
    rng = np.random.default_rng(H * 1000 + W * 10 + P)
    for channels in (1, 3):
        if channels == 1:
            L, R = pairs_u8(H, W, D, P, 500 + D)
            gL, gR = L, R
        else:
            L = rng.integers(96, 112, (P, H, W, 3), dtype=np.uint8)
            R = rng.integers(96, 112, (P, H, W, 3), dtype=np.uint8)
            gL, gR = np.stack([O.bgr2gray(x) for x in L]), np.stack([O.bgr2gray(x) for x in R])
        ref = [(O.wta(O.adcensus_view(gL[b], gR[b], D, SC, SS, 0)), O.wta(O.adcensus_view(gL[b], gR[b], D, SC, SS, 1)))
               for b in range(P)]
        Lt, Rt = torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory()
        for out_dtype, fill in ((torch.float32, -1.0), (torch.uint8, 255)):
            if out_dtype == torch.uint8 and D > 256:
                continue
            hb = smt.ADCensusHostBatch(H, W, D, SC, SS, channels=channels, out_dtype=out_dtype, chunk=chunk)
            ol = torch.full((P, H, W), fill, dtype=out_dtype).pin_memory()
            orr = torch.full((P, H, W), fill, dtype=out_dtype).pin_memory()
            dl, dr = hb.run(Lt, Rt, ol, orr)
            hb.close()
            cast = np.float32 if out_dtype == torch.float32 else np.uint8
            for b in range(P):
                assert np.array_equal(dl[b].numpy(), ref[b][0].astype(cast)), (channels, out_dtype, b, "L")
                assert np.array_equal(dr[b].numpy(), ref[b][1].astype(cast)), (channels, out_dtype, b, "R")


def test_slot_reuse_across_runs(smt):
    """One handle per chunk (1 and 3) runs 24, then 10, then 24 pairs of different data through the same slots:
    every map right after each run, so no slot was read after it was overwritten."""
    H, W, D = 20, 110, 128
    for chunk in (1, 3):
        hb = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=chunk)
        for P, seed in ((24, 7), (10, 900), (24, 31)):
            L, R = pairs_u8(H, W, D, P, seed + chunk)
            refl, refr = device_batch(smt, L, R, D)
            dl, dr = hb.run(torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory())
            assert same(dl.numpy(), refl) and same(dr.numpy(), refr), (chunk, P, seed)
        hb.close()


def test_pageable_tensors(smt):
    H, W, D = 24, 130, 64
    L, R = pairs_u8(H, W, D, 7, 55)
    hb = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=2)
    pl, pr = hb.run(torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory())
    assert hb.stats()["pinned_in"] == 1
    ql = torch.empty((7, H, W))
    qr = torch.empty((7, H, W))
    hb.run(torch.from_numpy(L.copy()), torch.from_numpy(R.copy()), ql, qr)
    st = hb.stats()
    assert st["pinned_in"] == 0 and st["pinned_out"] == 0
    assert same(ql.numpy(), pl.numpy()) and same(qr.numpy(), pr.numpy())
    hb.close()


@pytest.mark.parametrize("out_dtype,esz", [(torch.float32, 4), (torch.uint8, 1)])
@pytest.mark.parametrize("channels", [1, 3])
def test_stats_byte_counts(smt, out_dtype, esz, channels):
    H, W, D, P, chunk = 16, 77, 64, 11, 4
    hb = smt.ADCensusHostBatch(H, W, D, SC, SS, channels=channels, out_dtype=out_dtype, chunk=chunk)
    shp = (P, H, W) + ((3,) if channels == 3 else ())
    rng = np.random.default_rng(3)
    L = torch.from_numpy(rng.integers(0, 256, shp, dtype=np.uint8)).pin_memory()
    R = torch.from_numpy(rng.integers(0, 256, shp, dtype=np.uint8)).pin_memory()
    hb.run(L, R)
    st = hb.stats()
    assert st["h2d_bytes"] == 2 * P * H * W * channels
    assert st["d2h_bytes"] == 2 * P * H * W * esz
    assert st["chunks"] == (P + chunk - 1) // chunk
    assert st["wall_ms"] > 0 and st["compute_ms"] > 0 and st["h2d_ms"] > 0 and st["d2h_ms"] > 0
    hb.close()


def test_edge_cases(smt):
    H, W, D = 16, 70, 64
    hb = smt.ADCensusHostBatch(H, W, D, SC, SS, chunk=4)
    ol = torch.full((0, H, W), 7.0)
    dl, dr = hb.run(torch.empty((0, H, W), dtype=torch.uint8), torch.empty((0, H, W), dtype=torch.uint8), ol,
                    torch.full((0, H, W), 7.0))
    assert dl.shape == (0, H, W) and dr.shape == (0, H, W)
    L = torch.from_numpy(pairs_u8(H, W, D, 1, 5)[0])
    keep = torch.full((1, H, W), 7.0)
    good = torch.zeros((2, H, W), dtype=torch.uint8)
    with pytest.raises(ValueError):
        hb.run(L.float(), L)                                          # wrong dtype
    with pytest.raises(ValueError):
        hb.run(L[:, :, :-1].contiguous(), L[:, :, :-1].contiguous())  # wrong shape
    with pytest.raises(ValueError):
        hb.run(good, L)                                               # L and R of different pair counts
    with pytest.raises(ValueError):
        hb.run(L.to(DEV), L.to(DEV))                                  # on the GPU
    with pytest.raises(ValueError):
        hb.run(L, L, keep.to(torch.float64), keep)                    # wrong output dtype
    with pytest.raises(ValueError):
        hb.run(L, L, keep.to(DEV), keep)                              # output on the GPU
    big = torch.zeros((1, H, 2 * W), dtype=torch.uint8)
    with pytest.raises(ValueError):
        hb.run(big[:, :, ::2], big[:, :, ::2])                        # right shape, non-contiguous
    assert torch.equal(keep, torch.full((1, H, W), 7.0))
    with pytest.raises(ValueError):
        smt.ADCensusHostBatch(H, W, D, channels=2)
    hb.close()
