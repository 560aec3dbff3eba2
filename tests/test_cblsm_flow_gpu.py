"""smt_cblsm_flow_run_batch (api.CBLSMFlow, shard.cblsm_batch): CBLSM.cpp's active flow for batches of pairs, its
first pass from a summed-area table.  Maps against the oracle's composition of CBLSM.cpp:64-67, 101-104, 133-153,
first-pass volumes bit for bit against the oracle or against the composed device path (smt_cblsm_ad +
costAggregationV5 on the same arms), at the exactness bound of the summed-area pass and past it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle(O, L, R, D, maxlen=34, sec=17, tau=25):
    """CBLSM.cpp:64-67, 101-104, 133-153 composed from the oracle's pieces, in the file's order."""
    aL = O.arms_all(L, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    aR = O.arms_all(R, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    cr, _ = O.aggregate_rect(O.cblsm_ad(L, R, D, 1), aR, 1)                     # :146 right volume, right arms
    cl, _ = O.aggregate_rect(O.cblsm_ad(L, R, D, 0), aL, 1)                     # :147
    cl2, _ = O.aggregate_rect(cl, aL, 1)                                       # :149
    cr2, _ = O.aggregate_rect(cr, aL, 1)                                       # :150 right volume, LEFT arms
    return cl, cr, O.wta(cl2), O.wta(cr2)                                      # :152-153


def _device_composed(smt, Lt, Rt, D, **params):
    """The same flow as single calls of the library (two crossarm handles, smt_cblsm_ad, four order-1 aggregations)."""
    import torch
    H, W = Lt.shape
    p = dict(tau=25, sec_length=17, max_length=34)
    p.update(params)
    ca = [smt.CrossArmAggregation().Initialize(H, W, p["tau"], D, Lt.device, style="cblsm", sec_length=p["sec_length"],
                                               max_length=p["max_length"]) for _ in range(2)]
    ca[0].ComputeArmLengths(Lt)
    ca[1].ComputeArmLengths(Rt)
    vl, vr = smt.cblsm_ComputeAD(Lt, Rt, D, smt.VIEW_LEFT), smt.cblsm_ComputeAD(Lt, Rt, D, smt.VIEW_RIGHT)
    gl, gr, g2 = torch.empty_like(vl), torch.empty_like(vl), torch.empty_like(vl)
    dL, dR = torch.empty((H, W), device=Lt.device), torch.empty((H, W), device=Lt.device)
    ca[1].costAggregationV5(vr, gr)
    ca[0].costAggregationV5(vl, gl)
    ca[0].costAggregationV5(gl, g2, dL)
    ca[0].costAggregationV5(gr, g2, dR)
    arms = [[m.clone() for m in c.arm_maps()] for c in ca]
    for c in ca:
        c.status()
        c.close()
    return gl, gr, dL, dR, arms


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _run(smt, L, R, D, **params):
    H, W = L.shape[-2:]
    f = smt.CBLSMFlow(H, W, D, **params)
    dl, dr = f.run(_T(L), _T(R))
    f.status()
    vl, vr = (v.clone() for v in f.volumes())
    f.close()
    return dl.cpu().numpy(), dr.cpu().numpy(), vl, vr


def test_cblsm_cpp_size_against_oracle(smt, O):
    """450x375 D=60 (CBLSM.cpp:28-32): both maps equal the oracle, both first-pass volumes bit-equal."""
    H, W, D = 375, 450, 60
    L, R = O.synth_pair(H, W, D, 6)
    cl, cr, dl, dr = _oracle(O, L, R, D)
    gl, gr, gvl, gvr = _run(smt, L, R, D)
    assert gl.shape == (1, H, W)
    assert np.array_equal(gl[0], dl) and np.array_equal(gr[0], dr)
    assert np.array_equal(_bits(gvl), cl.view(np.uint32))
    assert np.array_equal(_bits(gvr), cr.view(np.uint32))


def test_batch_of_four_pairs_no_state_between_pairs(smt, O):
    H, W, D = 120, 200, 60
    pairs = [O.synth_pair(H, W, D, s, noise=(s == 23)) for s in (21, 22, 23, 24)]
    L = np.stack([p[0] for p in pairs])
    R = np.stack([p[1] for p in pairs])
    gl, gr, gvl, gvr = _run(smt, L, R, D)
    for b, (l, r) in enumerate(pairs):
        cl, cr, dl, dr = _oracle(O, l, r, D)
        assert np.array_equal(gl[b], dl) and np.array_equal(gr[b], dr), b
        al, ar, _, _ = _run(smt, l, r, D)                                     # the pair alone, fresh handle
        assert np.array_equal(al[0], gl[b]) and np.array_equal(ar[0], gr[b]), b
    assert np.array_equal(_bits(gvl), cl.view(np.uint32))                     # the last pair's volumes
    assert np.array_equal(_bits(gvr), cr.view(np.uint32))


@pytest.mark.parametrize("H,W,D", [(24, 40, 64), (1, 70, 16), (50, 1, 8), (31, 47, 1), (33, 65, 17), (20, 41, 300)])
def test_edges_against_oracle(smt, O, H, W, D):
    """W < D, one row, one column, one hypothesis, odd sizes, and D = 300 (five 64-hypothesis chunks; the second pass
    takes the D > 256 aggregation kernel)."""
    L, R = O.synth_pair(H, W, D, 7 + H)
    cl, cr, dl, dr = _oracle(O, L, R, D)
    gl, gr, gvl, gvr = _run(smt, L, R, D)
    assert np.array_equal(gl[0], dl) and np.array_equal(gr[0], dr)
    assert np.array_equal(_bits(gvl), cl.view(np.uint32))
    assert np.array_equal(_bits(gvr), cr.view(np.uint32))


def _flat_pair(H, W, seed):
    """Left 0..6, right 249..255: every neighbour difference is within tau_low (arms run to max_length or the border),
    every AD is 243..255."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 7, (H, W)).astype(np.uint8), rng.integers(249, 256, (H, W)).astype(np.uint8)


@pytest.mark.parametrize("maxlen", [127, 128])
def test_exactness_bound(smt, O, maxlen):
    """max_length 127: rectangles of 255 x 255 taps with sums up to 16.5 M, the summed-area path's bound; its volumes
    are bit-equal to the composed device path (the sequential order-1 walk) and to float64 direct sums divided in
    float32.  max_length 128 takes the materialised path: equal too."""
    H, W, D = 300, 300, 8
    L, R = _flat_pair(H, W, 5)
    Lt, Rt = _T(L), _T(R)
    gl, gr, dL, dR, arms = _device_composed(smt, Lt, Rt, D, max_length=maxlen)
    aL = [a.cpu().numpy() for a in arms[0]]
    assert aL[0].max() == maxlen and aL[2].max() == maxlen and aL[1][H // 2, W // 2] == maxlen
    f = smt.CBLSMFlow(H, W, D, max_length=maxlen)
    fl, fr = f.run(Lt, Rt)
    f.status()
    vl, vr = (v.clone() for v in f.volumes())
    assert np.array_equal(_bits(vl), _bits(gl)) and np.array_equal(_bits(vr), _bits(gr))
    assert np.array_equal(fl[0].cpu().numpy(), dL.cpu().numpy()) and np.array_equal(fr[0].cpu().numpy(), dR.cpu().numpy())
    f.close()
    if maxlen > 127:
        return                                             # past the bound the reference's own sums round
    ad = O.cblsm_ad(L, R, D, 0).astype(np.float64)
    v = _bits(vl).view(np.float32)
    rng = np.random.default_rng(1)
    pix = [(H // 2, W // 2), (0, 0), (H - 1, W - 1), (3, W - 2)] + [tuple(x) for x in rng.integers(0, [H, W], (40, 2))]
    for i, j in pix:
        l, r, u, d = (int(a[i, j]) for a in aL)
        s = ad[i - u:i + d + 1, j - l:j + r + 1].sum(axis=(0, 1))
        n = (u + d + 1) * (l + r + 1)
        assert np.array_equal((s.astype(np.float32) / np.float32(n)).view(np.uint32), v[i, j].view(np.uint32)), (i, j)


def test_kitti_size_two_pairs_against_composed_flow(smt, O):
    import torch
    H, W, D = 375, 1242, 128
    pairs = [O.synth_pair(H, W, D, s) for s in (31, 32)]
    L = _T(np.stack([p[0] for p in pairs]))
    R = _T(np.stack([p[1] for p in pairs]))
    f = smt.CBLSMFlow(H, W, D)
    fl, fr = f.run(L, R)
    f.status()
    vl, vr = f.volumes()
    for b in range(2):
        gl, gr, dL, dR, _ = _device_composed(smt, L[b], R[b], D)
        assert torch.equal(fl[b], dL) and torch.equal(fr[b], dR), b
    assert np.array_equal(_bits(vl), _bits(gl)) and np.array_equal(_bits(vr), _bits(gr))
    f.close()


def test_non_default_stream_and_arguments(smt, O):
    import ctypes as C
    import torch
    from stereo_match_traditional_amd._lib import SMT_ERR_ARG, lib
    H, W, D = 64, 96, 40
    L, R = O.synth_pair(H, W, D, 9)
    _, _, dl, dr = _oracle(O, L, R, D)
    s = torch.cuda.Stream()
    f = smt.CBLSMFlow(H, W, D)
    hostL, hostR = torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory()
    with torch.cuda.stream(s):
        # inputs produced, maps consumed and copied out on the same non-default stream, no host sync in between
        Lt, Rt = hostL.to("cuda:0", non_blocking=True), hostR.to("cuda:0", non_blocking=True)
        ml, mr = f.run(Lt, Rt)
        both = torch.stack([ml[0], mr[0]]) + 0.0
        out = torch.empty(both.shape, dtype=both.dtype, pin_memory=True)
        out.copy_(both, non_blocking=True)
    s.synchronize()
    assert np.array_equal(out[0].numpy(), dl) and np.array_equal(out[1].numpy(), dr)
    f.status()
    # pairs == 0: a no-op, also without buffers
    e = torch.empty((0, H, W), dtype=torch.uint8, device="cuda:0")
    zl, zr = f.run(e, e)
    assert zl.shape == (0, H, W) and zr.shape == (0, H, W)
    assert lib().smt_cblsm_flow_run_batch(f._h, None, None, 0, None, None) == 0
    assert lib().smt_cblsm_flow_run_batch(f._h, None, None, -1, None, None) == SMT_ERR_ARG
    assert lib().smt_cblsm_flow_run_batch(None, None, None, 1, None, None) == SMT_ERR_ARG
    f.status()
    f.close()
    for shape, kw in [((H, W, 0), {}), ((H, W, 513), {}), ((0, W, D), {}), ((H, 0, D), {}), ((H, W, D), dict(tau=-1)),
                      ((H, W, D), dict(tau=256)), ((H, W, D), dict(max_length=4097)), ((H, W, D), dict(max_length=-1)),
                      ((H, W, D), dict(sec_length=-1))]:
        with pytest.raises(smt.SmtError) as ei:
            smt.CBLSMFlow(*shape, **kw)
        assert ei.value.status == SMT_ERR_ARG, (shape, kw)
    h = C.c_void_p()
    assert lib().smt_cblsm_flow_create_on(0, H, W, D, None, C.byref(h)) == 0      # NULL params: the defaults
    assert lib().smt_cblsm_flow_create_on(-1, H, W, D, None, C.byref(C.c_void_p())) == SMT_ERR_ARG
    assert lib().smt_cblsm_flow_volumes(None, None, None) == SMT_ERR_ARG
    assert lib().smt_cblsm_flow_status(None) == SMT_ERR_ARG
    assert lib().smt_cblsm_flow_destroy(h) == 0


def test_sharded_without_process_group(smt, O):
    from stereo_match_traditional_amd import shard
    H, W, D = 48, 80, 32
    pairs = [O.synth_pair(H, W, D, s) for s in (41, 42, 43)]
    L = _T(np.stack([p[0] for p in pairs]))
    R = _T(np.stack([p[1] for p in pairs]))
    dl, dr = shard.run_sharded(L, R, D, shard.cblsm_batch)
    assert dl.shape == (3, H, W)
    for b, (l, r) in enumerate(pairs):
        _, _, ol, orr = _oracle(O, l, r, D)
        assert np.array_equal(dl[b].cpu().numpy(), ol) and np.array_equal(dr[b].cpu().numpy(), orr), b
