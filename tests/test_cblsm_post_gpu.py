"""The tail of CBLSM.cpp (:160-162) on the device: smt_cblsm_tail_batch (api.CBLSMTail) on maps, CBLSMFlow.run_post,
CrossAggFlow.run_post and shard.cblsm_post_batch, against the oracle chain LeftRightConsistency(5) ->
RemoveSpeckles(1, 50, INT_MIN) -> MedianFilter in place (orc_median with in == out)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import median_inplace_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

INT_MIN = -(2 ** 31)
_bgr_cache = {}
_flow_cache = {}


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _chain(O, dL, dR, gate=5, diff=1, area=50, wnd=3):
    """(after LR check, after speckles, finished map, cls, (n_occ, n_mis)) from the oracle"""
    lr, cls, no, nm = O.lrcheck(dL, dR, gate)
    sp = O.remove_speckles(lr, diff, area, INT_MIN)
    return lr, sp, MC.oracle_inplace(sp, wnd), cls, (no, nm)


def _surface_pair(H, W, seed):
    """A slanted disparity surface with a step, its right view by forward warping, about 10 % of the left pixels
    replaced by random disparities (the LR check rejects most of them) and a few 3 x 4 islands that are consistent in
    both views (they survive the LR check and are speckles)."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:H, 0:W]
    d = np.floor(4 + 0.04 * j + 0.05 * i).astype(np.int64)
    d[:, W // 2:] += 3
    d = np.minimum(d, 30)
    for k in range(4):
        y, x = 5 + (k * 9) % max(1, H - 10), 35 + (k * 37) % max(1, W - 45)
        if y + 3 <= H and x + 4 <= W:
            d[y:y + 3, x:x + 4] += 12
    dR = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            if x - d[y, x] >= 0:
                dR[y, x - d[y, x]] = d[y, x]
    bad = rng.random((H, W)) < 0.10
    dL = np.where(bad, rng.integers(0, 60, (H, W)), d)
    return dL.astype(np.float32), dR.astype(np.float32)


@pytest.mark.parametrize("H,W", ((40, 33), (120, 200)))
def test_tail_on_maps_against_oracle_chain(smt, O, H, W):
    pairs = [_surface_pair(H, W, 10 * H + s) for s in range(3)]
    dL, dR = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    tl, tr = _T(dL), _T(dR)
    out, cls, counts = smt.CBLSMTail(tl, tr)
    assert out is tl
    assert np.array_equal(tr.cpu().numpy(), dR)
    rejected = speckled = 0
    for b in range(3):
        lr, sp, fin, ocls, (no, nm) = _chain(O, dL[b], dR[b])
        rejected += no + nm
        speckled += int(np.sum(lr.view(np.uint32) != sp.view(np.uint32)))
        assert MC.same_bits(out[b].cpu().numpy(), fin), b
        assert np.array_equal(cls[b].cpu().numpy(), ocls), b
        assert tuple(counts[b].cpu().numpy()) == (no, nm), b
    assert rejected >= 1 and speckled >= 1, (rejected, speckled)
    # non-default parameters, a single [H][W] pair
    o1, c1, n1 = smt.CBLSMTail(_T(dL[0]), _T(dR[0]), gate=2, speckle_min_area=20, median_wnd=5)
    _, _, fin, ocls, cnt = _chain(O, dL[0], dR[0], gate=2, area=20, wnd=5)
    assert MC.same_bits(o1.cpu().numpy(), fin) and np.array_equal(c1.cpu().numpy(), ocls)
    assert tuple(n1[0].cpu().numpy()) == cnt


# ---- the flows: helpers copied from tests/test_cblsm_flow_gpu.py and tests/test_crossagg_flow_gpu.py -----------------
def _oracle(O, L, R, D, maxlen=34, sec=17, tau=25):
    """CBLSM.cpp:64-67, 101-104, 133-153 composed from the oracle's pieces, in the file's order."""
    aL = O.arms_all(L, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    aR = O.arms_all(R, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    cr, _ = O.aggregate_rect(O.cblsm_ad(L, R, D, 1), aR, 1)                     # :146 right volume, right arms
    cl, _ = O.aggregate_rect(O.cblsm_ad(L, R, D, 0), aL, 1)                     # :147
    cl2, _ = O.aggregate_rect(cl, aL, 1)                                       # :149
    cr2, _ = O.aggregate_rect(cr, aL, 1)                                       # :150 right volume, LEFT arms
    return cl, cr, O.wta(cl2), O.wta(cr2)                                      # :152-153


def _bgr(O, gray, seed):
    key = (gray.shape, gray.tobytes(), seed)
    if key not in _bgr_cache:
        _bgr_cache[key] = O.synth_bgr(gray, seed)
    return _bgr_cache[key]


def _expect(O, bgr, L, R, D, view, iters=4, **p):
    """(aggregated volume, map) of one view (0 left, 1 right): CBLSM.cpp:133-134, 139-143, 152.  From the compiled
    reference where it exists, else from the oracle."""
    if O.have_ref() and O.have_ref_cblsm():
        _, vol = O.ref_crossagg(bgr, O.ref_cblsm_ad(L, R, D, view), iters=iters, **p)
        return vol, O.ref_cblsm_disp(vol)
    _, vol = O.crossagg(bgr, O.cblsm_ad(L, R, D, view), iters=iters, **p)
    return vol, O.wta(vol)


SHAPES = ((120, 200, 60, 3), (40, 33, 16, 2))


def _cblsm_case(O, H, W, D, P):
    """images and the oracle's maps of the CBLSM flow with its tail, computed once per shape"""
    key = ("cblsm", H, W, D, P)
    if key not in _flow_cache:
        pairs = [O.synth_pair(H, W, D, 50 + H + s) for s in range(P)]
        raw = [_oracle(O, l, r, D)[2:] for l, r in pairs]
        fin = [_chain(O, dl, dr) for dl, dr in raw]
        _flow_cache[key] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), raw, fin)
    return _flow_cache[key]


def _check_flow(smt, f, run, run_post, raw, fin, P):
    """run / run_post are closures over the inputs; raw[b] = (dl, dr) of the flow, fin[b] = _chain of them"""
    a = run_post()
    f.status()
    for b in range(P):
        assert MC.same_bits(a[0][b].cpu().numpy(), fin[b][2]), ("dispL", b)
        assert np.array_equal(a[1][b].cpu().numpy(), raw[b][1]), ("dispR", b)
        assert np.array_equal(a[2][b].cpu().numpy(), fin[b][3]), ("cls", b)
        assert tuple(a[3][b].cpu().numpy()) == fin[b][4], ("counts", b)
    r = run()
    for b in range(P):
        assert np.array_equal(r[0][b].cpu().numpy(), raw[b][0]) and np.array_equal(r[1][b].cpu().numpy(), raw[b][1]), b
    b2 = run_post()
    f.status()
    before = smt.scratch_info()[0]
    b3 = run_post()
    f.status()
    assert smt.scratch_info()[0] == before, "the scratch arena grew on a warm call"
    for x, y in zip(a, b2):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for x, y in zip(a, b3):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("H,W,D,P", SHAPES)
def test_cblsm_flow_run_post(smt, O, H, W, D, P):
    L, R, raw, fin = _cblsm_case(O, H, W, D, P)
    Lt, Rt = _T(L), _T(R)
    f = smt.CBLSMFlow(H, W, D)
    _check_flow(smt, f, lambda: f.run(Lt, Rt), lambda: f.run_post(Lt, Rt), raw, fin, P)
    f.close()


@pytest.mark.parametrize("gray_given", (False, True))
@pytest.mark.parametrize("H,W,D,P", SHAPES)
def test_crossagg_flow_run_post(smt, O, H, W, D, P, gray_given):
    from stereo_match_traditional_amd._lib import SMT_ERR_ARG
    key = ("crossagg", H, W, D, P)
    if key not in _flow_cache:
        cases = []
        for s in range(P):
            L, R = O.synth_pair(H, W, D, 70 + H + s)
            cases.append((_bgr(O, L, 170 + s), _bgr(O, R, 270 + s)))
        # the flow's gray pair is cvtColor of the colour pair, whether the caller passes it or the flow derives it
        grays = [(O.bgr2gray(bl), O.bgr2gray(br)) for bl, br in cases]
        raw = [(_expect(O, bl, gl, gr, D, 0)[1], _expect(O, br, gl, gr, D, 1)[1]) for (bl, br), (gl, gr) in zip(cases, grays)]
        fin = [_chain(O, dl, dr) for dl, dr in raw]
        _flow_cache[key] = (cases, grays, raw, fin)
    cases, grays, raw, fin = _flow_cache[key]
    bL, bR = _T(np.stack([c[0] for c in cases])), _T(np.stack([c[1] for c in cases]))
    g = (_T(np.stack([x[0] for x in grays])), _T(np.stack([x[1] for x in grays]))) if gray_given else (None, None)
    f = smt.CrossAggFlow(H, W, D, gate=1)                   # the handle's gate must not reach run_post
    _check_flow(smt, f, lambda: f.run(bL, bR, *g), lambda: f.run_post(bL, bR, *g), raw, fin, P)
    with pytest.raises(smt.SmtError) as ei:
        f.run_post(bL, bR, median_wnd=8)
    assert ei.value.status == SMT_ERR_ARG
    f.close()


def test_sharded_without_process_group(smt, O):
    from stereo_match_traditional_amd import shard
    H, W, D, P = SHAPES[1]
    L, R, raw, fin = _cblsm_case(O, H, W, D, P)
    dl, dr = shard.run_sharded(_T(L), _T(R), D, shard.cblsm_post_batch)
    assert dl.shape == (P, H, W)
    for b in range(P):
        assert MC.same_bits(dl[b].cpu().numpy(), fin[b][2]), b
        assert np.array_equal(dr[b].cpu().numpy(), raw[b][1]), b


def test_cblsm_main_post_switch(smt, O):
    """host/cblsm_main.cpp --post: CBLSM.cpp:160-162 through the C++ mirror (MedianFilter(d, d, ...) routed to the
    in-place entry); without the switch the output has no tail lines."""
    import subprocess
    exe = os.path.join(MC.ROOT, "stereo_match_traditional_amd", "lib", "cblsm_main")
    assert os.path.exists(exe)
    H, W, D, seed = 40, 66, 16, 6
    r = subprocess.run([exe, str(H), str(W), str(D), str(seed), "--post"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    L, R = O.synth_pair(H, W, D, seed)
    _, _, dl, dr = _oracle(O, L, R, D)
    _, _, fin, _, (no, nm) = _chain(O, dl, dr)
    assert got["disp_left"] == f"{O.fnv1a(dl):016x}" and got["disp_right"] == f"{O.fnv1a(dr):016x}"
    assert got["disp_left_post"] == f"{O.fnv1a(fin):016x}"
    assert (int(got["occlusion"]), int(got["mismatches"])) == (no, nm)
    r = subprocess.run([exe, str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "disp_left_post" not in r.stdout
