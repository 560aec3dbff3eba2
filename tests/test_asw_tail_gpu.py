"""The tail of ASW/ASWeight.cpp (:67-78) on the device against the restatements of tests/asw_tail_cases.py, bit for bit:
every batch primitive into prefilled buffers whose guard bytes between the maps must stay untouched, the normalisation on
every uint8 (min, max) pair in one call, smt_asw_tail_batch stage by stage, ASWFlow.run_post against ASWFlow.run followed
by the restatement, and one case on a busy side stream with late inputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import asw_tail_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPE_IDS = [f"{H}x{W}" for H, W in TC.SHAPES]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def strided(buf, k, H, W):
    """the [k][H][W] view of a flat device buffer holding maps H*W + GAP apart"""
    return torch.as_strided(buf, (k, H, W), (H * W + TC.GAP, W, 1))


def three(make, H, W):
    return [make(H, W, s) for s in range(3)]


def rand_u8(H, W, s):
    rng = np.random.default_rng(7900 + 31 * s + H * 1000 + W)
    m = rng.integers(0, 256, (H, W)).astype(np.uint8)
    if s == 1:
        m = (m % 7 + 100).astype(np.uint8)                  # a narrow range
    if s == 2:
        m[:] = 77                                           # constant: scale 0
    return m


def check_batch(buf, want, H, W):
    got, gaps = TC.split_with_gaps(buf.cpu().numpy(), len(want), H, W)
    assert np.all(gaps == TC.GUARD), "a guard byte between the maps was written"
    for b, w in enumerate(want):
        assert np.array_equal(got[b], w), f"map {b}: {int((got[b] != w).sum())} of {w.size} pixels differ"


@pytest.mark.parametrize("H,W", TC.SHAPES, ids=SHAPE_IDS)
def test_normalize_u8(smt, H, W):
    maps = three(rand_u8, H, W)
    src, _ = TC.batch_with_gaps(maps)
    d_in, d_out = gpu(src), gpu(np.full(src.size, TC.GUARD, np.uint8))
    smt.MinMaxNormalizeU8(strided(d_in, 3, H, W), out=strided(d_out, 3, H, W))
    check_batch(d_out, [TC.ref_normalize(m) for m in maps], H, W)
    assert np.array_equal(d_in.cpu().numpy(), src)
    smt.MinMaxNormalizeU8(strided(d_in, 3, H, W), out=strided(d_in, 3, H, W))          # in == out
    check_batch(d_in, [TC.ref_normalize(m) for m in maps], H, W)


def rand_f32(H, W, s):
    rng = np.random.default_rng(7950 + 31 * s + H * 1000 + W)
    if s == 0:
        return rng.integers(0, 60, (H, W)).astype(np.float32)          # WTA indices, as the flow's maps
    if s == 1:
        return (rng.standard_normal((H, W)) * 1e3).astype(np.float32)  # negatives, fractions
    m = np.full((H, W), -2.5, np.float32)
    m.reshape(-1)[0] = -0.0 if H * W == 1 else 1e-3                    # two values; -0.0 alone (constant: zeros)
    return m


@pytest.mark.parametrize("H,W", TC.SHAPES, ids=SHAPE_IDS)
def test_normalize_f32(smt, H, W):
    maps = three(rand_f32, H, W)
    stride = H * W + TC.GAP
    src = np.full(3 * stride, 12345.0, np.float32)
    for b, m in enumerate(maps):
        src[b * stride: b * stride + H * W] = m.reshape(-1)
    d_in, d_out = gpu(src), gpu(np.full(src.size, TC.GUARD, np.uint8))
    smt.MinMaxNormalizeU8(strided(d_in, 3, H, W), out=strided(d_out, 3, H, W))
    check_batch(d_out, [TC.ref_normalize(m) for m in maps], H, W)


def test_normalize_every_min_max_pair(smt):
    rows = TC.minmax_table()
    d = gpu(rows.reshape(-1, 1, 4))
    out = smt.MinMaxNormalizeU8(d)
    assert np.array_equal(out.cpu().numpy().reshape(-1, 4), TC.ref_normalize_rows(rows))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("H,W", TC.SHAPES, ids=SHAPE_IDS)
def test_median_blur(smt, H, W, k):
    maps = three(rand_u8, H, W)
    maps[2] = TC.tail_maps()[TC.SHAPES.index((H, W))][1]
    src, _ = TC.batch_with_gaps(maps)
    d_in = gpu(src)
    out = smt.MedianBlurU8(strided(d_in, 3, H, W), k)
    assert out.stride() == strided(d_in, 3, H, W).stride()
    want = [TC.ref_median(m, k) for m in maps]
    got = out.cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
    # into a prefilled buffer through the C entry: the guard bytes stay
    d_out = gpu(np.full(src.size, TC.GUARD, np.uint8))
    from stereo_match_traditional_amd._lib import lib
    assert lib().smt_median_blur_u8_batch(d_in.data_ptr(), d_out.data_ptr(), 3, H * W + TC.GAP, W, H, k,
                                          torch.cuda.current_stream().cuda_stream) == 0
    check_batch(d_out, want, H, W)


SPECKLE = TC.speckle_maps()


@pytest.mark.parametrize("name,m,args", SPECKLE, ids=[s[0] for s in SPECKLE])
def test_filter_speckles(smt, name, m, args):
    H, W = m.shape
    maps = [m, np.ascontiguousarray(m[::-1, ::-1]), np.ascontiguousarray(m[::-1])]
    src, _ = TC.batch_with_gaps(maps)
    d = gpu(src)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    smt.FilterSpecklesU8(strided(d, 3, H, W), *args, err=err)
    check_batch(d, [TC.ref_speckles(x, *args) for x in maps], H, W)
    assert int(err.item()) == 0


FILL = TC.fill_maps()


@pytest.fixture(scope="module")
def fill_refs():
    return {n: (TC.ref_fill(m, 0), TC.ref_fill(m, TC.FIX_ROW_END)) for n, m in FILL}


@pytest.mark.parametrize("fix", [0, TC.FIX_ROW_END])
def test_fill_image_new(smt, fill_refs, fix):
    """maps of one shape go in one call, with a stride gap; counts per map"""
    by_shape = {}
    for n, m in FILL:
        by_shape.setdefault(m.shape, []).append(n)
    for (H, W), names in by_shape.items():
        maps = [dict(FILL)[n] for n in names]
        src, _ = TC.batch_with_gaps(maps)
        d = gpu(src)
        _, counts = smt.FillImageNew(strided(d, len(maps), H, W), fix=fix, counts=True)
        refs = [fill_refs[n][1 if fix else 0] for n in names]
        check_batch(d, [r[0] for r in refs], H, W)
        assert [tuple(c) for c in counts.cpu().numpy()] == [r[1] for r in refs], names
        if fix:
            assert not counts.any()
            got, _ = TC.split_with_gaps(d.cpu().numpy(), len(maps), H, W)
            for g, m in zip(got, maps):
                assert np.array_equal(g, TC.ref_fill_own(m))


def test_fill_image_new_rows_longer_than_the_staged_row(smt):
    """W above the row length the search kernel stages: the same rules on the row in global memory"""
    rng = np.random.default_rng(7960)
    m = rng.integers(1, 256, (2, 16390)).astype(np.uint8)
    m[rng.random(m.shape) < 0.7] = 0
    m[0, :] = 0                                              # no left find in row 0: holes at W - T(k) read (1, 0)
    m[0, 9000] = 33
    m[1, 0] = 0
    d = gpu(m)
    _, counts = smt.FillImageNew(d, counts=True)
    want, cnt, _ = TC.ref_fill(m)
    assert np.array_equal(d.cpu().numpy(), want) and tuple(counts.cpu().numpy()[0]) == cnt and cnt[0] > 0


TAIL = TC.tail_maps()


@pytest.mark.parametrize("fix", [0, TC.FIX_ROW_END])
@pytest.mark.parametrize("name,m", TAIL, ids=[t[0] for t in TAIL])
def test_tail_stage_by_stage(smt, name, m, fix):
    H, W = m.shape
    maps = [m, np.ascontiguousarray(m[::-1]), (m // 2).astype(np.uint8)]
    src, _ = TC.batch_with_gaps(maps)
    d = gpu(src)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _, am, af, counts = smt.ASWTail(strided(d, 3, H, W), stages=True, err=err, fix=fix)
    refs = [TC.ref_tail(x, fix=fix) for x in maps]
    check_batch(d, [r[2] for r in refs], H, W)
    for b, r in enumerate(refs):
        assert np.array_equal(am[b].cpu().numpy(), r[0]), ("after_median", b)
        assert np.array_equal(af[b].cpu().numpy(), r[1]), ("after_fill", b)
        assert tuple(counts[b].cpu().numpy()) == r[3]
    assert int(err.item()) == 0


def test_tail_other_parameters_without_copies(smt):
    m = TAIL[5][1]
    d = gpu(m[None].copy())
    _, counts = smt.ASWTail(d, speckle_newval=3, speckle_max_size=9, speckle_max_diff=1, median_first=3, median_last=5)
    r = TC.ref_tail(m, speckle=(3, 9, 1), median_first=3, median_last=5)
    assert np.array_equal(d[0].cpu().numpy(), r[2]) and tuple(counts[0].cpu().numpy()) == r[3]


# ------------------------------------------------------------------------------------------------------- the flow
def _pairs(n, H, W, D, seed):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (n, H, W + D)).astype(np.uint8)
    L = (L // 32 * 32 + rng.integers(0, 8, L.shape)).astype(np.uint8)
    shift = rng.integers(1, D - 1, (n, H // 4 + 1)).repeat(4, axis=1)[:, :H]
    R = np.stack([np.stack([np.roll(L[b, y], -int(shift[b, y])) for y in range(H)]) for b in range(n)])
    return np.ascontiguousarray(L[:, :, :W]), np.ascontiguousarray(R[:, :, :W])


def _check_post(r, dl, dr, last):
    """run_post's outputs against run's maps followed by the restatement"""
    assert np.array_equal(r["dispL"].cpu().numpy().view(np.uint32), dl.cpu().numpy().view(np.uint32))
    assert np.array_equal(r["dispR"].cpu().numpy().view(np.uint32), dr.cpu().numpy().view(np.uint32))
    for b in range(dl.shape[0]):
        am, af, fin, counts = TC.ref_tail(last[b].cpu().numpy())
        assert np.array_equal(r["after_median"][b].cpu().numpy(), am), b
        assert np.array_equal(r["after_fill"][b].cpu().numpy(), af), b
        assert np.array_equal(r["lastDisp"][b].cpu().numpy(), fin), b
        assert tuple(r["fill_counts"][b].cpu().numpy()) == counts
        assert np.array_equal(r["dispL8"][b].cpu().numpy(), TC.ref_normalize(r["dispL"][b].cpu().numpy())), b
        assert np.array_equal(r["dispR8"][b].cpu().numpy(), TC.ref_normalize(r["dispR"][b].cpu().numpy())), b


def test_flow_run_post(smt):
    H, W, D = 24, 40, 8
    flow = smt.ASWFlow(H, W, D, DEV, winSize=2)
    try:
        L, R = _pairs(3, H, W, D, 7970)
        dl, dr, last = flow.run(gpu(L[:2]), gpu(R[:2]))
        assert int((last == 0).sum()) > 0 and int((last != 0).sum()) > 0
        _check_post(flow.run_post(gpu(L[:2]), gpu(R[:2])), dl, dr, last)
        flow.status()
        # the same handle with another pair count
        dl, dr, last = flow.run(gpu(L), gpu(R))
        _check_post(flow.run_post(gpu(L), gpu(R)), dl, dr, last)
        dl, dr, last = flow.run(gpu(L[2]), gpu(R[2]))
        _check_post(flow.run_post(gpu(L[2]), gpu(R[2])), dl, dr, last)
        flow.status()
    finally:
        flow.close()


def test_shard_asw_post_batch(smt):
    from stereo_match_traditional_amd import shard
    H, W, D = 24, 40, 8
    L, R = _pairs(2, H, W, D, 7971)
    fin, l8 = shard.asw_post_batch(gpu(L), gpu(R), D, winSize=2)
    flow = smt.ASWFlow(H, W, D, DEV, winSize=2)
    dl, _, last = flow.run(gpu(L), gpu(R))
    flow.close()
    for b in range(2):
        assert np.array_equal(fin[b].cpu().numpy(), TC.ref_tail(last[b].cpu().numpy())[2])
        assert np.array_equal(l8[b].cpu().numpy(), TC.ref_normalize(dl[b].cpu().numpy()))


def test_matchers_main_asw_post(smt, O, tmp_path):
    """host/matchers_main --asw-post: smt::ASWTail on the cross-checked map, the three files of ASWeight.cpp:75-79"""
    import subprocess
    import stereo_match_traditional_amd.api as api
    exe = os.path.join(os.path.dirname(smt.__file__), "lib", "matchers_main")
    H, W, D, seed = 40, 90, 32, 5
    r = subprocess.run([exe, "--asw-post", str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=120,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    L, R = O.synth_pair(H, W, D, seed)
    flow = smt.ASWFlow(H, W, D, DEV, winSize=3)
    _, _, last = flow.run(gpu(L), gpu(R))
    flow.close()
    last = last[0].cpu().numpy()
    assert got["asw_cross"] == f"{O.fnv1a(last):016x}"
    am, af, fin, counts = TC.ref_tail(last)
    for key, want, path in (("asw_speckle", am, "speckle.png"), ("asw_filled", af, "filled.png"),
                            ("asw_medain", fin, "medain.png")):
        assert got[key] == f"{O.fnv1a(want):016x}", key
        assert np.array_equal(np.asarray(api.imread(str(tmp_path / path), 1)).reshape(H, W), want), path
    assert int(got["asw_fill_no_push"]) == counts[0]


def test_tail_on_a_busy_side_stream_with_late_inputs(smt):
    """the manner of tests/test_stream_order_gpu.py: the stream is busy, the inputs exist only behind the work in front
    of the call, a consumer on the same stream reads the results, nothing synchronises in between"""
    import test_stream_order_gpu as TSO
    name, m = TAIL[4]
    H, W = m.shape
    maps = [m, np.ascontiguousarray(m[::-1]), (m // 2).astype(np.uint8)]
    src, _ = TC.batch_with_gaps(maps)
    real = gpu(src)
    d = gpu(np.ascontiguousarray(src[::-1]))                 # decoys until the copy behind the sleep
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    smt.ASWTail(gpu(m[None].copy()))                         # warm: the arena holds the scratch
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(TSO.DELAY)
        slept = torch.cuda.Event()
        slept.record()
        d.copy_(real, non_blocking=True)
        _, am, af, counts = smt.ASWTail(strided(d, 3, H, W), stages=True, err=err)
        running = not slept.query()
        snap, am, af, counts = d.clone(), am.clone(), af.clone(), counts.clone()
    side.synchronize()
    torch.cuda.synchronize()
    assert running, "smt_asw_tail_batch returned only after the work in front of it: it synchronised"
    refs = [TC.ref_tail(x) for x in maps]
    check_batch(snap, [r[2] for r in refs], H, W)
    for b, r in enumerate(refs):
        assert np.array_equal(am[b].cpu().numpy(), r[0]) and np.array_equal(af[b].cpu().numpy(), r[1])
        assert tuple(counts[b].cpu().numpy()) == r[3]
    assert int(err.item()) == 0
