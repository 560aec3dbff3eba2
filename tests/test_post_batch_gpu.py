"""Batched post-filters on the GPU: smt_remove_speckles_batch and smt_median_filter_batch against the oracle and the
single-map entries, their asynchrony, and main.cpp:93-94 as the pipeline's tail (smt_pipeline_run_batch_post)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INT_MIN = -(2 ** 31)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_hashes.json")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def strided(maps, pad=37):
    """[P][H][W] device view whose maps lie H*W + pad elements apart (a non-dense batch)."""
    P, (H, W) = len(maps), maps[0].shape
    base = torch.full((P, H * W + pad), 12345.0, dtype=torch.float32, device=DEV)
    view = base[:, :H * W].view(P, H, W)
    view.copy_(T(np.stack(maps)))
    return base, view


def check_speckles(smt, O, maps, diff, area, inv, single=False):
    base, view = strided([np.asarray(m, np.float32) for m in maps])
    smt.RemoveSpecklesBatch(view, diff, area, inv)
    got = view.cpu().numpy()
    assert (base[:, -37:] == 12345.0).all(), "wrote past a map"
    H, W = maps[0].shape
    for b, m in enumerate(maps):
        ref = O.remove_speckles(m, diff, area, inv)
        assert np.array_equal(bits(got[b]), bits(ref)), (b, H, W, diff, area, inv, int((bits(got[b]) != bits(ref)).sum()))
        if single:
            t = T(np.array(m, np.float32))
            smt.RemoveSpeckles(t, W, H, diff, area, inv)
            assert np.array_equal(bits(t.cpu().numpy()), bits(ref)), b


def random_map(H, W, seed):
    """test_remove_speckles' maps: piecewise-constant planes + 0/1 noise, raised spots, +inf holes."""
    rng = np.random.default_rng(seed)
    base = (np.add.outer(np.arange(H) // 11, np.arange(W) // 13) * 3).astype(np.float32)
    d = base + rng.integers(0, 2, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.03] += 20
    d[rng.random((H, W)) < 0.04] = np.inf
    return d


@pytest.mark.parametrize("diff,area", [(1, 30), (0, 5), (2, 80)])
def test_remove_speckles_batch_random_maps(smt, O, diff, area):
    maps = [random_map(60, 90, s) for s in (1, 2, 3)]
    check_speckles(smt, O, maps, diff, area, INT_MIN, single=True)
    finite = [np.where(np.isinf(m), np.float32(65535.0), m) for m in maps]
    check_speckles(smt, O, finite, diff, area, 65535, single=True)


def serpentine(H, W):
    """One-pixel-wide path (1.0) along every even row, joined at alternate ends through the odd rows (50.0 elsewhere):
    one region crossing every tile edge."""
    a = np.full((H, W), 50.0, np.float32)
    a[0::2] = 1.0
    for r in range(1, H, 2):
        a[r, W - 1 if (r // 2) % 2 == 0 else 0] = 1.0
    return a


def spiral(n):
    """Square spiral path of 1.0 with a one-pixel gap between its arms, on 50.0."""
    g = np.zeros((n + 2, n + 2), bool)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = True                    # frame: the spiral keeps one pixel away from it
    a = np.zeros_like(g)
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    r, c, k = 1, 1, 0
    a[r, c] = True

    def free(r, c, k):
        dr, dc = dirs[k]
        return not (g[r + 2 * dr, c + 2 * dc] or a[r + 2 * dr, c + 2 * dc]) if 0 <= r + 2 * dr < n + 2 and 0 <= c + 2 * dc < n + 2 else False

    for _ in range(4 * n * n):
        if free(r, c, k):
            pass
        elif free(r, c, (k + 1) % 4):
            k = (k + 1) % 4
        else:
            break
        r, c = r + dirs[k][0], c + dirs[k][1]
        a[r, c] = True
    return np.where(a[1:-1, 1:-1], np.float32(1.0), np.float32(50.0))


def test_remove_speckles_batch_serpentine_1080p(smt, O):
    a = serpentine(1080, 1920)
    path = int((a == 1.0).sum())
    # the whole path is one region: kept at exactly its size, removed one above it
    check_speckles(smt, O, [a, a], 1, path, INT_MIN)
    check_speckles(smt, O, [a], 1, path + 1, INT_MIN)
    b = a.copy()
    b[::7, 3::11] = 9.0                                                 # cuts and speckles along the path
    check_speckles(smt, O, [a, b, a[::-1]], 1, 30, INT_MIN)


def test_remove_speckles_batch_spiral(smt, O):
    a = spiral(301)
    n = int((a == 1.0).sum())
    assert n > 301 * 301 // 3
    check_speckles(smt, O, [a, a.T.copy()], 1, n, INT_MIN)
    check_speckles(smt, O, [a], 1, n + 1, INT_MIN)


def test_remove_speckles_batch_chains_through_tile_corners(smt, O):
    """Regions linked only diagonally: the two diagonals of a 256 x 256 map cross every tile corner they meet, and
    two-pixel diagonal pairs straddle every tile corner of the map."""
    n = 256
    a = np.full((n, n), 50.0, np.float32)
    i = np.arange(n)
    a[i, i] = 1.0
    a[i, n - 1 - i] = 3.0
    a[n // 2 - 1: n // 2 + 1] = 50.0                                     # the two diagonals do not touch
    size1 = int((a == 1.0).sum())
    check_speckles(smt, O, [a], 1, size1 // 2, INT_MIN)
    check_speckles(smt, O, [a], 1, size1 // 2 + 1, INT_MIN)
    c = np.full((200, 300), 50.0, np.float32)
    for y in range(32, 200, 32):
        for x in range(32, 300, 32):
            c[y - 1, x - 1] = c[y, x] = 1.0                            # down-right across the corner
            if x + 2 < 300:
                c[y - 1, x + 1] = 7.0                                      # isolated
    d = np.full((200, 300), 50.0, np.float32)
    for y in range(32, 200, 32):
        for x in range(32, 300, 32):
            d[y - 1, x] = d[y, x - 1] = 1.0                            # down-left across the corner
    check_speckles(smt, O, [c, d], 1, 2, INT_MIN)
    check_speckles(smt, O, [c, d], 1, 3, INT_MIN)


def test_remove_speckles_batch_checkerboard_and_constant(smt, O):
    H, W = 97, 130
    y, x = np.mgrid[0:H, 0:W]
    chk = (4 * (2 * (y % 2) + (x % 2))).astype(np.float32)           # every 8-neighbour differs by >= 4: all singletons
    check_speckles(smt, O, [chk, chk + 1], 1, 2, INT_MIN)
    check_speckles(smt, O, [chk], 1, 1, INT_MIN)
    const = np.full((H, W), 7.0, np.float32)
    check_speckles(smt, O, [const, const], 1, H * W, INT_MIN)           # one region, kept at its exact size
    check_speckles(smt, O, [const], 0, H * W + 1, INT_MIN)
    big = np.full((1080, 1920), 7.0, np.float32)
    check_speckles(smt, O, [big], 1, 1080 * 1920, INT_MIN)
    check_speckles(smt, O, [big], 1, 1080 * 1920 + 1, INT_MIN)


def test_remove_speckles_batch_exact_area_regions(smt, O):
    a = np.full((80, 120), 100.0, np.float32)
    a[2:7, 2:8] = 1.0                                                    # 30 pixels
    a[10:15, 2:8] = 5.0
    a[14, 7] = 100.0                                                     # 29 pixels
    a[20:25, 30:36] = 9.0
    a[24, 35] = 100.0                                                    # 29, straddling nothing
    a[29:34, 29:35] = 13.0                                               # 30, across the tile corner at (32, 32)
    a[60:63, 60:70] = 17.0                                               # 30, across a tile edge
    a[70:73, 90:100] = 21.0
    a[72, 99] = 100.0                                                    # 29
    check_speckles(smt, O, [a, a[::-1, ::-1]], 1, 30, INT_MIN)
    check_speckles(smt, O, [a], 1, 29, INT_MIN)
    check_speckles(smt, O, [a], 1, 31, INT_MIN)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 1000), (1000, 1), (7, 1000), (33, 65), (97, 31), (64, 64), (45, 250)])
def test_remove_speckles_batch_shapes(smt, O, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    maps = [rng.integers(0, 4, (H, W)).astype(np.float32) for _ in range(3)]
    check_speckles(smt, O, maps, 1, 5, INT_MIN)
    check_speckles(smt, O, maps, 0, 3, INT_MIN)


def test_remove_speckles_batch_non_finite_and_invalid_values(smt, O):
    rng = np.random.default_rng(9)
    H, W = 70, 110
    maps = []
    for s in range(3):
        d = rng.integers(0, 3, (H, W)).astype(np.float32)
        r = rng.random((H, W))
        d[r < 0.05] = np.nan
        d[(r >= 0.05) & (r < 0.10)] = np.inf
        d[(r >= 0.10) & (r < 0.13)] = -np.inf
        d[(r >= 0.13) & (r < 0.18)] = 65535.0
        d[(r >= 0.18) & (r < 0.20)] = float(INT_MIN)
        d[(r >= 0.20) & (r < 0.25)] = -0.0
        d[20:40, 30:60] = np.inf                                         # a block of +inf: inf - inf is NaN, never linked
        maps.append(d)
    for inv in (INT_MIN, 65535, 0, 2):
        for diff, area in ((1, 30), (0, 4), (2, 1000)):
            check_speckles(smt, O, maps, diff, area, inv)


@pytest.mark.parametrize("diff,area", [(1, 0), (1, 1), (1, 2 ** 32 - 1), (1, 2 ** 31), (-1, 2), (0, 2), (-5, 0),
                                       (2 ** 31 - 1, 50)])
def test_remove_speckles_batch_extreme_parameters(smt, O, diff, area):
    maps = [random_map(50, 70, s) for s in (4, 5)]
    check_speckles(smt, O, maps, diff, area, INT_MIN)


@pytest.mark.parametrize("wnd", [1, 3, 5, 7])
def test_median_filter_batch(smt, O, wnd):
    rng = np.random.default_rng(wnd)
    H, W = 37, 53
    maps = []
    for s in range(3):
        d = rng.integers(0, 60, (H, W)).astype(np.float32)
        d[rng.random((H, W)) < 0.1] = np.inf
        maps.append(d)
    _, view = strided(maps)
    got = smt.MedianFilterBatch(view, wnd).cpu().numpy()
    dense = smt.MedianFilterBatch(T(np.stack(maps)), wnd).cpu().numpy()
    for b, d in enumerate(maps):
        ref = O.median(d, wnd)
        assert np.array_equal(bits(got[b]), bits(ref)), (wnd, b)
        assert np.array_equal(bits(dense[b]), bits(ref)), (wnd, b)
        assert np.array_equal(bits(smt.MedianFilter(T(d), W, H, wnd).cpu().numpy()), bits(ref)), (wnd, b)


def test_remove_speckles_batch_is_asynchronous(smt, O):
    """Enqueued behind a long sleep on a side stream, the call returns while the stream is still busy (the single-map
    entry synchronises); the maps are right once the stream has run."""
    maps = [random_map(60, 90, s) for s in (1, 2, 3)]
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        warm = T(np.stack(maps))
        smt.RemoveSpecklesBatch(warm, 1, 30, INT_MIN)                    # the arena holds the scratch from here on
        s.synchronize()
        t = T(np.stack(maps))
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        smt.RemoveSpecklesBatch(t, 1, 30, INT_MIN)
        pending = not s.query()
    s.synchronize()
    assert pending, "smt_remove_speckles_batch waited for the stream"
    got = t.cpu().numpy()
    for b, m in enumerate(maps):
        assert np.array_equal(bits(got[b]), bits(O.remove_speckles(m, 1, 30, INT_MIN))), b


def oracle_pipeline(O, L, R, D):
    cl = O.adcensus_view(L, R, D, 10.0, 30.0, 0)
    cr = O.adcensus_view(L, R, D, 10.0, 30.0, 1)
    al, _ = O.aggregate_rect(cl, O.arms_all(L), 0)
    ar, _ = O.aggregate_rect(cr, O.arms_all(R), 0)
    d_so, d_r = O.wta(O.scanline(al, L.astype(np.float32), 10, 150)), O.wta(ar)
    return O.lrcheck(d_so, d_r, 2)[0]


@pytest.mark.parametrize("schedule", ["default", "0", "1", "2"])
def test_pipeline_run_post_small_pairs_vs_oracle(smt, O, schedule, monkeypatch):
    if schedule != "default":
        monkeypatch.setenv("SMT_PIPE_SCHEDULE", schedule)
    H, W, D, P = 40, 96, 32, 5
    pairs = [O.synth_pair(H, W, D, 20 + b, b == 1) for b in range(P)]
    Lb = T(np.stack([p[0] for p in pairs]))
    Rb = T(np.stack([p[1] for p in pairs]))
    pipe = smt.Pipeline(H, W, D, DEV)
    dl0, dr0, cls0, counts0 = pipe.run(Lb, Rb)
    dl, dr, cls, counts, last = pipe.run_post(Lb, Rb)
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
    try:
        pipe.status()
    except SmtError as e:
        assert e.status == SMT_ERR_REF_UB, e                              # as test_pipeline_batch_small_pairs_vs_oracle
    assert torch.equal(dr, dr0) and torch.equal(cls, cls0) and torch.equal(counts, counts0)
    changed = 0
    for b, (L, R) in enumerate(pairs):
        lr = oracle_pipeline(O, L, R, D)
        assert np.array_equal(bits(dl0[b].cpu().numpy()), bits(lr)), b
        sp = O.remove_speckles(lr, 1, 30, INT_MIN)
        changed += int((bits(sp) != bits(lr)).sum())
        assert np.array_equal(bits(dl[b].cpu().numpy()), bits(sp)), b
        assert np.array_equal(bits(last[b].cpu().numpy()), bits(O.median(sp, 3))), b
    assert changed > 0, "the speckle filter changed nothing on these pairs: the test would not see it"
    # lastDisp may be omitted; other post parameters reach the kernels
    dl2, _, _, _, last2 = pipe.run_post(Lb[:2], Rb[:2], speckle_min_area=5, median_wnd=5)
    for b in range(2):
        sp = O.remove_speckles(dl0[b].cpu().numpy(), 1, 5, INT_MIN)
        assert np.array_equal(bits(dl2[b].cpu().numpy()), bits(sp)), b
        assert np.array_equal(bits(last2[b].cpu().numpy()), bits(O.median(sp, 5))), b
    pipe.close()


def test_pipeline_run_post_config3_full_size(smt, O):
    """Config 3 (1920x1080, D=192), 2 pairs: run()'s map is the lr_disp fixture; run_post()'s dispL and lastDisp are
    the oracle's RemoveSpeckles(1, 30, INT_MIN) and 3x3 median of it, bit for bit."""
    from stereo_match_traditional_amd import synth
    rec = json.load(open(GOLD))["cfg3_pipeline_1080p_d192"]
    H, W, D = rec["H"], rec["W"], rec["D"]
    L, R = synth.synth_pair(H, W, D, rec["seed"])
    Lb, Rb = T(np.stack([L, L])), T(np.stack([R, R]))
    pipe = smt.Pipeline(H, W, D, DEV)
    dl0, dr0, cls0, _ = pipe.run(Lb, Rb)
    dl, dr, cls, _, last = pipe.run_post(Lb, Rb)
    pipe.status()
    lr = dl0[0].cpu().numpy()
    assert "%016x" % O.fnv1a(lr) == rec["lr_disp"]
    sp = O.remove_speckles(lr, 1, 30, INT_MIN)
    med = O.median(sp, 3)
    assert int((bits(sp) != bits(lr)).sum()) > 0
    for b in range(2):
        assert np.array_equal(bits(dl[b].cpu().numpy()), bits(sp)), b
        assert np.array_equal(bits(last[b].cpu().numpy()), bits(med)), b
    assert torch.equal(dr, dr0) and torch.equal(cls, cls0)
    pipe.close()
