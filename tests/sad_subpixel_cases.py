"""Sub-pixel SAD (include/smt_sad_subpixel.h, csrc/sad_subpixel_rule.h): the case table and a
NumPy restatement that tests/test_sad_subpixel_cpu.py (host twin) and tests/test_sad_subpixel_gpu.py (kernels) share.

The restatement builds the integer SAD rows of both views in int64 -- box sums of |L - R| from summed-area tables, the
chain entries of Sad.h:125-129 (left, d > x) and :167-171 (right, x' + d > W - 1) included --, takes the integer winners
by OptimalDisparity (:40-85) and GetMinSadIndex (:22-38) restated on whole arrays, and applies the rule in np.float32,
one operation per step:
    a parabola exists iff 0 < r < D - 1 (r = 0: the uniqueness test, the ends, D <= 2; r = 65535: nothing below 0xffff);
    s = (c[r-1] + c[r+1]) - 2 c[r]; den = min_den < s ? s : min_den; result = r + (c[r-1] - c[r+1]) / (2 den).
The winners are pinned against oracle.sad by both test files before anything is compared to the floats.

The table (every case runs at every min_den of MIN_DENS, in every comparison):
  planted-d0   right image = texture, left = the texture shifted by d0: cost 0 at d0 only; d0 at 1, the lane boundary
               62..65, the slot boundary 127..129 and D - 2, at D = 192, 12 x 232, 5 x 5
  D<n>         random pairs at D of 1, 2, 3, 60, 64, 65, 128, 130, 200, 257, 512 (every slot instantiation), 5 x 70: W < D
               from 128 on, so the right view's copied tail (w == dmax) and the left chain columns (x < D - 1) are there
  W<w>-H<h>    W of 20 (< D), 63, 64, 65, 130 by H of 1, 2, 7 at D = 64: strip, wave and band edges (the GPU file runs them
               under bands of 1 and 3 rows too)
  win<n>       winsize 0 (3 x 3, the k_sad fallback), 1, 3; win8-sat: 19 x 19 with L all 0 against R all 255, every cost
               19^2 255 > 65535: the 65535.0f case
  tie-*        a pattern of period 4: equal minima -- left 0 by the uniqueness test, right the first"""
import functools

import numpy as np

MIN_DENS = (1.0, 2.0 ** -20, 64.0)
PLANTED_D, PLANTED_SHAPE = 192, (12, 232)
PLANTED = (1, 62, 63, 64, 65, 127, 128, 129, PLANTED_D - 2)
DS = (1, 2, 3, 60, 64, 65, 128, 130, 200, 257, 512)
WS, HS = (20, 63, 64, 65, 130), (1, 2, 7)


def _noise(H, W, seed):
    return np.random.default_rng([23, seed]).integers(0, 256, (H, W)).astype(np.uint8)


def _planted(d0, seed):
    H, W = PLANTED_SHAPE
    R = _noise(H, W, seed)
    L = _noise(H, W, seed + 1000)
    L[:, d0:] = R[:, :W - d0]
    return L, R


def _tie(shift):
    H, W = 4, 48
    R = np.tile(np.array([10, 200, 90, 30], np.uint8), (H, W // 4))
    R = (R + np.arange(H, dtype=np.uint8)[:, None] * 7).astype(np.uint8)     # rows differ, the period stays
    L = np.roll(R, shift, axis=1)
    return L, R


def _cases():
    c = []
    for k, d0 in enumerate(PLANTED):
        c.append((f"planted-{d0}", (lambda d0=d0, k=k: _planted(d0, k)), PLANTED_D, 1))
    for D in DS:
        c.append((f"D{D}", (lambda D=D: (_noise(5, 70, D), _noise(5, 70, D + 5000))), D, 1))
    for W in WS:
        for H in HS:
            c.append((f"W{W}-H{H}", (lambda H=H, W=W: (_noise(H, W, 31 * W + H), _noise(H, W, 37 * W + H))), 64, 1))
    for ws in (0, 1, 3):
        c.append((f"win{ws}", (lambda ws=ws: (_noise(6, 40, 70 + ws), _noise(6, 40, 80 + ws))), 16, ws))
    c.append(("win8-sat", lambda: (np.zeros((6, 40), np.uint8), np.full((6, 40), 255, np.uint8)), 16, 8))
    c.append(("tie-0", lambda: _tie(0), 16, 1))
    c.append(("tie-2", lambda: _tie(2), 16, 1))
    return c


CASES = _cases()
NAMES = [c[0] for c in CASES]
_BY_NAME = {c[0]: c for c in CASES}
BAND_CASES = [n for n in NAMES if n.startswith("W")]


def pad_replicate(img, w):
    return np.pad(img, w, mode="edge")


@functools.lru_cache(maxsize=None)
def pair(name):
    """-> (Lp, Rp, D, winsize): the padded images of the case, read-only"""
    _, make, D, ws = _BY_NAME[name]
    L, R = make()
    Lp, Rp = pad_replicate(L, ws + 1), pad_replicate(R, ws + 1)
    Lp.setflags(write=False); Rp.setflags(write=False)
    return Lp, Rp, D, ws


def sad_rows(Lp, Rp, D, ws):
    """-> (rowsL, rowsR) int64 [H][W][D]: the `sad` vectors of GetPointDepthLeft / Right, chain entries included.  The last
    row and column of the right view hold rows too; the caller zeroes their results (Sad.h:157, :160)."""
    w = ws + 1
    side = 2 * w + 1
    Hp, Wp = Lp.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    A, B = Lp.astype(np.int64), Rp.astype(np.int64)
    rowsL = np.zeros((H, W, D), np.int64)
    rowsR = np.zeros((H, W, D), np.int64)
    for d in range(D):
        if d > W - 1:                                          # no pixel of either view evaluates d: chains only
            rowsL[:, :, d] = rowsL[:, :, d - 1]
            rowsR[:, :, d] = rowsR[:, :, d - 1]
            continue
        ad = np.abs(A[:, d:] - B[:, :Wp - d])                  # ad[y][j] = |Lp[y][j + d] - Rp[y][j]|
        S = np.zeros((Hp + 1, ad.shape[1] + 1), np.int64)
        S[1:, 1:] = ad.cumsum(0).cumsum(1)
        box = S[side:, side:] - S[:-side, side:] - S[side:, :-side] + S[:-side, :-side]   # [H][W - d]: window at (i, j)
        assert box.shape == (H, W - d)
        rowsL[:, d:, d] = box                                  # left pixel x = j + d
        rowsR[:, :W - d, d] = box                              # right pixel x' = j
        if d:
            rowsL[:, :d, d] = rowsL[:, :d, d - 1]              # Sad.h:125-129
            rowsR[:, W - d:, d] = rowsR[:, W - d:, d - 1]      # :167-171
    return rowsL, rowsR


def optimal_disparity(rows):
    """OptimalDisparity (Sad.h:40-85) on [..][D] float32 rows -> int32"""
    D = rows.shape[-1]
    f = rows.astype(np.float32)
    top = np.float32(65535)
    if D > 1:
        tail = f[..., 1:]
        minv = np.minimum(tail.min(-1), top)
        first = 1 + np.argmax(tail == minv[..., None], -1)     # the first d >= 1 that reaches the minimum
        best = np.where(tail.min(-1) < top, first, 65535)
    else:
        minv = np.full(f.shape[:-1], top)
        best = np.full(f.shape[:-1], 65535)
    other = np.where(f == minv[..., None], np.float32(np.inf), f)
    sec = np.minimum(f[..., 0], other.min(-1))
    out = np.where((sec - minv).astype(np.float64) <= 0.01, 0, best)
    out = np.where((best == 0) | (best == D - 1), 0, out)
    return out.astype(np.int32)


def rule(rows, r, min_den):
    """the parabola on integer rows [..][D] at the integer results r, np.float32, one operation per step"""
    D = rows.shape[-1]
    f = rows.astype(np.float32)
    assert np.array_equal(f.astype(np.int64), rows)            # below 2^24: the floats are the integers
    fr = r.astype(np.float32)
    if D < 3:
        return fr
    para = (r > 0) & (r < D - 1)
    ri = np.clip(r.astype(np.int64), 1, D - 2)
    take = lambda idx: np.take_along_axis(f, idx[..., None], axis=-1)[..., 0]
    c1, cm, c2 = take(ri - 1), take(ri), take(ri + 1)
    two, md = np.float32(2), np.float32(min_den)
    s = (c1 + c2) - two * cm
    den = np.where(md < s, s, md).astype(np.float32)
    off = (c1 - c2) / (two * den)
    res = fr + off
    assert s.dtype == den.dtype == off.dtype == res.dtype == np.float32 and np.isfinite(off).all()
    return np.where(para, res, fr).astype(np.float32)


@functools.lru_cache(maxsize=None)
def winners(name):
    """-> (rowsL, rowsR, winL, winR): the rows and the integer maps of the restatement"""
    Lp, Rp, D, ws = pair(name)
    rowsL, rowsR = sad_rows(Lp, Rp, D, ws)
    winL = optimal_disparity(rowsL)
    winR = np.argmin(rowsR, -1).astype(np.int32)               # GetMinSadIndex: the first strict minimum
    winR[-1, :] = 0
    winR[:, -1] = 0
    for a in (rowsL, rowsR, winL, winR):
        a.setflags(write=False)
    return rowsL, rowsR, winL, winR


@functools.lru_cache(maxsize=None)
def restate(name, min_den):
    """-> (dispL, dispR, winL, winR): float32, float32, int32, int32 [H][W], read-only"""
    rowsL, rowsR, winL, winR = winners(name)
    dl = rule(rowsL, winL, min_den)
    dr = rule(rowsR, winR, min_den)
    dr[-1, :] = 0
    dr[:, -1] = 0
    dl.setflags(write=False); dr.setflags(write=False)
    return dl, dr, winL, winR


def crosscheck(winL, winR, dispL):
    """CrossCheckDiaparity (Sad.h:184-222) on the integer winners -> (lastdisp float32: dispL or +inf, cls uint8)"""
    H, W = winL.shape
    n = H * W
    lv = winL.reshape(-1).astype(np.int64)
    idx = np.arange(n) - lv                                    # flat pointer arithmetic, :204
    rv = np.where((idx >= 0) & (idx < n), winR.reshape(-1)[np.clip(idx, 0, n - 1)], 0).astype(np.int64)
    bad = np.abs(lv - rv) > 5
    cls = np.where(bad, np.where(lv < rv, 1, 2), 0).astype(np.uint8).reshape(H, W)
    last = np.where(bad.reshape(H, W), np.float32(np.inf), dispL).astype(np.float32)
    return last, cls


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
