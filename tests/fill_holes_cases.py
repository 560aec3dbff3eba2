"""FillHolesInDispMap (SAD/Sad.h:317-400) restated loop for loop in NumPy float32, and the cases of
test_fill_holes_cpu.py and test_fill_holes_gpu.py.  A plain helper module.

The restatement keeps the reference's structure: the pass loop k = 0, 1, 2, the target lists in list order, the third
pass's scan, `angle = angle2` from the first target in row height / 2 on, the eight rays one after the other, the walk
n = 1, 2, ... with `(int)((float)y + (float)n * sina)`, std::sort, and the choice by pass.  The float32 sums of the walk
are read from tables built with the same two float32 operations for every (coordinate, n) at once; nothing else is
vectorised.  sina and cosa are math.sin / math.cos of the float32 angle rounded to float32 (the correctly rounded value,
which is what glibc's sinf / cosf return for these sixteen arguments; test_fill_holes_cpu.py holds the three sources to
each other).  The two corners the header decides: a collected -0.0f is +0.0f, and a map with a NaN is left alone and
flagged."""
import math

import numpy as np

F = np.float32
INF = float("inf")
INT_MIN_F = float(np.float32(-2 ** 31))
UB_NAN = 1
MAX_DIM = 8192

PI = F(3.1415926)
ANGLE1 = [PI, F(3) * PI / F(4), PI / F(2), PI / F(4), F(0), F(7) * PI / F(4), F(3) * PI / F(2), F(5) * PI / F(4)]
ANGLE2 = [PI, F(5) * PI / F(4), F(3) * PI / F(2), F(7) * PI / F(4), F(0), PI / F(4), PI / F(2), F(3) * PI / F(4)]
assert all(type(a) is np.float32 for a in ANGLE1 + ANGLE2)


def sin_cos(angle):
    return F(math.sin(float(angle))), F(math.cos(float(angle)))


def constants():
    """the sixteen constants in the order of smt_fill_holes_constants: sina of angle1[0..7], then cosa"""
    sc = [sin_cos(a) for a in ANGLE1]
    return np.array([s for s, _ in sc] + [c for _, c in sc], F)


_TABLES = {}


def _walk_table(extent, direction, nmax):
    """T[at][n] = (int)((float)at + (float)n * direction) for at = 0..extent-1, n = 0..nmax-1: float32 product, float32
    sum, truncation toward zero"""
    key = (extent, float(direction), nmax)
    if key not in _TABLES:
        prod = np.arange(nmax, dtype=np.int32).astype(F) * F(direction)
        t = np.arange(extent, dtype=np.int32).astype(F)[:, None] + prod[None, :]
        assert prod.dtype == F and t.dtype == F
        _TABLES[key] = np.trunc(t).astype(np.int32)
    return _TABLES[key]


def probe(at, n, direction):
    """(int)((float)at + (float)n * direction), scalar"""
    return int(np.trunc(F(at) + F(n) * F(direction)))


def lists_of(cls):
    """the (row, col) lists of class 1 and class 2, in raster order, as LeftRightConsistency produces them"""
    occ = [(int(y), int(x)) for y, x in np.argwhere(cls == 1)]
    mis = [(int(y), int(x)) for y, x in np.argwhere(cls == 2)]
    return occ, mis


def fill_holes_lists(M, occlusion, mismatch, invalid=INF, use_angle2=True, collect_then_write=False):
    """Sad.h:317-400 on a copy of M with the two lists -> (maps after pass 0, 1, 2, number of third-pass targets).
    use_angle2=False never switches to angle2 (the test that it is immaterial); collect_then_write=True is NOT the
    reference: every pass reads the map as it was when the pass started (the form the 1 x 9 case tells apart)."""
    M = np.array(M, F)
    height, width = M.shape
    invalid = F(invalid)
    occlusion, mismatch = list(occlusion), list(mismatch)                  # by value
    angle = ANGLE1
    nmax = int(1.5 * max(height, width)) + 4                               # every ray has left the image by then
    after = []
    n_third = 0
    for k in range(3):
        trg_pixels = occlusion if k == 0 else mismatch
        if k == 2:
            inv_pixels = []
            for i in range(height):
                for j in range(width):
                    if M[i, j] == invalid:
                        inv_pixels.append((i, j))
            trg_pixels = inv_pixels
            n_third = len(inv_pixels)
        src = M.copy() if collect_then_write else M
        for (y, x) in trg_pixels:
            if y == height // 2 and use_angle2:
                angle = ANGLE2
            disp_collects = []
            for ray in range(8):
                sina, cosa = sin_cos(angle[ray])
                ty, tx = _walk_table(height, sina, nmax), _walk_table(width, cosa, nmax)
                n = 1
                while True:
                    yy, xx = int(ty[y, n]), int(tx[x, n])
                    if yy < 0 or yy >= height or xx < 0 or xx >= width:
                        break
                    disp = src[yy, xx]
                    if disp != invalid:
                        disp_collects.append(disp + F(0.0))                # -0.0f counts and is +0.0f
                        break
                    n += 1
            if not disp_collects:
                continue
            disp_collects.sort()
            if k == 0:
                M[y, x] = disp_collects[1] if len(disp_collects) > 1 else disp_collects[0]
            else:
                M[y, x] = disp_collects[len(disp_collects) // 2]
        after.append(M.copy())
    return after, n_third


def collected(M, y, x, invalid=INF):
    """the values the eight rays of (y, x) collect on M as it stands, in ray order"""
    M = np.asarray(M, F)
    out = []
    for ray in range(8):
        sina, cosa = sin_cos(ANGLE1[ray])
        n = 1
        while True:
            yy, xx = probe(y, n, sina), probe(x, n, cosa)
            if yy < 0 or yy >= M.shape[0] or xx < 0 or xx >= M.shape[1]:
                break
            if M[yy, xx] != F(invalid):
                out.append(M[yy, xx])
                break
            n += 1
    return out


def fill_holes(M, cls, invalid=INF, **kw):
    """the entry points' contract on one map -> (maps after pass 0, 1, 2; status int32 [4])"""
    M = np.array(M, F)
    occ, mis = lists_of(cls)
    if np.isnan(M).any():
        return [M.copy(), M.copy(), M.copy()], np.array([len(occ), len(mis), 0, UB_NAN], np.int32)
    after, n_third = fill_holes_lists(M, occ, mis, invalid, **kw)
    return after, np.array([len(occ), len(mis), n_third, 0], np.int32)


_EXPECTED = {}


def expected(key, M, cls, invalid=INF):
    """fill_holes computed once per key and handed out read-only"""
    if key not in _EXPECTED:
        after, st = fill_holes(M, cls, invalid)
        for a in after + [st]:
            a.setflags(write=False)
        _EXPECTED[key] = (after, st)
    return _EXPECTED[key]


# ---- the case table --------------------------------------------------------------------------------------------------
# 1030 x 9 has more rows than a workgroup has threads; 9 x 33, 17 x 65 and 37 x 130 are odd, not multiples of a wave and
# give the kernel 64, 64 and 128 threads; 1 x 70 and 7 x 1 have no second axis
TABLE = [("1x1", 1, 1, 1), ("1x70", 1, 70, 2), ("7x1", 7, 1, 3), ("9x33", 9, 33, 4), ("17x65", 17, 65, 5),
         ("37x130", 37, 130, 6), ("1030x9", 1030, 9, 7)]


def case(H, W, seed, invalid=INF, density=0.3, neg_zero=True):
    """a random map with holes (single pixels and a few blobs), a class map that lists most holes as occlusion or
    mismatch, leaves some to the third pass and lists a few valid pixels, and some -0.0f values"""
    rng = np.random.default_rng(1000 + seed)
    M = rng.integers(0, 64, (H, W)).astype(F)
    frac = rng.random((H, W)) < 0.2
    M[frac] += rng.integers(1, 8, int(frac.sum())).astype(F) / F(8)
    M[rng.random((H, W)) < 0.03] = F(-0.0) if neg_zero else F(0.0)
    if float(invalid) == 0.0:
        M[M == 0] = F(1.0)                                                 # zeros would be holes
    hole = rng.random((H, W)) < density
    for _ in range(3):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        hole[y:y + int(rng.integers(1, 7)), x:x + int(rng.integers(1, 9))] = True
    M[hole] = F(invalid)
    cls = np.zeros((H, W), np.uint8)
    pick = rng.random((H, W))
    cls[hole & (pick < 0.45)] = 1
    cls[hole & (pick >= 0.45) & (pick < 0.9)] = 2
    listed_valid = ~hole & (rng.random((H, W)) < 0.04)
    cls[listed_valid] = rng.integers(1, 3, int(listed_valid.sum())).astype(np.uint8)
    cls[~hole & ~listed_valid & (rng.random((H, W)) < 0.05)] = 3           # another class value: not a target
    return M, cls


def table_case(gid):
    _, H, W, seed = next(t for t in TABLE if t[0] == gid)
    return case(H, W, seed)


def table_expected(gid):
    M, cls = table_case(gid)
    return expected(("table", gid), M, cls)


def _ramp(H, W):
    return (np.arange(H * W, dtype=np.int64).reshape(H, W) % 61 + 1).astype(F)


def crafted():
    """name -> (M, cls, invalid, check(after, status) or None)"""
    out = {}
    # a 1 x 9 run of holes between 3 and 7: each takes its left neighbour's fresh fill, which the left ray and the two
    # left staircase rays all see ({3, 3, 3, 7}, element 2 = 3); reading the map as it was, a hole whose left neighbour is
    # a hole collects {3, 7} and takes 7
    M = np.full((1, 9), INF, F); M[0, 0] = 3; M[0, 8] = 7
    cls = np.full((1, 9), 2, np.uint8); cls[0, 0] = cls[0, 8] = 0
    out["run_1x9"] = (M, cls, INF, lambda a, s: bool((a[1][0, :8] == 3).all()))
    # a solid blob wider and taller than 64
    M = _ramp(80, 90); M[5:75, 8:84] = INF
    cls = np.zeros((80, 90), np.uint8); cls[5:75, 8:84] = 1; cls[20:60, 30:70] = 2; cls[30:40, 40:50] = 0
    out["blob_70x76"] = (M, cls, INF, lambda a, s: bool(np.isfinite(a[2]).all()))
    # a hole on every border pixel and corner (the self-visit at row 0 and column 0)
    M = _ramp(11, 13); cls = np.zeros((11, 13), np.uint8)
    for sl, c in (((0, slice(None)), 1), ((10, slice(None)), 2), ((slice(None), 0), 2), ((slice(None), 12), 1)):
        M[sl] = INF; cls[sl] = c
    out["borders"] = (M, cls, INF, None)
    # listed pixels that are valid, on the top row and left column too: they can collect themselves
    M = _ramp(6, 7); cls = np.zeros((6, 7), np.uint8)
    cls[0, 3] = 1; cls[3, 0] = 2; cls[2, 2] = 1; cls[4, 5] = 2; cls[0, 0] = 2
    out["listed_valid"] = (M, cls, INF, lambda a, s: int(s[2]) == 0)
    # an occlusion that collects exactly one value, and exactly two (element 1, the larger)
    M = np.array([[INF, 7]], F)
    assert len(collected(M, 0, 0)) == 1
    out["occ_one_value"] = (M, np.array([[1, 0]], np.uint8), INF, lambda a, s: a[0][0, 0] == 7)
    M = np.array([[INF, 7], [9, INF]], F)
    assert sorted(collected(M, 0, 0)) == [7, 9]
    out["occ_two_values"] = (M, np.array([[1, 0], [0, 0]], np.uint8), INF, lambda a, s: a[0][0, 0] == 9)
    # mismatches with an even count: two values, element 1; four values {3, 3, 3, 7} (the staircase rays of a one-row
    # map reach the left neighbour too), element 2
    out["mis_two_values"] = (M, np.array([[2, 0], [0, 0]], np.uint8), INF, lambda a, s: a[1][0, 0] == 9)
    M = np.array([[3, INF, 7]], F)
    assert sorted(collected(M, 0, 1)) == [3, 3, 3, 7]
    out["mis_four_values"] = (M, np.array([[0, 2, 0]], np.uint8), INF, lambda a, s: a[1][0, 1] == 3)
    # all holes: nothing changes
    out["all_holes"] = (np.full((5, 6), INF, F), np.full((5, 6), 1, np.uint8), INF,
                        lambda a, s: bool(np.isinf(a[2]).all()) and int(s[2]) == 30)
    # a mismatch whose only valid neighbour is an occlusion filled in pass 0 and read in pass 1
    M = np.array([[4, INF, INF]], F); cls = np.array([[0, 1, 2]], np.uint8)
    out["pass0_feeds_pass1"] = (M, cls, INF, lambda a, s: np.isinf(a[0][0, 2]) and a[1][0, 2] == 4)
    # -0.0f: collected, written as +0.0f
    M = np.array([[F(-0.0), INF, F(-0.0)], [INF, INF, INF]], F); cls = np.array([[0, 2, 0], [0, 0, 0]], np.uint8)
    out["negative_zero"] = (M, cls, INF, lambda a, s: not np.signbit(a[1][0, 1]) and a[1][0, 1] == 0)
    # the other invalid values
    for name, inv in (("invalid_int_min", INT_MIN_F), ("invalid_zero", 0.0)):
        m, c = case(9, 33, 40, invalid=inv)
        out[name] = (m, c, inv, None)
    # with invalid = 0 an infinity is a value like any other
    M = np.array([[0, INF, 0, 3]], F); cls = np.array([[2, 0, 1, 0]], np.uint8)
    out["invalid_zero_inf_is_a_value"] = (M, cls, 0.0, lambda a, s: np.isinf(a[2][0, 0]))
    return out


def nan_pair():
    """a NaN map beside a clean one -> (maps [2][H][W], cls [2][H][W])"""
    M, cls = case(9, 33, 41)
    bad = M.copy(); bad[4, 17] = np.nan
    return np.stack([bad, M]), np.stack([cls, cls])


ERR_ARG = -1
