"""Region voting and outlier interpolation (include/smt_refine.h): the NumPy restatement, one loop per sentence of the
rule, and the case table shared by tests/test_refine_cpu.py and tests/test_refine_gpu.py.  Parity unpinned: the reference
has no code for this step, the header's rule is the definition and this file restates it independently of
csrc/refine_rule.h.  Everything is held bit for bit: every output is an integer or a copy of an input float."""
import functools

import numpy as np

INT_MIN_F = np.float32(-2147483648.0)
INF = np.float32(np.inf)
NAN = np.float32(np.nan)
ARM_CLAMPED = 1
INTERPOLATED, OUTLIER = 254, 255
DIRECT, WAVE = 1, 2
DEFAULTS = dict(irv_ts=20, irv_th=0.4, irv_iters=5, search=0)

RAYS = ((0, 1), (1, 2), (1, 1), (2, 1),
        (1, 0), (2, -1), (1, -1), (1, -2),
        (0, -1), (-1, -2), (-1, -1), (-2, -1),
        (-1, 0), (-2, 1), (-1, 1), (-1, 2))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- Reliable ------------------------------------------------------------------------------------------------------
def reliable(M, D):
    """v >= 0.0f && v < (float)D; false for NaN, +-inf and (float)INT_MIN, true for -0.0f"""
    M = np.asarray(M, np.float32)
    with np.errstate(invalid="ignore"):
        return (M >= np.float32(0.0)) & (M < np.float32(D))


def bin_of(v, D):
    """min(D-1, (int)(v + 0.5f)): one float32 addition, truncation"""
    v = np.asarray(v, np.float32)
    return np.minimum(D - 1, (v + np.float32(0.5)).astype(np.int32))


# ---- Region --------------------------------------------------------------------------------------------------------
def clamp_arms(arms):
    """every length into 0..255 -> (clamped maps, whether any length was clamped)"""
    clamped = any(bool(((a < 0) | (a > 255)).any()) for a in arms)
    return [np.clip(a, 0, 255) for a in arms], clamped


def region_rows(i, j, H, aT, aB):
    return max(0, i - int(aT[i, j])), min(H - 1, i + int(aB[i, j]))


def region_cols(r, j, W, aL, aR):
    return max(0, j - int(aL[r, j])), min(W - 1, j + int(aR[r, j]))


# ---- One voting iteration ------------------------------------------------------------------------------------------
def vote_once(M, arms, D, irv_ts, irv_th):
    """reads M, writes M' -> (M', filled mask)"""
    aL, aR, aT, aB = arms
    H, W = M.shape
    rel = reliable(M, D)
    b = np.where(rel, bin_of(np.where(rel, M, np.float32(0)), D), 0)
    out = M.copy()                                   # a reliable pixel is copied bit for bit; otherwise M'(p) = M(p)
    filled = np.zeros((H, W), bool)
    th = float(np.float32(irv_th))
    for i, j in zip(*np.nonzero(~rel)):
        hist = np.zeros(D, np.int64)
        r0, r1 = region_rows(i, j, H, aT, aB)
        for r in range(r0, r1 + 1):
            c0, c1 = region_cols(r, j, W, aL, aR)
            m = rel[r, c0:c1 + 1]
            hist += np.bincount(b[r, c0:c1 + 1][m], minlength=D)
        S = int(hist.sum())
        d = int(np.argmax(hist))                     # the smallest bin with the largest count
        h = int(hist[d])
        if S > irv_ts and float(h) > th * float(S):
            out[i, j] = np.float32(d)
            filled[i, j] = True
    return out, filled


def vote(M, arms, D, p):
    """-> (map, state, status)"""
    M = np.ascontiguousarray(M, np.float32).copy()
    arms, clamped = clamp_arms(arms)
    rel = reliable(M, D)
    state = np.where(rel, 0, OUTLIER).astype(np.uint8)
    status = np.array([int((~rel).sum()), 0, 0, ARM_CLAMPED if clamped else 0], np.int32)
    for k in range(1, p["irv_iters"] + 1):
        M, filled = vote_once(M, arms, D, p["irv_ts"], p["irv_th"])
        state[filled] = k
        status[1] += int(filled.sum())
    return M, state, status


# ---- Interpolation -------------------------------------------------------------------------------------------------
def interpolate(M, cls, gray, D, p, state=None, status=None):
    """on the map as it stands, for every pixel at once -> (map, state, status)"""
    M = np.ascontiguousarray(M, np.float32)
    H, W = M.shape
    rel = reliable(M, D)
    if state is None:
        state = np.where(rel, 0, OUTLIER).astype(np.uint8)
        status = np.array([int((~rel).sum()), 0, 0, 0], np.int32)
    out = M.copy()
    search = p["search"]
    for i, j in zip(*np.nonzero(~rel)):
        best = None
        for dy, dx in RAYS:
            k, y, x = 1, i + dy, j + dx
            while 0 <= y < H and 0 <= x < W and (search <= 0 or k <= search):
                if rel[y, x]:
                    if cls[i, j] == 1:
                        key = M[y, x]                                   # the smallest value
                    else:
                        key = abs(int(gray[i, j]) - int(gray[y, x]))    # the smallest |gray(p) - gray(q)|
                    if best is None or key < best[0]:                   # ties go to the lower ray index
                        best = (key, y, x)
                    break
                k, y, x = k + 1, y + dy, x + dx
        if best is not None:
            out[i, j] = M[best[1], best[2]]
            state[i, j] = INTERPOLATED
            status[2] += 1
    return out, state, status


def refine(M, arms, cls, gray, D, p):
    M, state, status = vote(M, arms, D, p)
    return interpolate(M, cls, gray, D, p, state, status)


# ---- the case table ------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 70), (7, 1), (9, 33), (17, 65), (37, 130))
DS = (1, 16, 64, 192, 200, 512)
# every size and every D at least once; the largest map with the largest range
TABLE = tuple((f"{H}x{W}-D{D}-s{s}", H, W, D, s) for s, ((H, W), D) in enumerate(
    list(zip(SIZES, DS)) + [((9, 33), 1), ((17, 65), 16), ((37, 130), 64), ((9, 33), 512), ((1, 70), 200), ((17, 65), 192)]))


@functools.lru_cache(maxsize=None)
def _case(H, W, D, seed):
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (0.35 * D + 0.2 * D * np.sin(xx / 9.0 + seed) + 0.1 * D * (yy / max(H, 1))) % max(D, 1)
    M = np.floor(base).astype(np.float32)
    sub = rng.random((H, W)) < 0.2
    M[sub] += rng.random(int(sub.sum())).astype(np.float32)            # sub-pixel values
    M = np.minimum(M, np.float32(D) - np.float32(0.001)).astype(np.float32)
    M[rng.random((H, W)) < 0.05] = rng.integers(0, D, 1)[0]
    hostile = np.array([INF, -INF, NAN, INT_MIN_F, np.float32(D), np.float32(-1.0), np.float32(D + 7), INF, INT_MIN_F], np.float32)
    n = max(1, H * W // 40)
    for _ in range(n):                                                 # blobs of outliers, wide ones included
        i, j = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, 4)), int(rng.integers(1, 9 if rng.random() < 0.8 else 70))
        M[i:i + h, j:j + w] = hostile[rng.integers(0, len(hostile))]
    M[rng.random((H, W)) < 0.03] = np.float32(-0.0)
    arms = []
    for _ in range(4):
        a = rng.integers(0, 7, (H, W)).astype(np.int32)
        big = rng.random((H, W)) < 0.05
        a[big] = rng.integers(17, 80, int(big.sum()))
        arms.append(a)
    cls = rng.integers(0, 3, (H, W)).astype(np.uint8)
    gray = rng.integers(0, 256, (H, W)).astype(np.uint8)
    for a in (M, cls, gray, *arms):
        a.setflags(write=False)
    return M, tuple(arms), cls, gray


def case(H, W, D, seed):
    """-> (map, (aL, aR, aT, aB), cls, gray), read-only, shared"""
    return _case(H, W, D, seed)


TABLE_PARAMS = params(irv_ts=4, irv_th=0.3, irv_iters=3)              # small regions vote too; the defaults: CRAFTED


@functools.lru_cache(maxsize=None)
def table_expected(H, W, D, seed, which):
    """the restatement on a table case under TABLE_PARAMS, computed once: which = vote | interpolate | refine"""
    M, arms, cls, gray = case(H, W, D, seed)
    if which == "vote":
        r = vote(M, arms, D, TABLE_PARAMS)
    elif which == "interpolate":
        r = interpolate(M, cls, gray, D, TABLE_PARAMS)
    else:
        r = refine(M, arms, cls, gray, D, TABLE_PARAMS)
    for a in r:
        a.setflags(write=False)
    return r


def _arms(H, W, L=0, R=0, T=0, B=0):
    return tuple(np.full((H, W), v, np.int32) for v in (L, R, T, B))


def _row(values):
    return np.array([values], np.float32)


def crafted_vote():
    """name -> (map, arms, D, params, check(map', state, status) or None)"""
    c = {}
    D = 16

    def count_case(n_reliable, **kw):
        # 1 x (n + 1): the outlier at column 0 reaches the n reliable 3s to its right
        M = _row([INF] + [3.0] * n_reliable)
        return M, _arms(1, n_reliable + 1, R=n_reliable), D, params(**kw)

    c["S-equals-ts-is-not-filled"] = count_case(20) + ((lambda m, s, t: np.isinf(m[0, 0]) and s[0, 0] == OUTLIER and list(t) == [1, 0, 0, 0]),)
    c["S-ts-plus-one-is-filled"] = count_case(21) + ((lambda m, s, t: m[0, 0] == 3.0 and s[0, 0] == 1 and list(t) == [1, 1, 0, 0]),)

    def share_case(n_a, n_b, a, b, th):
        M = _row([NAN] + [a] * n_a + [b] * n_b)
        return M, _arms(1, n_a + n_b + 1, R=n_a + n_b), D, params(irv_th=th)

    c["h-20-of-40-at-half-is-not-filled"] = share_case(20, 20, 5.0, 2.0, 0.5) + ((lambda m, s, t: np.isnan(m[0, 0]) and t[1] == 0),)
    c["h-21-of-40-at-half-is-filled"] = share_case(21, 19, 5.0, 2.0, 0.5) + ((lambda m, s, t: m[0, 0] == 5.0 and t[1] == 1),)
    c["two-equal-top-bins-give-the-lower"] = share_case(20, 20, 7.0, 4.0, 0.3) + ((lambda m, s, t: m[0, 0] == 4.0),)
    # a chain: every outlier sees itself and its left neighbour; Jacobi fills one per iteration
    M = _row([2.0] + [INT_MIN_F] * 6)
    c["a-chain-fills-one-pixel-per-iteration"] = (M, _arms(1, 7, L=1), D, params(irv_ts=0, irv_iters=3),
                                                  lambda m, s, t: list(s[0]) == [0, 1, 2, 3, 255, 255, 255] and
                                                  list(m[0, :4]) == [2.0] * 4 and (m[0, 4:] == INT_MIN_F).all() and list(t) == [6, 3, 0, 0])
    c["all-outliers"] = (np.full((9, 33), INF, np.float32), _arms(9, 33, 34, 34, 34, 34), D, params(irv_ts=0),
                         lambda m, s, t: np.isinf(m).all() and (s == OUTLIER).all() and list(t) == [297, 0, 0, 0])
    c["all-reliable"] = (np.full((9, 33), 3.25, np.float32), _arms(9, 33, 5, 5, 5, 5), D,
                         params(), lambda m, s, t: (m == np.float32(3.25)).all() and (s == 0).all() and list(t) == [0, 0, 0, 0])
    # values: D - 0.4 votes for bin D - 1, (float)D is an outlier, -0.0f is reliable and votes for 0, 2.5 for 3, 2.49 for 2
    vals = [NAN, np.float32(D - 0.4), np.float32(D - 0.4), np.float32(D - 0.4), np.float32(D), INF, -INF, INT_MIN_F, np.float32(-0.0),
            np.float32(2.5), np.float32(2.49), np.float32(15.0)]
    c["values-top-bin"] = (_row(vals), _arms(1, len(vals), R=len(vals)), D, params(irv_ts=2, irv_th=0.3),
                           lambda m, s, t: m[0, 0] == 15.0 and bits(m[0, 8:9])[0] == 0x80000000 and t[0] == 5)
    vals = [NAN, np.float32(-0.0), np.float32(0.49), np.float32(0.2), np.float32(0.5), np.float32(2.5), np.float32(2.5), np.float32(2.49)]
    c["values-minus-zero-and-halves"] = (_row(vals), _arms(1, len(vals), R=len(vals)), D, params(irv_ts=2, irv_th=0.3),
                                         lambda m, s, t: m[0, 0] == 0.0 and bits(m[0, :1])[0] == 0)
    M = case(9, 33, 16, 2)[0]
    c["no-iterations"] = (M, case(9, 33, 16, 2)[1], D, params(irv_iters=0),
                          lambda m, s, t, M0=M: np.array_equal(bits(m), bits(M0)) and t[1] == 0 and set(np.unique(s)) <= {0, 255})
    # arms
    M = case(9, 33, 64, 3)[0]
    c["arms-all-zero"] = (M, _arms(9, 33), 64, params(irv_ts=0, irv_th=0.0), lambda m, s, t: np.array_equal(bits(m), bits(M)) and t[1] == 0)
    c["arms-34-at-every-border"] = (M, _arms(9, 33, 34, 34, 34, 34), 64, params(), None)
    c["arms-255-the-region-is-the-image"] = (M, _arms(9, 33, 255, 255, 255, 255), 64, params(), None)
    a = list(_arms(9, 33, 300, 300, 300, 300))
    a[0] = a[0].copy(); a[0][::2] = -3
    a[2] = a[2].copy(); a[2][:, ::3] = -3
    c["arms-300-and-minus-3-clamp"] = (M, tuple(a), 64, params(), lambda m, s, t: t[3] == ARM_CLAMPED)
    return c


def crafted_interp():
    """name -> (map, cls, gray, D, params, check(map', state, status) or None)"""
    c = {}
    D = 16
    o = INF
    M = np.array([[7, 2, 9], [4, o, 3], [8, 6, 5]], np.float32)
    flat = np.full((3, 3), 100, np.uint8)
    c["an-occlusion-takes-the-minimum"] = (M, np.full((3, 3), 1, np.uint8), flat, D, params(),
                                           lambda m, s, t: m[1, 1] == 2.0 and s[1, 1] == INTERPOLATED and list(t) == [1, 0, 1, 0])
    gray = np.array([[0, 0, 0], [60, 50, 41], [0, 0, 58]], np.uint8)
    c["a-mismatch-takes-the-nearest-gray"] = (M, np.full((3, 3), 2, np.uint8), gray, D, params(), lambda m, s, t: m[1, 1] == 5.0)
    gray = np.array([[0, 0, 0], [60, 50, 40], [0, 0, 0]], np.uint8)
    c["an-exact-gray-tie-goes-to-the-lower-ray"] = (M, np.zeros((3, 3), np.uint8), gray, D, params(), lambda m, s, t: m[1, 1] == 3.0)
    Mz = np.array([[np.float32(0.0), o, np.float32(-0.0)]], np.float32)
    c["equal-zeros-tie-to-the-lower-ray"] = (Mz, np.ones((1, 3), np.uint8), np.zeros((1, 3), np.uint8), D, params(),
                                             lambda m, s, t: bits(m[0, 1:2])[0] == 0x80000000)      # ray 0 points right
    M2 = np.full((5, 7), o, np.float32)
    M2[3, 5] = 11.0                                                        # (2, 1) + (1, 2)
    c["a-candidate-only-a-step-2-ray-reaches"] = (M2, np.zeros((5, 7), np.uint8), np.zeros((5, 7), np.uint8), D, params(),
                                                  lambda m, s, t: m[2, 3] == 11.0 and np.isinf(m[2, 2]) and m[1, 1] == 11.0)
    M3 = _row([5.0, 6.0, o, o, o, 9.0])
    ones = np.ones((1, 6), np.uint8)
    c["search-1"] = (M3, ones, ones, D, params(search=1), lambda m, s, t: m[0, 2] == 6.0 and np.isinf(m[0, 3]) and m[0, 4] == 9.0)
    c["search-2"] = (M3, ones, ones, D, params(search=2), lambda m, s, t: m[0, 2] == 6.0 and m[0, 3] == 6.0 and m[0, 4] == 9.0)
    c["no-candidate"] = (np.full((4, 5), INT_MIN_F, np.float32), np.ones((4, 5), np.uint8), np.ones((4, 5), np.uint8), D, params(),
                         lambda m, s, t: (m == INT_MIN_F).all() and (s == OUTLIER).all() and list(t) == [20, 0, 0, 0])
    # filled pixels are no candidates: with search = 1 the right outlier sees only the 9
    M4 = _row([5.0, o, o, 9.0])
    c["adjacent-outliers-do-not-feed-each-other"] = (M4, np.ones((1, 4), np.uint8), np.ones((1, 4), np.uint8), D, params(search=1),
                                                     lambda m, s, t: m[0, 1] == 5.0 and m[0, 2] == 9.0)
    return c
