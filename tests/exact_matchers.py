"""Shared by test_exact_matchers_cpu.py, test_exact_matchers_gpu.py and the tightened assertions of the older GPU tests:
NCC (NCC.h:15-95) and ASW (ASW.h:193-257, 329-431) restated as exact rational functions of the bytes and of the given
float64 table entries, evaluated in np.longdouble (64-bit significand) independently of the oracle's C; a checker in
fractions.Fraction for the longdouble values; the two WinTakeAll rules applied to a cost volume; the error bounds, which are
derived from the arithmetic and not measured; the case lists and their input builders.

Bounds (u = 2^-53, n = taps of the window):
  * NCC, integer-sum form (k_ncc_stats + k_ncc2): numerator and both radicands are exact integers below 2^53; two roots,
    one product and one quotient are four roundings of at most u each; the bound is that doubled: 2^-50 |exact|.
  * NCC, loop nest (k_ncc, the oracle): three length-n float64 sums of products of mean-subtracted bytes, |cost| <= 1:
    first order 2 n u, doubled: 4 n u absolute.
  * ASW, every formulation: all summands are non-negative (no cancellation), so the float64 quotient is within ~2 n u
    relative, doubled; then one narrowing to float32: ulp_f32(exact) / 2 + 4 n u |exact|.
"""
import functools
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, (
    f"np.longdouble has a {np.finfo(LD).nmant}-bit significand here; the exact references need 63 bits or more")

U53 = LD(2.0) ** -53


# ------------------------------------------------------------------------------------------------------------ NCC
def _box(a, win):
    """window sums of side 2 win + 1 over the last two axes (integers, exact) -> [..., H - 2 win, W - 2 win]"""
    side = 2 * win + 1
    s = np.zeros(a.shape[:-2] + (a.shape[-2] + 1, a.shape[-1] + 1), np.int64)
    s[..., 1:, 1:] = a.cumsum(-2).cumsum(-1)
    return s[..., side:, side:] - s[..., :-side, side:] - s[..., side:, :-side] + s[..., :-side, :-side]


def ncc_sums(L, R, D, win):
    """The integers of NCC.h:15-49 per interior pixel and hypothesis, [Hi][Wi][D] int64 (Hi = H - 2 win, Wi = W - 2 win):
    A = n Saa - Sa^2, B = n Sbb - Sb^2, num = n Sab - Sa Sb, and the sentinel mask j - win - d < 0.  Entries under the
    sentinel mask are meaningless."""
    L = np.asarray(L).astype(np.int64)
    R = np.asarray(R).astype(np.int64)
    H, W = L.shape
    n = (2 * win + 1) ** 2
    Hi, Wi = H - 2 * win, W - 2 * win
    assert Hi > 0 and Wi > 0
    Sa, Saa, Sb, Sbb = _box(L, win), _box(L * L, win), _box(R, win), _box(R * R, win)
    d = np.arange(D)
    x = np.arange(W)[None, :] - d[:, None]                                 # [D][W]: column of R under column x of L
    Rs = np.where(x >= 0, R[:, np.clip(x, 0, W - 1)], 0)                   # [H][D][W]
    Sab = _box((L[:, None, :] * Rs).transpose(1, 0, 2), win).transpose(1, 2, 0)          # [Hi][Wi][D]
    jm = np.arange(Wi)[:, None] - d[None, :]                               # interior column index of the right window
    sentinel = np.broadcast_to(jm < 0, (Hi, Wi, D)).copy()
    jc = np.clip(jm, 0, Wi - 1)
    A = np.broadcast_to((n * Saa - Sa * Sa)[:, :, None], (Hi, Wi, D))
    Bp = n * Sbb - Sb * Sb
    B = Bp[:, jc]
    num = n * Sab - Sa[:, :, None] * Sb[:, jc]
    assert max(int(np.abs(num).max()), int(A.max()), int(B.max())) < 2 ** 53
    return A, B, num, sentinel


def ncc_exact(L, R, D, win):
    """-> (exact, flat, sentinel), each [H][W][D]: exact = num / (sqrt(A) sqrt(B)) in longdouble where the hypothesis is
    valid and not flat (NaN elsewhere); flat = A B == 0 on valid hypotheses (the reference's 0/0); sentinel =
    j - win - d < 0 on interior pixels (the cost is exactly 255.0).  Border pixels: NaN, False, False."""
    H, W = np.asarray(L).shape
    A, B, num, sent = ncc_sums(L, R, D, win)
    fl = ((A == 0) | (B == 0)) & ~sent
    ok = ~fl & ~sent
    ex = np.full(A.shape, np.nan, LD)
    ex[ok] = num[ok].astype(LD) / (np.sqrt(A[ok].astype(LD)) * np.sqrt(B[ok].astype(LD)))
    exact = np.full((H, W, D), np.nan, LD)
    flat = np.zeros((H, W, D), bool)
    sentinel = np.zeros((H, W, D), bool)
    inner = (slice(win, H - win), slice(win, W - win))
    exact[inner], flat[inner], sentinel[inner] = ex, fl, sent
    return exact, flat, sentinel


def ncc_wta(cost, win):
    """NCC.h:53-67 on a float64 [H][W][D] volume: best = 0, m = (float)c[0]; d >= 1 wins where (double)m < c[d], and then
    m = (float)c[d].  NaN as IEEE comparison makes it; border pixels 0."""
    cost = np.asarray(cost, np.float64)
    H, W, D = cost.shape
    best = np.zeros((H, W), np.int32)
    with np.errstate(invalid="ignore"):
        m = cost[..., 0].astype(np.float32)
        for d in range(1, D):
            c = cost[..., d]
            upd = m.astype(np.float64) < c
            best[upd] = d
            m[upd] = c[upd].astype(np.float32)
    inner = np.zeros((H, W), bool)
    inner[win:H - win, win:W - win] = True
    best[~inner] = 0
    return best


# ------------------------------------------------------------------------------------------------------------ ASW
def _asw_windows(img, side):
    return np.lib.stride_tricks.sliding_window_view(np.asarray(img).astype(np.int64), (side, side))


def asw_taps(Lp, Rp, D, winSize, space, color, T, view, dtype):
    """The hypotheses of ASW.h:329-431, one d at a time: yields (d, jl, m2, e) with jl the columns whose dmax >= 0, m2 =
    (color space)(color space) [H][len(jl)][taps] in `dtype` (products in the reference's order) and e = min(|a - b|, T)
    as int64.  Padded images (by wins = winSize + 1); dd = min(d, dmax) with dmax = j (left view, 0) or W - wins - 2 - j
    (right view, 1)."""
    wins = winSize + 1
    side = 2 * wins + 1
    Hp, Wp = np.asarray(Lp).shape
    H, W = Hp - 2 * wins, Wp - 2 * wins
    sp = np.asarray(space, np.float64).reshape(-1).astype(dtype)
    cm = np.asarray(color, np.float64).astype(dtype)
    A, B = (Lp, Rp) if view == 0 else (Rp, Lp)
    wa = _asw_windows(A, side)[:H, :W].reshape(H, W, side * side)          # windows by their first padded column
    wb = _asw_windows(B, side)[:H, :W].reshape(H, W, side * side)
    ctr = wins * side + wins
    w0 = cm[np.abs(wa - wa[..., ctr:ctr + 1])] * sp
    w1 = cm[np.abs(wb - wb[..., ctr:ctr + 1])] * sp
    j = np.arange(W)
    dmax = j if view == 0 else W - wins - 2 - j
    jl = j[dmax >= 0]
    if not len(jl):
        return
    for d in range(D):
        dd = np.minimum(d, dmax[jl])
        x0 = jl - dd if view == 0 else jl + dd
        yield d, jl, w0[:, jl] * w1[:, x0], np.minimum(np.abs(wa[:, jl] - wb[:, x0]), T)


def asw_volume(Lp, Rp, D, winSize, space, color, T, view, dtype, quotient):
    """[H][W][D] volume of quotient(m2, e) over asw_taps in `dtype`; NaN where dmax < 0"""
    wins = winSize + 1
    Hp, Wp = np.asarray(Lp).shape
    out = None
    for d, jl, m2, e in asw_taps(Lp, Rp, D, winSize, space, color, T, view, dtype):
        q = quotient(m2, e)
        if out is None:
            out = np.full((Hp - 2 * wins, Wp - 2 * wins, D), np.nan, q.dtype)
        out[:, jl, d] = q
    return out if out is not None else np.full((Hp - 2 * wins, Wp - 2 * wins, D), np.nan, np.float32)


def asw_exact(Lp, Rp, D, winSize, space, color, T, view):
    """ASW.h:210-257 -> exact [H][W][D] longdouble: sum(m2 e) / sum(m2) with the tables and all products and sums in
    longdouble; dmax < 0: every cost NaN."""
    return asw_volume(Lp, Rp, D, winSize, space, color, T, view, LD,
                      lambda m2, e: (m2 * e.astype(LD)).sum(-1) / m2.sum(-1)).astype(LD)


def asw_nan_mask(H, W, D, winSize, view):
    """the dmax rule: right-view pixels with W - wins - 2 - j < 0 hold NaN for every d"""
    m = np.zeros((H, W, D), bool)
    if view == 1:
        m[:, np.arange(W) > W - (winSize + 1) - 2] = True
    return m


def asw_wta(cost):
    """ASW.h:193-208 on a float32 [H][W][D] volume: first strict minimum; all NaN -> 0.  -> float32 [H][W]"""
    cost = np.asarray(cost, np.float32)
    mv = cost[..., 0].copy()
    best = np.zeros(cost.shape[:2], np.float32)
    with np.errstate(invalid="ignore"):
        for d in range(1, cost.shape[2]):
            upd = mv > cost[..., d]
            best[upd] = d
            mv[upd] = cost[..., d][upd]
    return best


# ------------------------------------------------------------------------------------------------------------ Fraction
def ld_fraction(v):
    """an np.longdouble as an exact Fraction (two float64 pieces hold a 64-bit significand)"""
    v = LD(v)
    hi = float(v)
    lo = float(v - LD(hi))
    assert LD(hi) + LD(lo) == v
    return Fraction(hi) + Fraction(lo)


def ncc_fraction(L, R, i, j, d, win):
    """num / sqrt(A B) for one valid hypothesis, from plain Python integers; the root to 40 digits"""
    L = np.asarray(L); R = np.asarray(R)
    a = [int(v) for v in L[i - win:i + win + 1, j - win:j + win + 1].reshape(-1)]
    b = [int(v) for v in R[i - win:i + win + 1, j - win - d:j + win - d + 1].reshape(-1)]
    n = len(a)
    A = n * sum(v * v for v in a) - sum(a) ** 2
    B = n * sum(v * v for v in b) - sum(b) ** 2
    num = n * sum(x * y for x, y in zip(a, b)) - sum(a) * sum(b)
    scale = 10 ** 40
    return Fraction(num * scale, math.isqrt(A * B * scale * scale))


def asw_fraction(Lp, Rp, i, j, d, winSize, space, color, T, view):
    """one hypothesis with dmax >= 0 in exact rational arithmetic: the table entries are float64, hence dyadic rationals
    m / 2^k, and both sums are taken as integers over the common denominator"""
    wins = winSize + 1
    side = 2 * wins + 1
    W = np.asarray(Lp).shape[1] - 2 * wins
    A, B = (Lp, Rp) if view == 0 else (Rp, Lp)
    dmax = j if view == 0 else W - wins - 2 - j
    assert dmax >= 0
    dd = min(d, dmax)
    x0 = j - dd if view == 0 else j + dd
    a = np.asarray(A)[i:i + side, j:j + side].astype(int)
    b = np.asarray(B)[i:i + side, x0:x0 + side].astype(int)
    sp = [float(v).as_integer_ratio() for v in np.asarray(space, np.float64).reshape(-1)]
    cm = [float(v).as_integer_ratio() for v in np.asarray(color, np.float64)]
    taps = []
    for r in range(side):
        for c in range(side):
            sn, sd = sp[r * side + c]
            an, ad = cm[abs(int(a[r, c]) - int(a[wins, wins]))]
            bn, bd = cm[abs(int(b[r, c]) - int(b[wins, wins]))]
            taps.append((an * sn * bn * sn, (ad * sd * bd * sd).bit_length() - 1, min(abs(int(a[r, c]) - int(b[r, c])), T)))
    kmax = max(k for _, k, _ in taps)
    sw = sum(m << (kmax - k) for m, k, _ in taps)
    sv = sum((m * e) << (kmax - k) for m, k, e in taps)
    return Fraction(sv, sw)


def fraction_rel_err(value, frac):
    """|value - frac| / |frac| as a float (0 where both are 0)"""
    v = ld_fraction(value)
    if frac == 0:
        return 0.0 if v == 0 else math.inf
    return float(abs(v - frac) / abs(frac))


# ------------------------------------------------------------------------------------------------------------ bounds
def ncc_bound_int(exact):
    """integer-sum form: 2^-50 |exact| (and exact == 0 => got == 0)"""
    return np.abs(np.asarray(exact, LD)) * LD(2.0) ** -50


def ncc_bound_loop(win):
    """loop nest and oracle: 4 n 2^-53, absolute"""
    return LD(4 * (2 * win + 1) ** 2) * U53


def ulp_f32(x):
    """float32 spacing of the binade that holds |x| (x longdouble; the smallest subnormal below 2^-126)"""
    _, e = np.frexp(np.abs(np.asarray(x, LD)))                             # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(LD(1.0), np.maximum(e - 24, -149))


def asw_bound(exact, winSize):
    """ulp_f32(exact) / 2 + 4 n 2^-53 |exact|, n = (2 winSize + 3)^2 (and exact == 0 => got == +0)"""
    exact = np.asarray(exact, LD)
    n = (2 * winSize + 3) ** 2
    return ulp_f32(exact) / 2 + LD(4 * n) * U53 * np.abs(exact)


def ncc_pair_bound(win):
    """two loop-nest evaluations against each other (a kernel and the oracle): 8 n 2^-53"""
    return float(2 * ncc_bound_loop(win))


def ncc_forms_bound(win):
    """the loop nest against the integer-sum form: 4 n 2^-53 + 2^-50 (|cost| <= 1)"""
    return float(ncc_bound_loop(win) + LD(2.0) ** -50)


def units(err, bound):
    """largest err / bound over the entries with bound > 0 (0.0 when there is none)"""
    err, bound = np.asarray(err, LD), np.broadcast_to(np.asarray(bound, LD), np.shape(err))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max(initial=LD(0)))


def check_ncc(got, exact, flat, sentinel, win, form):
    """The assertions of one NCC cost volume against the exact reference; form "int" (2^-50 |exact|) or "loop"
    (4 n 2^-53).  -> largest error in units of the bound."""
    got = np.asarray(got, np.float64)
    H, W, D = got.shape
    inner = np.zeros((H, W, 1), bool)
    inner[win:H - win, win:W - win] = True
    valid = inner & ~sentinel
    assert np.array_equal(np.isnan(got) & valid, flat), "NaN pattern != {A B == 0}"
    assert (got[sentinel] == 255.0).all(), "sentinel hypotheses must cost exactly 255.0"
    rest = valid & ~flat
    err = np.abs(got[rest].astype(LD) - exact[rest])
    if form == "int":
        bound = ncc_bound_int(exact[rest])
        zero = exact[rest] == 0
        assert (got[rest][zero] == 0).all(), "exact == 0 must give 0"
    else:
        bound = np.full(err.shape, ncc_bound_loop(win), LD)
    worst = units(err, bound)
    assert (err <= bound).all(), f"NCC {form}: largest error is {worst:.3g} bounds"
    return worst


def check_asw(got, exact, winSize, nan_mask):
    """The assertions of one ASW cost volume (float32) against the exact reference -> largest error in units of the bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    assert np.array_equal(np.isnan(got), nan_mask), "NaN pattern != the dmax rule"
    assert np.array_equal(np.isnan(exact), nan_mask)
    ok = ~nan_mask
    g, e = got[ok], exact[ok]
    zero = e == 0
    assert (g[zero].view(np.uint32) == 0).all(), "exact == 0 must give +0"
    err = np.abs(g.astype(LD) - e)
    bound = asw_bound(e, winSize)
    worst = units(err, bound)
    assert (err <= bound).all(), f"ASW: largest error is {worst:.3g} bounds"
    return worst


def one_f32_ulp_apart(a, b):
    """largest |a - b| in float32 ulps of b, over the entries where b is not NaN (a, b float32 arrays)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ok = ~np.isnan(b)
    err = np.abs(a[ok].astype(np.float64) - b[ok].astype(np.float64))
    return float((err / np.spacing(np.abs(b[ok])).astype(np.float64)).max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------ inputs
def _rng(*key):
    return np.random.default_rng(list(key))


def ncc_images(O, H, W, kind, seed):
    if kind == "synth":
        L, R = O.synth_pair(H, W, 16, seed)
    elif kind == "synth_flat":
        L, R = O.synth_pair(H, W, 16, seed)
        L, R = L.copy(), R.copy()
        L[2:10, 6:30] = 90                     # flat patches larger than the window: A = 0 and / or B = 0
        R[1:11, 2:34] = 90
    elif kind == "noise":
        L, R = O.synth_pair(H, W, 16, seed, True)
    elif kind == "bright":                     # pixels 200..255, R = L shifted by 3 with 20 % of the pixels 255
        rng = _rng(seed, H, W)
        L = rng.integers(200, 256, (H, W)).astype(np.uint8)
        R = np.roll(L, -3, axis=1)
        R[rng.random((H, W)) < 0.2] = 255
    elif kind == "nearly_flat":                # constant 90 with 2 % of the pixels + 1: tiny radicands
        rng = _rng(seed, H, W)
        L = (90 + (rng.random((H, W)) < 0.02)).astype(np.uint8)
        R = (90 + (rng.random((H, W)) < 0.02)).astype(np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


# (H, W, D, win, image): the issue's table
NCC_CASES = [
    (12, 40, 20, 2, "synth_flat"),             # flat windows
    (10, 50, 30, 4, "bright"),                 # largest n Saa and Sa Sb
    (25, 41, 12, 10, "synth"),                 # NCC_main.cpp's 21x21 window
    (34, 40, 6, 15, "bright"),                 # 31x31, the last side of the integer-sum form
    (36, 38, 5, 16, "synth"),                  # side 33: both settings take the loop nest
    (9, 30, 33, 0, "synth"),                   # side 1: every window flat -> every valid cost NaN, map 0
    (7, 90, 65, 1, "noise"),                   # one hypothesis past a wave
    (6, 150, 257, 1, "noise"),                 # the D > 256 instantiation
    (12, 40, 20, 2, "nearly_flat"),            # tiny radicands
]
NCC_IDS = [f"{h}x{w}-D{d}-win{k}-{img}" for h, w, d, k, img in NCC_CASES]


def ncc_form(win, impl):
    """which bound a kernel setting is held to: the integer-sum form exists for sides up to 31"""
    return "int" if impl == 2 and 2 * win + 1 <= 31 else "loop"


@functools.lru_cache(maxsize=None)
def _ncc_case(idx):
    from oracle import oracle as O
    H, W, D, win, kind = NCC_CASES[idx]
    L, R = ncc_images(O, H, W, kind, 40 + idx)
    exact, flat, sentinel = ncc_exact(L, R, D, win)
    for a in (L, R, exact, flat, sentinel):
        a.setflags(write=False)
    return L, R, exact, flat, sentinel


def ncc_case(idx):
    """(L, R, exact, flat, sentinel) of NCC_CASES[idx]; computed once, read-only"""
    return _ncc_case(idx)


def asw_images(O, H, W, kind, seed):
    if kind == "synth":
        L, R = O.synth_pair(H, W, 16, seed)
    elif kind == "noise":
        L, R = O.synth_pair(H, W, 16, seed, True)
    elif kind == "checker":                    # 0 / 255 with 20 % of the pixels 128: weights from 1 down to e^-17 in one sum
        rng = _rng(seed, H, W)
        ii, jj = np.mgrid[0:H, 0:W]
        L = (((ii + jj) & 1) * 255).astype(np.uint8)
        L[rng.random((H, W)) < 0.2] = 128
        R = np.roll(L, -2, axis=1)
        R[rng.random((H, W)) < 0.2] = 128
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


# (H, W, D, winSize, T, image, sigma_color): the issue's table, then its first shape with the smallest sigma_color
# that keeps every product w0 w1 a normal float64
ASW_CASES = [
    (6, 30, 16, 2, 40, "synth", 30.0),         # basic
    (5, 24, 70, 1, 40, "noise", 30.0),         # D > 64, dd clamped on most of the row
    (4, 40, 12, 16, 40, "synth", 30.0),        # config 4's 35x35 window, 1 225 taps
    (5, 26, 10, 4, 40, "checker", 30.0),       # weights from 1 down to e^-17 in one sum
    (4, 20, 8, 2, 0, "synth", 30.0),           # T = 0: every cost exactly 0
    (4, 20, 8, 2, 255, "checker", 30.0),       # T = 255
    (5, 140, 130, 3, 40, "synth", 30.0),       # three hypotheses per lane
    (4, 150, 257, 1, 40, "noise", 30.0),       # D > 256
    (5, 20, 1, 2, 40, "synth", 30.0),          # D = 1
    (4, 3, 4, 2, 40, "synth", 30.0),           # right view: dmax < 0 everywhere -> all NaN, map 0
    (6, 30, 16, 2, 40, "synth", 2.0),          # sigma_color 2
]
ASW_IDS = [f"{h}x{w}-D{d}-ws{k}-T{t}-{img}-sc{sc:g}" for h, w, d, k, t, img, sc in ASW_CASES]
ASW_SIGMA_SPACE = 50.0


@functools.lru_cache(maxsize=None)
def _asw_case(idx):
    from oracle import oracle as O
    H, W, D, ws, T, kind, sc = ASW_CASES[idx]
    L, R = asw_images(O, H, W, kind, 60 + idx)
    Lp, Rp = np.pad(L, ws + 1, mode="edge"), np.pad(R, ws + 1, mode="edge")
    sp, cm = O.asw_masks(ws, ASW_SIGMA_SPACE, sc)
    exact = tuple(asw_exact(Lp, Rp, D, ws, sp, cm, T, v) for v in (0, 1))
    nan = tuple(asw_nan_mask(H, W, D, ws, v) for v in (0, 1))
    for a in (L, R, Lp, Rp, sp, cm) + exact + nan:
        a.setflags(write=False)
    return L, R, Lp, Rp, sp, cm, exact, nan


def asw_case(idx):
    """(L, R, Lp, Rp, space, color, (exactL, exactR), (nanL, nanR)) of ASW_CASES[idx]; computed once, read-only"""
    return _asw_case(idx)
