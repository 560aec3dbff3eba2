"""Cases and references shared by tests/test_ncc_whole_cpu.py, tests/test_ncc_whole_gpu.py and
tests/golden/make_ncc_whole_golden.py: NCC.h's whole-image ncc() (NCC/NCC.h:117-272) and bgr_to_grey (:97-115).

fixture_pairs   the six seeded pairs the fixture records (9x83 and 14x100: the reference's 79 offsets need W >= 79; noise,
                smooth, and images with all-zero and constant patches), and the BGR image of the bgr_to_grey record.
ref_loops       :181-267 restated loop for loop, vectorised over pixels and offsets only: every pixel's float64 sums run
                over its taps in the reference's order (rows outer), so each value is the reference's own sequence of IEEE
                operations.  -> (cost [H][W][O], offset [H][W]).
ref_int         the integer form of include/smt.h in int64 and float64, the same expression in the same order as
                csrc/ncc_whole_rules.h: bit for bit what the INT kernels compute.
exact_ld        the exact rational function Ci / (n sqrt(Ai Bi)) in np.longdouble from Python-exact integers;
                exact_fraction checks it on a sample.
winner          the sequential rule of :261-266 on a cost volume.

Bounds (u = 2^-53; each derived, then doubled, as tests/exact_matchers.py does):
bound_int       nw_int_cost takes exact integers (below 2^53) through five roundings -- two roots, their product, the
                product with n, the quotient -- each within u relative: (1 + u)^5 - 1 < 5.0000001 u relative.  Doubled:
                10 u |exact|.
bound_loop      With m = S / n: the computed mean is m (1 + d), |d| <= u (S and n are exact).  A = sum (a - m)^2 has
                non-negative terms, so sequential summation errs by at most (N - 1) u A; a term's own roundings (the
                difference, the square) add 3 u A; the mean's error moves the sum by 2 m d sum (a - m) = 2 m^2 d (N - n)
                to first order, and A >= N (mean - m)^2 = m^2 (N - n)^2 / N, so by at most 2 u N / (N - n) A <= 2 N u A.
                Hence A^ = A (1 + tA), |tA| <= (3 N + 2) u, and the same for B.  C = sum (a - ma)(b - mb) has terms of
                both signs, bounded through Cauchy-Schwarz: sum |terms| <= sqrt(A B), so summation adds (N - 1) u sqrt(A B),
                the terms' roundings 3 u sqrt(A B), the two means 2 u ma mb (N - n) <= 2 N u sqrt(A B):
                |C^ - C| <= (3 N + 2) u sqrt(A B).  res = C / (sqrt(A) sqrt(B)) / n after three divisions by n, two
                roots, a product and two quotients (8 u relative, and |res n| <= 1):
                |res^ - res| <= ((3 N + 2) + (3 N + 2) / 2 + (3 N + 2) / 2 + 8) u / n = (6 N + 12) u / n.
                Doubled: (12 N + 24) u / n, absolute.  Note |res| <= 1 / n.
The module also registers the new entry points in the bounds and stream-order tables (bottom), as
tests/cblsm_window_cases.py does.  The flow's ABI takes dense batches, so its rows have no strided gaps; the arena's
guards stand on both sides of every tensor all the same."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U53 = LD(2.0) ** -53
LOOP, INT = 1, 2
VL, VR = 1, 2
INT_MAX_K = 35
OUTS = ("depthL", "depthR", "offL", "offR", "lastdisp", "cls")
FIXTURE_SHAPES = ((9, 83), (14, 100))
FIXTURE_KINDS = ("noise", "smooth", "patches")


# ------------------------------------------------------------------------------------------------------------ images
def pair(H, W, kind, seed):
    """-> (L, R) uint8 [H][W]; the right image is mostly the left one moved by 4 columns (left type: b = R[x - o])"""
    rng = np.random.default_rng([seed, H, W, FIXTURE_KINDS.index(kind) if kind in FIXTURE_KINDS else 9])
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        base = 120 + 70 * np.sin(x / 5.0 + y / 3.0) + 30 * np.cos(x / 2.3) + rng.integers(-4, 5, (H, W))
        L = np.clip(base, 0, 255).astype(np.uint8)
    else:
        L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R[:, :W - 4] = np.where(rng.random((H, W - 4)) < 0.85, L[:, 4:], R[:, :W - 4])
    if kind == "patches":
        L[:, 10:30] = 0; R[:, 6:30] = 0                    # all-zero windows: NaN at every offset for some pixels
        L[:, 50:75] = 77; R[:, 40:75] = 200                # constant windows: the maximum 1 / n, exact ties
        L[H // 2:, W - 8:] = 0
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def fixture_pairs():
    """[(name, L, R)] in the fixture's order"""
    return [(f"{h}x{w}_{kind}", *pair(h, w, kind, 7)) for h, w in FIXTURE_SHAPES for kind in FIXTURE_KINDS]


def fixture_bgr():
    return np.random.default_rng(11).integers(0, 256, (7, 45, 3)).astype(np.uint8)


def add10(R):
    return np.minimum(R.astype(np.int32) + 10, 255).astype(np.uint8)


# -------------------------------------------------------------------------------------------------------- references
def shifted(L, R, O, view):
    """-> (a, b) uint8 [O][H][W]: the two images of every offset's comparison (NCC.h:143-174)"""
    H, W = L.shape
    o = np.arange(1, O + 1)[:, None]
    c = np.arange(W)[None, :]
    if view == VL:
        src = np.where(c < o, c, c - o)                    # T[y][c] = R[y][c] below o, R[y][c - o] from o on
        return np.broadcast_to(L, (O, H, W)), np.ascontiguousarray(R[:, src].transpose(1, 0, 2))
    src = np.where(c < W - o, c + o, c)                    # T'[y][c] = L[y][c + o] below W - o, L[y][c] from there on
    return np.ascontiguousarray(L[:, src].transpose(1, 0, 2)), np.broadcast_to(R, (O, H, W))


def extents(H, W, k):
    """-> (h, w) int64 [H][W]: rows and columns the loops visit; N = h w, n = (h - 1)(w - 1)"""
    y, x = np.mgrid[0:H, 0:W]
    h = np.minimum(H - 1, y + k) - np.maximum(0, y - k) + 1
    w = np.minimum(W - 1, x + k) - np.maximum(0, x - k) + 1
    return h.astype(np.int64), w.astype(np.int64)


def winner(cost):
    """:261-266 on cost [H][W][O] -> offset int32 [H][W] (0: no offset won)"""
    H, W, O = cost.shape
    best = np.full((H, W), -2.0)
    off = np.zeros((H, W), np.int32)
    for o in range(1, O + 1):
        c = cost[:, :, o - 1]
        with np.errstate(invalid="ignore"):
            up = c > best
        best = np.where(up, c, best)
        off = np.where(up, o, off).astype(np.int32)
    return off


def ref_loops(L, R, k, O, view):
    H, W = L.shape
    a, b = (np.pad(v.astype(np.float64), ((0, 0), (k, k), (k, k))) for v in shifted(L, R, O, view))
    y, x = np.mgrid[0:H, 0:W]
    h, w = extents(H, W, k)
    n = ((h - 1) * (w - 1)).astype(np.float64)
    taps = [(di, dj) for di in range(-k, k + 1) for dj in range(-k, k + 1)]

    def tap(v, di, dj):
        return v[:, k + di:k + di + H, k + dj:k + dj + W]

    def inside(di, dj):
        return (y + di >= 0) & (y + di < H) & (x + dj >= 0) & (x + dj < W)

    am = np.zeros((O, H, W)); bm = np.zeros((O, H, W))
    for di, dj in taps:
        ok = inside(di, dj)
        am = np.where(ok, am + tap(a, di, dj), am)
        bm = np.where(ok, bm + tap(b, di, dj), bm)
    am = am / n; bm = bm / n
    sa = np.zeros((O, H, W)); sb = np.zeros((O, H, W)); num = np.zeros((O, H, W))
    for di, dj in taps:
        ok = inside(di, dj)
        da, db = tap(a, di, dj) - am, tap(b, di, dj) - bm
        sa = np.where(ok, sa + da * da, sa)
        sb = np.where(ok, sb + db * db, sb)
        num = np.where(ok, num + da * db, num)
    with np.errstate(invalid="ignore", divide="ignore"):
        num = num / n; sa = sa / n; sb = sb / n
        res = num / (np.sqrt(sa) * np.sqrt(sb)) / n
    cost = np.ascontiguousarray(res.transpose(1, 2, 0))
    return cost, winner(cost)


def _box(v, k):
    """clamped (2k + 1)^2 window sums of int64 [..][H][W]"""
    H, W = v.shape[-2:]
    s = np.zeros(v.shape[:-2] + (H + 1, W + 1), np.int64)
    s[..., 1:, 1:] = v.cumsum(-2).cumsum(-1)
    y0 = np.maximum(0, np.arange(H) - k)[:, None]; y1 = (np.minimum(H - 1, np.arange(H) + k) + 1)[:, None]
    x0 = np.maximum(0, np.arange(W) - k)[None, :]; x1 = (np.minimum(W - 1, np.arange(W) + k) + 1)[None, :]
    return s[..., y1, x1] - s[..., y0, x1] - s[..., y1, x0] + s[..., y0, x0]


def int_terms(L, R, k, O, view):
    """-> (n, Ai, Bi, Ci) int64, [H][W] and three [H][W][O]; Python-exact while below 2^63 (k <= 35 keeps them below 2^53)"""
    a, b = (v.astype(np.int64) for v in shifted(L, R, O, view))
    H, W = L.shape
    h, w = extents(H, W, k)
    n = (h - 1) * (w - 1)
    q = 2 * n - h * w
    Sa, Sb, Saa, Sbb, Sab = _box(a, k), _box(b, k), _box(a * a, k), _box(b * b, k), _box(a * b, k)
    Ai = n * n * Saa - q * Sa * Sa
    Bi = n * n * Sbb - q * Sb * Sb
    Ci = n * n * Sab - q * Sa * Sb
    return n, Ai.transpose(1, 2, 0), Bi.transpose(1, 2, 0), Ci.transpose(1, 2, 0)


def ref_int(L, R, k, O, view):
    assert k <= INT_MAX_K
    n, Ai, Bi, Ci = int_terms(L, R, k, O, view)
    assert max(np.abs(Ai).max(), np.abs(Bi).max(), np.abs(Ci).max()) < 2 ** 53 and Ai.min() >= 0 and Bi.min() >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cost = Ci.astype(np.float64) / (n.astype(np.float64)[:, :, None] * (np.sqrt(Ai.astype(np.float64)) * np.sqrt(Bi.astype(np.float64))))
    cost = np.ascontiguousarray(cost)
    return cost, winner(cost)


def exact_ld(L, R, k, O, view):
    """-> (exact longdouble [H][W][O], flat bool [H][W][O] = {Ai Bi == 0}); the integers go into longdouble exactly while
    below 2^64 (asserted)"""
    n, Ai, Bi, Ci = int_terms(L, R, k, O, view)
    assert max(np.abs(Ai).max(), np.abs(Bi).max(), np.abs(Ci).max()) < 2 ** 62
    flat = (Ai == 0) | (Bi == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ex = Ci.astype(LD) / (n.astype(LD)[:, :, None] * (np.sqrt(Ai.astype(LD)) * np.sqrt(Bi.astype(LD))))
    return ex, flat


def exact_fraction(L, R, k, O, view, y, x, o):
    """one hypothesis from Python integers, the root to 40 digits"""
    a, b = shifted(L, R, O, view)
    H, W = L.shape
    ys, xs = slice(max(0, y - k), min(H - 1, y + k) + 1), slice(max(0, x - k), min(W - 1, x + k) + 1)
    av = [int(v) for v in a[o - 1][ys, xs].reshape(-1)]
    bv = [int(v) for v in b[o - 1][ys, xs].reshape(-1)]
    hh, ww = ys.stop - ys.start, xs.stop - xs.start
    n, N = (hh - 1) * (ww - 1), hh * ww
    q = 2 * n - N
    Ai = n * n * sum(v * v for v in av) - q * sum(av) ** 2
    Bi = n * n * sum(v * v for v in bv) - q * sum(bv) ** 2
    Ci = n * n * sum(p * r for p, r in zip(av, bv)) - q * sum(av) * sum(bv)
    if Ai * Bi == 0:
        return None
    scale = 10 ** 40
    return Fraction(Ci * scale, n * math.isqrt(Ai * Bi * scale * scale))


def bound_int(exact):
    return np.abs(np.asarray(exact, LD)) * (10 * U53)


def bound_loop(H, W, k):
    """[H][W][1] longdouble"""
    h, w = extents(H, W, k)
    return ((12 * h * w + 24).astype(LD) * U53 / ((h - 1) * (w - 1)).astype(LD))[:, :, None]


def bound_of(form, exact, k):
    H, W, _ = exact.shape
    return bound_int(exact) if form == INT else np.broadcast_to(bound_loop(H, W, k), exact.shape)


def units(err, bound):
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    pos = bound > 0
    return float((err[pos] / bound[pos]).max(initial=LD(0)))


def check_costs(got, exact, flat, form, k):
    """NaN exactly where Ai Bi == 0; elsewhere within the form's bound -> largest error in units of the bound"""
    assert np.array_equal(np.isnan(got), flat), "NaN pattern != {Ai Bi == 0}"
    ok = ~flat
    err = np.abs(got[ok].astype(LD) - exact[ok])
    bound = bound_of(form, exact, k)[ok]
    worst = units(err, bound)
    if form == INT:
        assert (got[ok][exact[ok] == 0] == 0).all(), "exact == 0 must give 0"
    assert (err <= bound).all(), f"form {form}: the largest error is {worst:.3g} bounds"
    return worst


def excused(off_got, off_ref, exact, bound_got, bound_ref):
    """-> number of pixels at which the two maps differ, every one of them excused: in the exact values the two choices lie
    closer than the sum of the two bounds (a pixel where one map names no offset is never excused)"""
    diff = np.argwhere(off_got != off_ref)
    for y, x in diff:
        g, f = int(off_got[y, x]), int(off_ref[y, x])
        assert g >= 1 and f >= 1, f"pixel ({y}, {x}): offsets {g} and {f}"
        gap = abs(exact[y, x, g - 1] - exact[y, x, f - 1])
        room = bound_got[y, x, g - 1] + bound_got[y, x, f - 1] + bound_ref[y, x, g - 1] + bound_ref[y, x, f - 1]
        assert gap < room / 2, f"pixel ({y}, {x}): offsets {g} and {f} lie {float(gap):.3g} apart, the bounds allow {float(room / 2):.3g}"
    assert len(diff) <= 0.005 * off_got.size, f"{len(diff)} of {off_got.size} pixels need the excuse"
    return len(diff)


def bgr_to_grey(bgr):
    t = np.array([int(0.333 * v) for v in range(256)], np.int32)           # uchar(0.333 v): truncated
    return (t[bgr[..., 2]] + t[bgr[..., 1]] + t[bgr[..., 0]]).astype(np.uint8)


def form_for(k, impl):
    return LOOP if impl == 1 or k > INT_MAX_K else INT


def reference(L, R, k, O, view, form, addc=False):
    Ru = add10(R) if addc else R
    return ref_int(L, Ru, k, O, view) if form == INT else ref_loops(L, Ru, k, O, view)


# (H, W, k, O): H = 2; every window clamped on both sides; k = 1; O = 1, O = W, the uchar wrap at 86 and 255; widths around
# the INT kernel's tile (256 - 2k output columns per workgroup: 246 at k = 5) and the wave; more than one row strip (8 rows)
SHAPES = [(2, 9, 5, 4), (7, 9, 5, 9), (5, 33, 1, 12), (3, 40, 2, 1), (4, 20, 3, 20), (3, 90, 2, 86), (2, 260, 1, 255),
          (3, 63, 5, 7), (3, 64, 5, 7), (3, 65, 5, 7), (3, 129, 5, 7), (2, 246, 5, 3), (2, 247, 5, 3), (19, 21, 5, 10)]


# ------------------------------------------------------------------------- rows of the bounds and stream-order suites
import ctypes as C  # noqa: E402

import bounds_cases as BC  # noqa: E402
import stream_order_cases as SC  # noqa: E402

BC.NOT_CALLER_BUFFER.update({
    "smt_whole_ncc_default_params": "fills a parameter struct", "smt_whole_ncc_set_impl": "setter",
    "smt_whole_ncc_last_form": "no buffers", "smt_whole_ncc_set_groups": "setter", "smt_whole_ncc_last_groups": "no buffers", "smt_whole_ncc_selftest_box": "host-only selftest",
    "smt_whole_ncc_flow_create_on": "handle", "smt_whole_ncc_flow_destroy": "handle",
    "smt_whole_ncc_flow_set_stream": "setter", "smt_whole_ncc_flow_set_form": "setter",
})


def _params(X, k, O, addc=False):
    p = X.L.NCCWholeParams()
    p.kernel_size, p.max_offset, p.add_constant = k, O, int(addc)
    return p


_WHOLE_CASES = [dict(H=h, W=w, k=k, O=o, view=v, impl=i, cost=c) for (h, w, k, o) in ((2, 9, 5, 4), (5, 33, 1, 12), (3, 65, 5, 7), (10, 21, 2, 21))
                for v, i, c in ((VL, 2, True), (VR, 2, True), (VL, 1, True), (VR, 1, False))]
_WHOLE_CASES += [dict(H=3, W=80, k=36, O=3, view=VL, impl=0, cost=True), dict(H=4, W=30, k=2, O=9, view=VR, impl=0, cost=False, addc=True)]


@BC.entry("smt_whole_ncc", *_WHOLE_CASES)
def _whole(A, X, H, W, k, O, view, impl, cost, addc=False):
    L, R = pair(H, W, "noise", 300)
    if addc:
        R = (228 + R % 28).astype(np.uint8)                  # bytes above 245 saturate
    A.inp("L", L); A.inp("R", R)
    A.out("depth", (H, W), np.uint8); A.out("off", (H, W), np.int32)
    if cost:
        A.out("cost", (H, W, O), np.float64)

    def call():
        X.lib.smt_whole_ncc_set_impl(impl)
        try:
            p = _params(X, k, O, addc)
            rc = X.lib.smt_whole_ncc(A.ptr("L"), A.ptr("R"), H, W, C.byref(p), view, A.ptr("depth"), A.ptr("off"),
                                     A.ptr("cost" if cost else None), X.st())
            A.extra["form"] = np.array([X.lib.smt_whole_ncc_last_form()], np.int32)
            return rc
        finally:
            X.lib.smt_whole_ncc_set_impl(0)

    def verify(o):
        form = form_for(k, impl)
        assert int(o["form"][0]) == form, "the hook and the integer limit must select the form"
        rcost, roff = reference(L, R, k, O, view, form, addc)
        if cost:
            BC.nan_bits_eq(o["cost"], rcost, "cost")
        BC.val_eq(o["off"], roff, "offset")
        BC.val_eq(o["depth"], (3 * roff).astype(np.uint8), "depth")
    return call, verify


@BC.entry("smt_bgr_to_grey_batch", dict(n=1, H=1, W=63), dict(n=3, H=5, W=65), dict(n=2, H=3, W=257))
def _grey(A, X, n, H, W):
    bgr = BC.rb((n, H, W, 3), 17)
    A.inp("bgr", bgr); A.out("grey", (n, H, W), np.uint8)
    return (lambda: X.lib.smt_bgr_to_grey_batch(A.ptr("bgr"), n, H, W, A.ptr("grey"), X.st()),
            lambda o: BC.bits_eq(o["grey"], bgr_to_grey(bgr), "grey"))


FLOW_CASES = [dict(H=h, W=w, k=k, O=o, form=f, P=p, outs=outs) for h, w, k, o, f, p, outs in [
    (5, 33, 1, 12, INT, 3, OUTS), (5, 33, 1, 12, LOOP, 3, OUTS), (5, 33, 1, 12, 0, 1, OUTS), (3, 65, 5, 7, INT, 3, ("depthR",)),
    (3, 65, 5, 7, INT, 1, ("lastdisp",)), (2, 9, 5, 4, INT, 3, ("offL", "cls")), (10, 21, 2, 21, LOOP, 2, ("depthL", "offR")),
    (10, 21, 2, 21, INT, 3, OUTS)]]


def flow_pairs(H, W, P):
    return [pair(H, W, "noise", 310 + 3 * b) for b in range(P)]


def flow_reference(X, L, R, k, O, form, addc=False):
    """{name: map} of one pair: both views by the form's restatement, then the oracle's Sad.h:184-222 on the offset maps"""
    ol, orr = reference(L, R, k, O, VL, form, addc)[1], reference(L, R, k, O, VR, form, addc)[1]
    last, cls = X.O.sad_crosscheck(ol, orr)
    return dict(depthL=(3 * ol).astype(np.uint8), depthR=(3 * orr).astype(np.uint8), offL=ol, offR=orr, lastdisp=last, cls=cls)


@BC.entry("smt_whole_ncc_flow_run_batch", *FLOW_CASES)
def _whole_flow(A, X, H, W, k, O, form, P, outs):
    imgs = flow_pairs(H, W, P)
    A.inp("L", np.stack([i[0] for i in imgs])); A.inp("R", np.stack([i[1] for i in imgs]))
    for nm in outs:
        A.out(nm, (P, H, W), np.int32 if nm in ("offL", "offR", "lastdisp") else np.uint8)

    def call():
        h = C.c_void_p()
        p = _params(X, k, O)
        rc = X.lib.smt_whole_ncc_flow_create_on(X.dev_index, H, W, C.byref(p), C.byref(h))
        if rc:
            return rc
        try:
            rc = X.lib.smt_whole_ncc_flow_set_form(h, form) or X.lib.smt_whole_ncc_flow_set_stream(h, X.st())
            rc = rc or X.lib.smt_whole_ncc_flow_run_batch(h, A.ptr("L"), A.ptr("R"), P, *[A.ptr(nm if nm in outs else None) for nm in OUTS])
            A.extra["form"] = np.array([X.lib.smt_whole_ncc_last_form()], np.int32)
            return rc
        finally:
            X.lib.smt_whole_ncc_flow_destroy(h)

    def verify(o):
        f = form or form_for(k, 0)
        assert int(o["form"][0]) == f, "set_form must select the form"
        for b, (L, R) in enumerate(imgs):
            ref = flow_reference(X, L, R, k, O, f)
            for nm in outs:
                BC.val_eq(o[nm][b], ref[nm], f"{nm}[{b}]")
    return call, verify


SC.SYNCHRONISING.update({name: SC.ASYNC for name in ("smt_whole_ncc", "smt_bgr_to_grey_batch", "smt_whole_ncc_flow_run_batch")})
