"""Cases and references shared by tests/test_cblsm_window_cpu.py and tests/test_cblsm_window_gpu.py: CBLSM's window cost
volumes (ComputeDispLeft / ComputeDispRight / ComputeDispV4, CBLSM/CBLSM.h:451-489, :409-447, :494-532) and the flow of
CBLSM.cpp with :132 enabled.

ref_loops       the three functions restated loop for loop in NumPy on a flat buffer: a guarded entry copies the element
                before it, whichever pixel that belongs to (RIGHT's read of the previous pixel's last entry included).
ref_volume      the vectorised form (integral images per hypothesis, then the chain as a gather); the tests hold it to
                ref_loops on the small shapes and use it everywhere.
quotient        the float nearest to S / n, the value sadvalueMean returns for an integer sum S of n taps.
TABLE           (H, W, D, winSize) of the issue: every lane-slot count, D past W, W = w + 1, the strip edge of the box
                kernel's workgroups (32 columns at D <= 64, 16 beyond), a 31 x 31 and the 181 x 181 window (FILL, FILL_R: all-0 against all-255 images).
The module also registers the new entry points in the bounds and stream-order tables (bottom), as
tests/asw_tail_cases.py does."""
import numpy as np

LEFT, RIGHT, V4 = 1, 2, 3
STRIP = 32                                      # columns per workgroup of k_win_box at D <= 64 (16 beyond: 64 is an edge of both)
FILL = (12, 12, 4, 89)                          # W <= w: LEFT and V4 only, RIGHT is the reference's undefined case
FILL_R = (12, 100, 4, 89)                       # the same window where RIGHT has legal columns
TABLE = [(5, 7, 4, 0), (9, 20, 12, 1), (6, 5, 9, 1), (4, 6, 1, 1), (4, 3, 5, 1), (6, 70, 65, 1), (5, 150, 130, 1),
         (4, 300, 257, 0), (3, 40, 512, 1), (7, STRIP - 1, 8, 1), (7, STRIP, 8, 1), (7, STRIP + 1, 8, 1),
         (7, 63, 8, 1), (7, 64, 8, 1), (7, 65, 8, 1), (4, 17, 70, 1), (40, 50, 16, 14), FILL, FILL_R]
SMALL = [c for c in TABLE if c[0] * c[1] * c[2] <= 6000 and c[3] <= 1]


def quotient(S, n):
    """float32 nearest to S / n (double division, then narrowed: the same float as cv::mean's sum * (1.0 / n))"""
    return (np.asarray(S, np.float64) / np.float64(n)).astype(np.float32)


def pair(H, W, winSize, seed, channels=1):
    """-> padded (Lp, Rp): random bytes, the right image mostly the left shifted by 3; FILL's shape gives 0 against 255"""
    w = winSize + 1
    rng = np.random.default_rng([seed, H, W, winSize, channels])
    shp = (H, W) if channels == 1 else (H, W, channels)
    L = rng.integers(0, 256, shp).astype(np.uint8)
    R = rng.integers(0, 256, shp).astype(np.uint8)
    if W > 3:
        keep = rng.random(shp)[:, :W - 3] < 0.8
        R[:, :W - 3] = np.where(keep, L[:, 3:], R[:, :W - 3])
    pad = ((w, w), (w, w)) + (((0, 0),) if channels != 1 else ())
    return np.pad(L, pad, mode="edge"), np.pad(R, pad, mode="edge")


def fill_pair(H, W, winSize):
    w = winSize + 1
    return np.zeros((H + 2 * w, W + 2 * w), np.uint8), np.full((H + 2 * w, W + 2 * w), 255, np.uint8)


def case_pair(case, seed=1):
    H, W, D, ws = case
    return fill_pair(H, W, ws) if tuple(case) in (FILL, FILL_R) else pair(H, W, ws, seed)


def legal(case, form):
    """False where the reference reads before its buffer (RIGHT with W <= winSize + 1): SMT_ERR_REF_UB, nothing written"""
    return not (form == RIGHT and case[1] <= case[3] + 1)


def _window_cost(lw, rw, form):
    d = np.abs(lw.astype(np.int64) - rw.astype(np.int64))
    if form == V4:
        # minValue per tap, `sumvalue +=` into a uchar, `sumvalue / number` as integers, returned as float
        return np.float32((int(d.min(axis=2).sum()) % 256) // (d.shape[0] * d.shape[1]))
    return quotient(int(d.sum()), d.size)


def ref_loops(Lp, Rp, D, winSize, form):
    """the reference's loops as written: padded indices i, j; output pixel (i - win_r, j - win_r)"""
    win_r = winSize + 1
    row, col = Lp.shape[:2]
    H, W = row - 2 * win_r, col - 2 * win_r
    rowrange, colrange = row - winSize - 1, col - winSize - 1
    vol = np.full(H * W * D, np.nan, np.float32)
    for i in range(win_r, rowrange):
        for j in range(win_r, colrange):
            own = (Rp if form == RIGHT else Lp)[i - win_r:i + win_r + 1, j - win_r:j + win_r + 1]
            for d in range(D):
                idx = (i - win_r) * W * D + (j - win_r) * D + d
                guard = (j + d + win_r + 1 > colrange) if form == RIGHT else (j - win_r - d < 0)
                if guard:
                    assert idx >= 1, "the reference reads before its buffer"
                    vol[idx] = vol[idx - 1]
                    continue
                if form == RIGHT:
                    vol[idx] = _window_cost(Lp[i - win_r:i + win_r + 1, j - win_r + d:j + d + win_r + 1], own, form)
                else:
                    vol[idx] = _window_cost(own, Rp[i - win_r:i + win_r + 1, j - win_r - d:j - d + win_r + 1], form)
    return vol.reshape(H, W, D)


def _box(a, side):
    """[Hp][Wc] -> sums over side x side windows, [Hp - side + 1][Wc - side + 1]"""
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    return s[side:, side:] - s[:-side, side:] - s[side:, :-side] + s[:-side, :-side]


def ref_sums(Lp, Rp, D, winSize, form):
    """integer window sums S[y][x][d] of every hypothesis whose windows lie inside the padded rows (-1 elsewhere):
    LEFT / V4 d <= x, RIGHT x + d <= W - 1"""
    w = winSize + 1
    side = 2 * w + 1
    H, W = Lp.shape[0] - 2 * w, Lp.shape[1] - 2 * w
    S = np.full((H, W, D), -1, np.int64)
    Li, Ri = Lp.astype(np.int64), Rp.astype(np.int64)
    for d in range(min(D, W)):
        a = np.abs(Li[:, d:] - Ri[:, :Lp.shape[1] - d])           # column c: left c + d against right c
        if form == V4:
            a = a.min(axis=2)
        b = _box(a, side)                                          # [H][W - d]: right window at column x', left at x' + d
        if form == RIGHT:
            S[:, :W - d, d] = b
        else:
            S[:, d:, d] = b
    return S


def ref_volume(Lp, Rp, D, winSize, form):
    w = winSize + 1
    n = (2 * w + 1) ** 2
    S = ref_sums(Lp, Rp, D, winSize, form)
    H, W = S.shape[:2]
    cost = (((S % 256) // n).astype(np.float32) if form == V4 else quotient(S, n))
    x, d = np.meshgrid(np.arange(W), np.arange(D), indexing="ij")
    if form == RIGHT:
        assert W > w, "the reference reads before its buffer"
        lim = W - 1 - w - x
        xs, ds = np.where(lim >= 0, x, W - 1 - w), np.where(lim >= 0, np.minimum(d, lim), 0)
    else:
        xs, ds = x, np.minimum(d, x)
    assert (S[:, xs, ds] >= 0).all()
    return np.ascontiguousarray(cost[:, xs, ds])


def flow_oracle(O, L, R, D, winSize, maxlen=34, sec=17, tau=25):
    """CBLSM.cpp:64-67, 101-104, 124-125, 132 (and its right counterpart), 146-153 from the oracle's pieces; the shape
    of tests/test_cblsm_flow_gpu.py::_oracle with the window volumes in place of the AD volumes"""
    w = winSize + 1
    aL = O.arms_all(L, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    aR = O.arms_all(R, tau0=tau, tau_low=6, sec=sec, maxlen=maxlen, chain=False, right_row_bug=False)
    Lp, Rp = np.pad(L, w, mode="edge"), np.pad(R, w, mode="edge")
    cr, _ = O.aggregate_rect(ref_volume(Lp, Rp, D, winSize, RIGHT), aR, 1)
    cl, _ = O.aggregate_rect(ref_volume(Lp, Rp, D, winSize, LEFT), aL, 1)
    cl2, _ = O.aggregate_rect(cl, aL, 1)
    cr2, _ = O.aggregate_rect(cr, aL, 1)
    return cl, cr, O.wta(cl2), O.wta(cr2)


# ------------------------------------------------------------------------- rows of the bounds and stream-order suites
# Registered on import, as tests/asw_tail_cases.py does.  The all-0 / all-255 case has no decoy (a constant image is its
# own reversal), so it is not in the table: tests/test_cblsm_window_gpu.py runs it on NaN-prefilled outputs itself.
import ctypes as C  # noqa: E402

import bounds_cases as BC  # noqa: E402
import stream_order_cases as SC  # noqa: E402

BC.NOT_CALLER_BUFFER.update({
    "smt_cblsm_window_set_impl": "setter", "smt_cblsm_window_set_band": "setter", "smt_cblsm_window_set_store": "setter",
    "smt_cblsm_window_last_form": "no buffers", "smt_cblsm_selftest_window": "host-only selftest",
    "smt_cblsm_window_quotient": "test hook over a flat array of sums; tests/test_cblsm_window_gpu.py sweeps every sum",
})
BC.HOST_ENTRIES = tuple(BC.HOST_ENTRIES) + ("smt_cblsm_window_cost_host",)


def _vol_entry(host):
    def f(A, X, H, W, D, ws, form, impl=0, band=0, gap=0, P=1):
        w = ws + 1
        prs = [pair(H, W, ws, 40 + b, 3 if form == V4 else 1) for b in range(P)]
        Lp, Rp = np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])
        si, sv = BC._strided(gap, Lp[0].size), BC._strided(gap, H * W * D)
        A.inp("Lp", Lp, stride=si); A.inp("Rp", Rp, stride=si); A.out("vol", (P, H, W, D), np.float32, stride=sv)

        def call():
            args = (A.ptr("Lp"), A.ptr("Rp"), P, BC.sz(si), H, W, D, ws, form, A.ptr("vol"), BC.sz(sv))
            if host:
                return X.lib.smt_cblsm_window_cost_host(*args)
            X.lib.smt_cblsm_window_set_impl(impl); X.lib.smt_cblsm_window_set_band(band)
            try:
                rc = X.lib.smt_cblsm_window_cost_batch(*args, X.st())
                A.extra["form"] = np.array([X.lib.smt_cblsm_window_last_form()], np.int32)
                return rc
            finally:
                X.lib.smt_cblsm_window_set_impl(0); X.lib.smt_cblsm_window_set_band(0)

        def verify(o):
            if not host and impl:
                assert int(o["form"][0]) == (1 if form == V4 else impl), "the hook must select the formulation"
            for b in range(P):
                BC.bits_eq(o["vol"][b], ref_volume(Lp[b], Rp[b], D, ws, form), f"vol[{b}]")
        return call, verify
    return f


_VOL_CASES = [dict(H=h, W=w, D=d, ws=k, form=f, impl=i) for (h, w, d, k) in ((4, 3, 5, 1), (3, 65, 65, 1), (2, 40, 300, 0))
              for f in (LEFT, RIGHT) for i in (1, 2)]
_VOL_CASES += [dict(H=5, W=33, D=20, ws=1, form=f, impl=2, band=b, gap=1, P=3) for f in (LEFT, RIGHT) for b in (0, 2)]
_VOL_CASES += [dict(H=5, W=33, D=20, ws=1, form=LEFT, impl=1, gap=1, P=3), dict(H=3, W=9, D=12, ws=0, form=V4, gap=1, P=3),
               dict(H=4, W=20, D=8, ws=3, form=RIGHT, impl=0)]
BC.entry("smt_cblsm_window_cost_batch", *_VOL_CASES)(_vol_entry(False))
BC.entry("smt_cblsm_window_cost_host", *[dict(c) for c in _VOL_CASES if c.get("impl", 0) != 1 and not c.get("band")])(_vol_entry(True))


@BC.entry("smt_cblsm_flow_run_batch_window", dict(H=5, W=65, D=64, ws=1, P=2), dict(H=3, W=33, D=65, ws=0, P=1),
          dict(H=2, W=20, D=1, ws=2, P=2))
def _b_flow_window(A, X, H, W, D, ws, P):
    import cblsm_v4_cases as VC
    Ls = np.stack([VC.noisy_pair(H, W, 70 + b)[0] for b in range(P)])
    Rs = np.stack([VC.noisy_pair(H, W, 70 + b)[1] for b in range(P)])
    A.inp("L", Ls); A.inp("R", Rs); A.out("dispL", (P, H, W), np.float32); A.out("dispR", (P, H, W), np.float32)

    def call():
        p, h = X.L.CBLSMParams(), C.c_void_p()
        X.lib.smt_cblsm_default_params(C.byref(p))
        rc = X.lib.smt_cblsm_flow_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
        try:
            rc = rc or X.lib.smt_cblsm_flow_set_stream(h, X.st())
            rc = rc or X.lib.smt_cblsm_flow_run_batch_window(h, A.ptr("L"), A.ptr("R"), P, ws, A.ptr("dispL"), A.ptr("dispR"))
            return rc or X.lib.smt_cblsm_flow_status(h)
        finally:
            X.lib.smt_cblsm_flow_destroy(h)

    def verify(o):
        for b in range(P):
            _, _, dl, dr = flow_oracle(X.O, Ls[b], Rs[b], D, ws)
            BC.val_eq(o["dispL"][b], dl, f"dispL[{b}]"); BC.val_eq(o["dispR"][b], dr, f"dispR[{b}]")
    return call, verify


SC.SYNCHRONISING.update({name: SC.ASYNC for name in ("smt_cblsm_window_cost_batch", "smt_cblsm_flow_run_batch_window")})
