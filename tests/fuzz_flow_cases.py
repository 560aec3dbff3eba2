"""Case table and oracle compositions of the random-shape sweep over the batched flows on reused handles
(tests/test_fuzz_flows_cpu.py holds the table to its coverage on the oracle alone, tests/test_fuzz_flows_gpu.py runs it on
the device).  A plain module, importable without a GPU.

A GROUP is one handle: a shape, its parameters, and three BATCHES run on that handle in order, with different images and
different pair counts (every group holds a one-pair batch; one group per family holds a five-pair batch).  The table
comes from numpy.random.default_rng(SEED): the rows a family must reach (a D bin, one row, W < D, ...) are fixed per group
index, everything they leave open is drawn.  Sizes follow the oracle's CPU time, not the kernels: about 4e5 hypotheses
per batch (6e4 for ASW, 1.2e5 for CBLSM, whose costAggregationV4 restatement runs in NumPy).

oracle_batch(family, group, k, O) -> (list of per-pair dicts of named arrays, dict of the last pair's volumes), computed
once per process and returned read-only; the compositions are the ones the hand-picked tests use, imported from them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cblsm_v4_cases as VC  # noqa: E402
import exact_matchers as X  # noqa: E402
import median_inplace_cases as MC  # noqa: E402
from test_cblsm_flow_gpu import _oracle as cblsm_oracle  # noqa: E402
from prefill import first_diff  # noqa: E402,F401  (re-exported for the sweep's messages)
from test_fuzz_gpu import rand_img  # noqa: E402

SEED = 20261019
INT_MIN = -(2 ** 31)
FAMILIES = ("pipeline", "cblsm", "crossagg", "sad", "ncc", "asw", "host")
BUDGET = dict(pipeline=4e5, cblsm=1.2e5, crossagg=4e5, sad=4e5, ncc=4e5, asw=6e4, host=4e5)
P_ORDERS = ((3, 1, 2), (2, 1, 3), (1, 3, 2), (2, 3, 1))
P_FIVE = ((5, 1, 2), (2, 5, 1))
NCC_LOOP, NCC_DOT4, NCC_BOX = 1, 2, 3
ASW_SIGMA_SPACE, ASW_SIGMA_COLOR, ASW_T = 50.0, 30.0, 40           # smt_asw_default_params


def _fit(rng, D, P, budget, hmax=24, wmin=2, wmax=160, H=None, W=None):
    """(H, W) drawn under H * W * D * P <= budget; a given H or W is kept"""
    for _ in range(1000):
        h = int(rng.integers(1, hmax + 1)) if H is None else H
        w = int(rng.integers(wmin, wmax + 1)) if W is None else W
        if h * w * D * P <= budget:
            return h, w
    raise AssertionError(("no shape under the budget", D, P, budget, H, W))


def _batches(rng, order):
    return [dict(P=int(P), seed=int(rng.integers(1, 2 ** 31))) for P in order]


def _order(rng, k, five_at):
    return P_FIVE[int(rng.integers(0, 2))] if k in five_at else P_ORDERS[int(rng.integers(0, len(P_ORDERS)))]


# ------------------------------------------------------------------------------------------------ the table
PIPE_D_BINS = ((1, 63), (64, 64), (65, 127), (128, 128), (129, 191), (192, 192), (193, 255), (256, 256), (257, 320))
PIPE_BIN_OF_GROUP = (4, 1, 0, 3, 6, 5, 0, 7, 8, 2, 0, 2, 0, 0, 0, 0)   # index into PIPE_D_BINS per group: every bin is taken
PIPE_SCHEDULES = (None, "0", "1", "2")


def _pipeline(rng):
    """16 groups over the nine D bins; schedules cycle unset, 0, 1, 2; every fourth group (2, 6, 10, 14) runs under
    QUIRK_FIX_RIGHT_ARM_STRIDE: a square, a portrait and two landscape shapes.  Schedule 2 gets the groups 3, 7, 11, 15:
    one of them holds the five-pair batch, and all hold P = 1 and 2.  Group 0 is one row, groups 1 and 5 have W < D,
    groups 12 .. 15 have 20 .. 40 rows of 100 .. 180 pixels (several tiles in both directions) and few hypotheses."""
    out = []
    for k in range(16):
        lo, hi = PIPE_D_BINS[PIPE_BIN_OF_GROUP[k]]
        D = int(rng.integers(max(lo, 4), hi + 1))                      # under 4 hypotheses the maps have nothing to show
        order = _order(rng, k, five_at=(7, 9))
        Pmax = max(order)
        fix = k % 4 == 2
        if k >= 12:
            D = int(rng.integers(8, 25))
            H, W = _fit(rng, D, Pmax, BUDGET["pipeline"], hmax=40, wmin=100, wmax=180)
            H = max(H, 20)
        elif fix:
            side = int(rng.integers(32, 41))
            room = int(BUDGET["pipeline"] // (side * D * Pmax))
            H, W = ((side, side), (side + int(rng.integers(2, 9)), side), (side, min(side + int(rng.integers(20, 60)), room)))[k // 4]
        elif k == 0:
            H, W = _fit(rng, D, Pmax, BUDGET["pipeline"], H=1, wmin=65)
        elif k in (1, 5):                                               # W < D, W no multiple of 4
            W = int(rng.integers(D // 2, D))
            W += (W % 4 == 0)
            H = int(rng.integers(2, 8))
        else:
            H, W = _fit(rng, D, Pmax, BUDGET["pipeline"], hmax=12, wmin=66 if k % 2 else 25)
        if not fix and W % 4 == 0:
            W += 1
        assert H * W * D * Pmax <= 1.3 * BUDGET["pipeline"] and (fix or H <= W), (k, H, W, D, Pmax)
        out.append(dict(family="pipeline", name=f"pipe{k}_{H}x{W}x{D}", H=H, W=W, D=D, schedule=PIPE_SCHEDULES[k % 4],
                        fix_stride=fix, batches=_batches(rng, order)))
    return out


def _cblsm(rng):
    """8 groups: D <= 64, 65 .. 256, > 256; one row, one column; tau 0 and 255; short and long arms"""
    spec = [dict(D=(2, 64)), dict(D=(65, 256), tau=0), dict(D=(257, 320), tau=255), dict(D=(2, 64), H=1),
            dict(D=(2, 40), W=1), dict(D=(64, 64), tau=255), dict(D=(65, 130), tau=0), dict(D=(2, 64))]
    out = []
    for k, s in enumerate(spec):
        D = int(rng.integers(s["D"][0], s["D"][1] + 1))
        order = _order(rng, k, five_at=(3,))
        H, W = _fit(rng, D, max(order), BUDGET["cblsm"], hmax=12, wmin=32, wmax=80, H=s.get("H"), W=s.get("W"))
        tau = s.get("tau", int(rng.choice([25, 8, 40])))
        maxlen = int(rng.choice([34, 5, 12]))
        sec = int(rng.integers(0, maxlen + 1)) if k % 2 else min(17, maxlen)
        out.append(dict(family="cblsm", name=f"cblsm{k}_{H}x{W}x{D}", H=H, W=W, D=D, tau=tau, max_length=maxlen,
                        sec_length=sec, batches=_batches(rng, order)))
    return out


def _crossagg(rng):
    """8 groups: num_iters 0 .. 4; L1 above W; D = 1, 64, 65, > 256; the gray pair given in the odd groups"""
    spec = [dict(D=1, iters=4), dict(D=64, iters=0), dict(D=65, iters=1), dict(D=int(rng.integers(257, 321)), iters=2),
            dict(D=int(rng.integers(2, 64)), iters=3, L1_above_W=True), dict(D=int(rng.integers(66, 200)), iters=4),
            dict(D=int(rng.integers(2, 33)), iters=2, big=True), dict(D=int(rng.integers(129, 257)), iters=3)]
    out = []
    for k, s in enumerate(spec):
        D = s["D"]
        order = _order(rng, k, five_at=(6,))
        H, W = _fit(rng, D, max(order), BUDGET["crossagg"], hmax=40 if s.get("big") else 14, wmin=16, wmax=130)
        L1 = W + int(rng.integers(1, 40)) if s.get("L1_above_W") else int(rng.choice([34, 5, 60]))
        out.append(dict(family="crossagg", name=f"xagg{k}_{H}x{W}x{D}", H=H, W=W, D=D, L1=L1, L2=int(rng.choice([17, 2])),
                        t1=int(rng.choice([20, 8])), t2=int(rng.choice([6, 3])), num_iters=s["iters"],
                        gate=int(rng.choice([1, 2, 5])), gray_given=bool(k % 2), batches=_batches(rng, order)))
    return out


def _sad(rng):
    """8 groups: winsize 0 .. 4; D = 1, 64, 65, 130; W <= D"""
    spec = [dict(D=1, ws=0), dict(D=64, ws=1), dict(D=65, ws=2), dict(D=130, ws=3), dict(D=64, ws=4, W_le_D=True),
            dict(D=130, ws=0, W_le_D=True), dict(D=int(rng.integers(2, 64)), ws=2), dict(D=int(rng.integers(66, 130)), ws=4)]
    out = []
    for k, s in enumerate(spec):
        D = s["D"]
        order = _order(rng, k, five_at=(6,))
        H, W = _fit(rng, D, max(order), BUDGET["sad"], hmax=16, wmax=D if s.get("W_le_D") else 150)
        out.append(dict(family="sad", name=f"sad{k}_{H}x{W}x{D}_ws{s['ws']}", H=H, W=W, D=D, winsize=s["ws"],
                        batches=_batches(rng, order)))
    return out


def ncc_rule(side, D):
    """ncc_flow_rule of csrc/ncc_box.hip, restated: the form NCCFlow takes when none is set"""
    if side <= 31:
        return NCC_BOX if (side >= 9 and 33 <= D <= 64) else NCC_DOT4
    return NCC_BOX if side <= 181 else NCC_LOOP


def _ncc(rng):
    """9 groups: the sides on both sides of every switch of the dispatch rule (7 | 9 with 33 <= D <= 64, 31 | 33,
    181 | 183), D on both sides of 33 and 64 at side 9, and an empty interior (H or W <= 2 win)"""
    d31 = int(rng.integers(2, 12))
    spec = [dict(win=3, D=48), dict(win=4, D=48), dict(win=4, D=32), dict(win=4, D=65), dict(win=15, D=d31),
            dict(win=16, D=d31), dict(win=90, D=2), dict(win=91, D=2),
            dict(win=5, D=int(rng.integers(2, 40)), empty=True)]
    out = []
    for k, s in enumerate(spec):
        win, D = s["win"], s["D"]
        side = 2 * win + 1
        order = (2, 1, 1) if win >= 90 else _order(rng, k, five_at=(0,))
        if s.get("empty"):
            H, W = (2 * win, int(rng.integers(side, 60))) if rng.integers(0, 2) else (int(rng.integers(side, 30)), 2 * win - 1)
        else:
            # the reference's argmax takes the 255.0 it stores for j - win - d < 0: real costs decide only at columns
            # past win + D, so the rows are longer than that
            H = side + int(rng.integers(1, 7))
            W = side + (int(rng.integers(3, 8)) if win >= 90 else D + int(rng.integers(12, 40)))
        assert H * W * D * max(order) <= BUDGET["ncc"], (k, H, W, D)
        forms = [0, NCC_LOOP, NCC_BOX] + ([NCC_DOT4] if side <= 31 else [])
        if side > 181:
            forms = [0, NCC_LOOP]                                           # box and dot4 do not exist past 181
        out.append(dict(family="ncc", name=f"ncc{k}_{H}x{W}x{D}_win{win}", H=H, W=W, D=D, winSize=win, forms=forms,
                        batches=_batches(rng, order)))
    return out


def _asw(rng):
    """6 groups: winSize 1 .. 3; D = 1, 64, 70"""
    spec = [dict(D=1, ws=1), dict(D=64, ws=2), dict(D=70, ws=3), dict(D=int(rng.integers(2, 30)), ws=3),
            dict(D=70, ws=1), dict(D=int(rng.integers(2, 64)), ws=2)]
    out = []
    for k, s in enumerate(spec):
        D = s["D"]
        order = _order(rng, k, five_at=(3,))
        H, W = _fit(rng, D, max(order), BUDGET["asw"], hmax=6, wmin=8, wmax=90)
        out.append(dict(family="asw", name=f"asw{k}_{H}x{W}x{D}_ws{s['ws']}", H=H, W=W, D=D, winSize=s["ws"],
                        batches=_batches(rng, order)))
    return out


def _host(rng):
    """8 groups: gray and BGR, f32 and u8 maps; chunk 1, 2 and above P; D = 64, 192, 256, and 320 with f32 maps"""
    spec = [dict(D=64, ch=1, u8=False, chunk=1), dict(D=192, ch=3, u8=True, chunk=2), dict(D=256, ch=1, u8=True, chunk=16),
            dict(D=320, ch=3, u8=False, chunk=2), dict(D=int(rng.integers(2, 64)), ch=3, u8=True, chunk=1),
            dict(D=256, ch=3, u8=False, chunk=7), dict(D=int(rng.integers(65, 192)), ch=1, u8=True, chunk=2),
            dict(D=64, ch=1, u8=False, chunk=2)]
    out = []
    for k, s in enumerate(spec):
        D = s["D"]
        order = _order(rng, k, five_at=(1, 7))
        H, W = _fit(rng, D, max(order), BUDGET["host"], hmax=10, wmax=140)
        out.append(dict(family="host", name=f"host{k}_{H}x{W}x{D}_ch{s['ch']}", H=H, W=W, D=D, channels=s["ch"], u8=s["u8"],
                        chunk=s["chunk"], sigmaC=float(rng.choice([10.0, 3.5])), sigmaS=float(rng.choice([30.0, 11.0])),
                        batches=_batches(rng, order)))
    return out


def _table():
    # one generator per family: a change to one family's rows leaves the others' as they are
    t = {f: b(np.random.default_rng([SEED, k])) for k, (f, b) in enumerate(
        (("pipeline", _pipeline), ("cblsm", _cblsm), ("crossagg", _crossagg), ("sad", _sad), ("ncc", _ncc), ("asw", _asw),
         ("host", _host)))}
    names = [g["name"] for f in FAMILIES for g in t[f]]
    assert len(set(names)) == len(names)
    return t


TABLE = _table()


def groups(family):
    return TABLE[family]


# ------------------------------------------------------------------------------------------------ images
_img_cache = {}


def is_constant_pair(L, R):
    """a pair with a constant image: its costs do not depend on the column, and its maps need not either"""
    return L.min() == L.max() or R.min() == R.max()


def _synth_pair(O, rng, H, W, D, noise, turn=0):
    """O.synth_pair.  Its disparity is D / 8 + (i / 8 % 7) (D / 16): it changes every 8 rows, never along a row, and not
    at all under 16 hypotheses.  So an image with fewer than 16 rows or hypotheses keeps only the right image -- the
    noise, or the texture plus a random offset of -50 .. 49 per column: the pipeline's scanline stage charges
    P2 / (gray step + 1) for a change of disparity, and on the plain texture, whose gray steps are small, that price
    flattens its whole map -- and gets a left image displaced by 1 .. min(D - 1, W / 4, 16) columns, in max(2, W / 24)
    segments of equal width whose neighbours differ: L[x] = R[x - g(x)], random bytes where x < g(x)."""
    Ds = max(1, min(D, W // 3))
    L, R = O.synth_pair(H, W, Ds, int(rng.integers(1, 2 ** 31)), noise)
    if H >= 16 and Ds >= 16:
        return L, R
    x = np.arange(W)
    if not noise:
        R = np.clip(R.astype(np.int32) + rng.integers(-50, 50, W)[None, :], 0, 255).astype(np.uint8)
    gmax = max(1, min(D - 1, W // 4, 16))
    nseg = max(2, W // 24)
    vals = [int(rng.integers(1, gmax + 1))]
    for _ in range(nseg - 1):
        v = int(rng.integers(1, gmax + 1))
        vals.append(v % gmax + 1 if v == vals[-1] else v)
    vals = [(v - 1 + turn) % gmax + 1 for v in vals]                    # batch k turns them by k: equal draws, other maps
    g = np.array(vals)[np.minimum(x * nseg // max(W, 1), nseg - 1)]
    L = np.where((x >= g)[None, :], R[:, np.maximum(x - g, 0)], rng.integers(0, 256, (H, W))).astype(np.uint8)
    return L, R


def by_construction_constant(family, g, m):
    """Whether map m of group g is constant whatever the images are: one hypothesis or one column leaves nothing to choose
    (every map is 0); an NCC interior that is empty leaves only border pixels (0); costAggregationV4 on one row has no
    vertical arms, so every rectangle is empty, every cost NaN and the map 0.  (Under tau = 0 that depends on the
    image -- arms still run over equal neighbours -- and is recorded per pair as v4_empty.)"""
    if g["D"] == 1 or g["W"] == 1:
        return True
    if family == "ncc":
        return g["H"] <= 2 * g["winSize"] or g["W"] <= 2 * g["winSize"]
    return m == "v4" and g["H"] == 1


def _maps_vary(g, O, L, R):
    """pipeline and CBLSM groups only: no map of the pair's oracle is constant (beyond by_construction_constant)"""
    o = (pipeline_pair(O, L, R, g["D"], g["fix_stride"]) if g["family"] == "pipeline" else cblsm_pair(O, L, R, g))[0]
    return all(o[m].min() != o[m].max() for m in MAPS[g["family"]]
               if not (by_construction_constant(g["family"], g, m) or (m == "v4" and o["v4_empty"])))


def gray_pairs(g, k, O):
    """The P gray pairs of batch k of group g, uint8 [H][W] each.  Pair 0 comes from _synth_pair (with noise in the odd
    batches), so that the WTA has real minima and the LR check meets every class; the others are drawn from _synth_pair
    with and without noise and from test_fuzz_gpu.rand_img (random, piecewise smooth, constant; each image on its own).
    The last pair of a batch has no constant image: the next batch is compared against it.  Two independent rand_img
    draws share no structure, and the smoothing stages of the pipeline and of CBLSM flatten a view of about a quarter
    of such pairs at these sizes: there a pair without a constant image is drawn again until no map of its oracle is
    constant."""
    key = (g["name"], k)
    if key not in _img_cache:
        b = g["batches"][k]
        rng = np.random.default_rng(b["seed"])
        H, W, D = g["H"], g["W"], g["D"]
        pairs, kinds = [], []
        for p in range(b["P"]):
            kind = (k % 2) if p == 0 else int(rng.integers(0, 4))
            if kind < 2:
                L, R = _synth_pair(O, rng, H, W, D, bool(kind), turn=k)
            else:
                for _ in range(200):
                    L, R = rand_img(rng, H, W), rand_img(rng, H, W)
                    if p == b["P"] - 1 and is_constant_pair(L, R):
                        L, R = (rng.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(2))
                    if g["family"] not in ("pipeline", "cblsm") or is_constant_pair(L, R) or _maps_vary(g, O, L, R):
                        break
                else:
                    raise AssertionError(("no rand_img pair with varying maps", g["name"], k, p))
            L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
            L.setflags(write=False)
            R.setflags(write=False)
            pairs.append((L, R))
            kinds.append(kind)
        _img_cache[key] = pairs
        _img_cache[key + ("kinds",)] = kinds
    return _img_cache[key]


def is_stereo_pair(g, k, p, O):
    """whether pair p of batch k is a synthetic stereo pair (a displaced copy), not two independent rand_img draws"""
    gray_pairs(g, k, O)
    return _img_cache[(g["name"], k, "kinds")][p] < 2


def bgr_pairs(g, k, O):
    """Colour pairs for CrossAggFlow and the BGR host feed: every gray pair plus 0 .. 2 per channel (test_fuzz_gpu's
    rule), and the gray pair the flows derive from them (O.bgr2gray).  -> list of (bgrL, bgrR, grayL, grayR)"""
    key = (g["name"], k, "bgr")
    if key not in _img_cache:
        rng = np.random.default_rng(g["batches"][k]["seed"] ^ 0x5A5A5A)
        out = []
        for L, R in gray_pairs(g, k, O):
            c = [np.clip(x[..., None].astype(np.int32) + rng.integers(0, 3, x.shape + (3,)), 0, 255).astype(np.uint8)
                 for x in (L, R)]
            out.append((c[0], c[1], O.bgr2gray(c[0]), O.bgr2gray(c[1])))
        _img_cache[key] = out
    return _img_cache[key]


# ------------------------------------------------------------------------------------------------ oracle compositions
def pipeline_pair(O, L, R, D, fix_stride):
    """oracle_pipeline of tests/test_post_batch_gpu.py with every intermediate kept, then main.cpp:93-94"""
    cl = O.adcensus_view(L, R, D, 10.0, 30.0, 0)
    cr = O.adcensus_view(L, R, D, 10.0, 30.0, 1)
    kw = dict(right_row_bug=False) if fix_stride else {}
    al, _ = O.aggregate_rect(cl, O.arms_all(L, **kw), 0)
    ar, _ = O.aggregate_rect(cr, O.arms_all(R, **kw), 0)
    so = O.scanline(al, L.astype(np.float32), 10, 150)
    raw, dr = O.wta(so), O.wta(ar)
    lr, cls, no, nm = O.lrcheck(raw, dr, 2)
    sp = O.remove_speckles(lr, 1, 30, INT_MIN)
    return (dict(raw=raw, dr=dr, lr=lr, cls=cls, counts=np.array([no, nm], np.int32), sp=sp, med=O.median(sp, 3)),
            dict(cost_left=cl, cost_right=cr, agg_left=al, agg_right=ar, scanline_sum=so))


def cblsm_tail(O, dL, dR, gate=5):
    """_chain of tests/test_cblsm_post_gpu.py: CBLSM.cpp:160-162 with smt_cblsm_post_default_params"""
    lr, cls, no, nm = O.lrcheck(dL, dR, gate)
    sp = O.remove_speckles(lr, 1, 50, INT_MIN)
    return dict(lr=lr, cls=cls, counts=np.array([no, nm], np.int32), sp=sp, fin=MC.oracle_inplace(sp, 3))


def v4_volume(vol, aL, aR, aUp, aDown):
    """cblsm_v4_cases.v4_numpy with the taps as the outer loops: for every (i, j, d) the same np.float32 adds in the same
    order (rows top in [-up, down) outer, columns left in [-L, R) inner), all hypotheses at once.  A tap outside the
    plane is an AssertionError, as there."""
    vol = np.asarray(vol, np.float32)
    H, W, D = vol.shape
    value = np.zeros((H, W, D), np.float32)
    number = np.zeros((H, W, D), np.int32)
    ii, jj = np.mgrid[0:H, 0:W]
    for top in range(-int(aUp.max(initial=0)), int(aDown.max(initial=0))):
        rows = (top >= -aUp) & (top < aDown)
        if not rows.any():
            continue
        for left in range(-int(aL.max(initial=0)), int(aR.max(initial=0))):
            m = rows & (left >= -aL) & (left < aR)
            if not m.any():
                continue
            i2, j2 = ii + top, jj + left
            inside = (i2 >= 0) & (i2 < H) & (j2 >= 0) & (j2 < W)
            assert not (m & ~inside[..., None]).any(), "costAggregationV4 tap outside the plane"
            src = vol[np.clip(i2, 0, H - 1), np.clip(j2, 0, W - 1)]
            value[m] = value[m] + src[m]
            number[m] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(number > 0, value / number.astype(np.float32), np.float32(np.nan)).astype(np.float32)


def cblsm_pair(O, L, R, g):
    D = g["D"]
    cl, cr, dl, dr = cblsm_oracle(O, L, R, D, maxlen=g["max_length"], sec=g["sec_length"], tau=g["tau"])
    arms = VC.oracle_arm_volumes(O, L, R, D, tau=g["tau"], sec=g["sec_length"], maxlen=g["max_length"])
    v4 = v4_volume(O.cblsm_ad(L, R, D, 0), *arms)
    # v4_empty: no rectangle of costAggregationV4 holds a tap (one row; or tau = 0 on an image without equal neighbours)
    out = dict(dl=dl, dr=dr, v4=VC.disp_origin(v4), v4_empty=np.array(np.isnan(v4).all()))
    out.update({"post_" + n: a for n, a in cblsm_tail(O, dl, dr).items()})
    return out, dict(pass1_left=cl, pass1_right=cr, v4=v4)


def crossagg_pair(O, bL, bR, gL, gR, g):
    """the composition of tests/test_crossagg_flow_gpu.py (CBLSM.cpp:133-143, 152, 160) on the oracle"""
    D = g["D"]
    p = dict(L1=g["L1"], L2=g["L2"], t1=g["t1"], t2=g["t2"], iters=g["num_iters"])
    _, vl = O.crossagg(bL, O.cblsm_ad(gL, gR, D, 0), **p)
    _, vr = O.crossagg(bR, O.cblsm_ad(gL, gR, D, 1), **p)
    dl, dr = O.wta(vl), O.wta(vr)
    lr, cls, no, nm = O.lrcheck(dl, dr, g["gate"])
    out = dict(dl=dl, dr=dr, lr=lr, cls=cls, counts=np.array([no, nm], np.int32))
    out.update({"post_" + n: a for n, a in cblsm_tail(O, dl, dr).items()})
    return out, dict(left=vl, right=vr)


def sad_pair(O, L, R, g):
    ws, D = g["winsize"], g["D"]
    Lp, Rp = O.pad_replicate(L, ws + 1), O.pad_replicate(R, ws + 1)
    dl, dr = O.sad(Lp, Rp, D, ws, 0), O.sad(Lp, Rp, D, ws, 1)
    last, cls = O.sad_crosscheck(dl, dr)
    return dict(dl=dl, dr=dr, last=last, cls=cls), {}


def ncc_pair(O, L, R, g):
    """O.ncc's map and costs, and the exact rational reference with its masks (exact_matchers.ncc_exact); an empty
    interior has no exact reference: every pixel is border"""
    win, D, H, W = g["winSize"], g["D"], g["H"], g["W"]
    disp, cost = O.ncc(L, R, D, win, want_cost=True)
    out = dict(disp=disp, cost=cost)
    if H > 2 * win and W > 2 * win:
        out["exact"], out["flat"], out["sentinel"] = X.ncc_exact(L, R, D, win)
    return out, {}


def asw_pair(O, L, R, g):
    ws, D = g["winSize"], g["D"]
    Lp, Rp = O.pad_replicate(L, ws + 1), O.pad_replicate(R, ws + 1)
    sp, cm = O.asw_masks(ws, ASW_SIGMA_SPACE, ASW_SIGMA_COLOR)
    dl, cl = O.asw(Lp, Rp, D, ws, sp, cm, ASW_T, 0, want_cost=True)
    dr, cr = O.asw(Lp, Rp, D, ws, sp, cm, ASW_T, 1, want_cost=True)
    out = dict(dl=dl, dr=dr, last=O.asw_crosscheck(dl, dr), Lp=Lp, Rp=Rp, cost_l=cl, cost_r=cr)
    for v, n in ((0, "exact_l"), (1, "exact_r")):
        out[n] = X.asw_exact(Lp, Rp, D, ws, sp, cm, ASW_T, v)
    return out, dict(cost_left=cl, cost_right=cr)


def host_pair(O, L, R, g):
    D = g["D"]
    dl = O.wta(O.adcensus_view(L, R, D, g["sigmaC"], g["sigmaS"], 0))
    dr = O.wta(O.adcensus_view(L, R, D, g["sigmaC"], g["sigmaS"], 1))
    if g["u8"]:
        dl, dr = dl.astype(np.uint8), dr.astype(np.uint8)
    return dict(dl=dl, dr=dr), {}


_oracle_cache = {}


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def oracle_batch(family, g, k, O):
    """-> (per-pair dicts, the last pair's volumes); computed once per process, read-only"""
    key = (family, g["name"], k)
    if key not in _oracle_cache:
        outs, vols = [], {}
        if family in ("crossagg",) or (family == "host" and g["channels"] == 3):
            pairs = bgr_pairs(g, k, O)
        else:
            pairs = gray_pairs(g, k, O)
        for pr in pairs:
            if family == "pipeline":
                o, vols = pipeline_pair(O, pr[0], pr[1], g["D"], g["fix_stride"])
            elif family == "cblsm":
                o, vols = cblsm_pair(O, pr[0], pr[1], g)
            elif family == "crossagg":
                o, vols = crossagg_pair(O, *pr, g)
            elif family == "sad":
                o, vols = sad_pair(O, pr[0], pr[1], g)
            elif family == "ncc":
                o, vols = ncc_pair(O, pr[0], pr[1], g)
            elif family == "asw":
                o, vols = asw_pair(O, pr[0], pr[1], g)
            elif family == "host":
                o, vols = host_pair(O, pr[2], pr[3], g) if g["channels"] == 3 else host_pair(O, pr[0], pr[1], g)
            else:
                raise KeyError(family)
            outs.append(_freeze(o))
        _oracle_cache[key] = (outs, _freeze(vols))
    return _oracle_cache[key]


# the disparity maps of a family's per-pair dict (what "the maps differ between batches" and "no map is constant" look at)
MAPS = dict(pipeline=("raw", "dr"), cblsm=("dl", "dr", "v4"), crossagg=("dl", "dr"), sad=("dl", "dr"), ncc=("disp",),
            asw=("dl", "dr"), host=("dl", "dr"))
