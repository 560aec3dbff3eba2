"""Case list and input generators of the reference pin (tests/test_ref_pin_cpu.py, tests/test_ref_pin_gpu.py,
`make_golden.py ref-pin`, `make -C oracle ref-asan`).  A plain module, not a conftest.

Every case is a dict: "kind", "name" and the parameters its generator needs.  inputs(case, O) regenerates the
inputs (O = oracle.oracle, used for the integer synthetic images only), run(case, inp, O, impl) computes the
outputs with the oracle (impl "oracle") or with the reference's own compiled code (impl "ref"), in one fixed
order of named arrays.  tests/golden/ref_pin_hashes.json holds the orc_fnv1a hashes of the inputs and of the
"ref" outputs.

Float outputs are hashed after every NaN is replaced by the one pattern 0x7fc00000 (canon): CPU and GPU NaNs
differ in sign and payload.

A case is admitted only where the reference is defined: admitted(case, inp, O) asks the oracle (no out-of-plane
read in the aggregation, no H > W with the right-arm stride bug, no overrun in FillTheHole).  Cases the reference
cannot run defined are left out here, not suppressed there.
"""
import numpy as np

INT_MIN = -(2 ** 31)
D_EDGES = (1, 5, 63, 64, 65, 100, 192, 255, 256, 257, 320, 512)


HOSTILE_LR = ((1, 1, 71, 0), (1, 9, 72, 1), (7, 1, 73, 2), (5, 300, 74, -1), (33, 77, 75, 1))     # (H, W, seed, gate)


def hostile_lr_maps(H, W, seed):
    """(dL, dR) float32 [H][W] for LeftRightConsistency: a valid integer base -- a third of the pixels consistent in both
    views, the rest random small integers -- plus sprinkles of what a disparity map is not supposed to hold: fractional
    parts .25 / .5 / .75 (the x.5 ties of j - d + 0.5 among them), negative disparities, -0.0, NaN, +-inf, +-3e9, 1e30, a
    denormal, in either map; left disparities that put col_right = (int)(j - d + 0.5) on -1, 0, W - 1 and W; right
    disparities that put col_rl = (int)(col_right + dR + 0.5) on 0, j, W - 1 and W."""
    rng = np.random.default_rng(seed)
    top = max(1, min(W, 12))
    dL = rng.integers(0, top, (H, W)).astype(np.float32)
    dR = rng.integers(0, top, (H, W)).astype(np.float32)
    jj = np.broadcast_to(np.arange(W), (H, W))
    ii = np.broadcast_to(np.arange(H)[:, None], (H, W))
    cr = jj - dL.astype(np.int64)
    ok = (cr >= 0) & (rng.random((H, W)) < 0.33)
    dR[ii[ok], cr[ok]] = dL[ok]                                           # consistent pixels
    special = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30, 1e-40, -0.0], np.float32)
    for m in (dL, dR):
        r = rng.random((H, W))
        frac = r < 0.12
        m[frac] += rng.choice(np.array([0.25, 0.5, 0.75], np.float32), int(frac.sum()))
        neg = (r >= 0.12) & (r < 0.18)
        m[neg] = -m[neg] - rng.choice(np.array([0.0, 0.5, 1.0, 1.5], np.float32), int(neg.sum()))
        sp = (r >= 0.18) & (r < 0.26)
        m[sp] = rng.choice(special, int(sp.sum()))
    # col_right on -1 (j - d + 0.5 = -1.5, and -1.0 exactly), 0 (from +0.5 and from -0.5: truncation toward zero), W - 1, W
    r = rng.random((H, W))
    for lo, hi, off in ((0.00, 0.02, 2.0), (0.02, 0.04, 1.5), (0.04, 0.06, 0.0), (0.06, 0.08, 1.0), (0.08, 0.10, 1.0 - W),
                        (0.10, 0.12, -float(W))):
        m = (r >= lo) & (r < hi)
        dL[m] = (jj[m] + off).astype(np.float32)
    # col_rl on 0, j, W - 1 and W: through pixels whose col_right is inside the row
    r = rng.random((H, W))
    with np.errstate(invalid="ignore"):
        c = np.trunc(jj.astype(np.float32) - dL + np.float32(0.5))
    inside = np.isfinite(c) & (c >= 0) & (c < W)
    for k, (lo, hi) in enumerate(((0.00, 0.04), (0.04, 0.08), (0.08, 0.12), (0.12, 0.16))):
        m = inside & (r >= lo) & (r < hi)
        cc = c[m].astype(np.int64)
        target = (np.zeros_like(cc), jj[m], np.full_like(cc, W - 1), np.full_like(cc, W))[k]
        # (a right disparity that leads back to j exactly is consistent; a quarter more still lands on j and is a
        # mismatch under the gates below 1, the only ones that can reach col_rl == j)
        dR[ii[m], cc] = (target - cc).astype(np.float32) + np.float32(0.25 if k == 1 else 0.0)
    return dL, dR


def d2i(x):
    """the oracle's orc_d2i on float64 values: truncation toward zero, INT_MIN where the value does not fit an int"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        fits = (x > -2147483649.0) & (x < 2147483648.0)
        return np.where(fits, np.trunc(np.where(fits, x, 0.0)), float(INT_MIN)).astype(np.int64)


def chain_counts(dL, dR, gate, after):
    """Over the pixels the LR check classifies through leftDisp[i][col_rl] with col_rl < j (PostProcessing.h:110-118): how
    many of those pixels col_rl had been rejected before (the reference reads the +inf it wrote there; smt_lrcheck
    recomputes that in lr_rejected), how many had not, and on how many the class depends on it.  `after`: the oracle's
    leftDisp after the check (+inf = rejected).  Also the sets of col_right and col_rl values met at the row ends."""
    H, W = dL.shape
    rejected = kept = decides = 0
    ends_cr, ends_crl = set(), set()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(H):
            for j in range(W):
                d = dL[i, j]
                if d == np.inf:
                    continue
                cr = int(d2i(np.float64(np.float32(j) - d) + 0.5))
                if cr in (-1, 0, W - 1, W):
                    ends_cr.add(cr)
                if not 0 <= cr < W:
                    continue
                dr = dR[i, cr]
                if not np.abs(d - dr) > np.float32(gate):
                    continue
                crl = int(d2i(np.float64(np.float32(cr) + dr) + 0.5))
                if crl in (0, W - 1, W) or crl == j:
                    ends_crl.add("j" if crl == j and crl not in (0, W - 1) else crl)
                if 0 < crl < j:
                    if after[i, crl] == np.inf:
                        rejected += 1
                        decides += not (dL[i, crl] > d)                 # without the chain: class 2; with it: class 1
                    else:
                        kept += 1
    return rejected, kept, decides, ends_cr, ends_crl


def smooth_img(H, W, seed, step=3):
    """piecewise-smooth image with long flat runs so arms pass 17 and the sticky threshold flips
    (the generator of tests/test_pipeline_gpu.py)"""
    rng = np.random.default_rng(seed)
    base = (np.add.outer(np.arange(H) // 9, np.arange(W) // 23) * 17) % 200 + 20
    return (base + rng.integers(0, step, (H, W))).astype(np.uint8)


def image(H, W, kind, seed, O):
    if kind == "synth":
        return O.synth_pair(H, W, 32, seed)[0]
    if kind == "noise":
        return O.synth_pair(H, W, 32, seed, True)[0]
    if kind == "smooth":
        return smooth_img(H, W, seed)
    return np.full((H, W), 77, np.uint8)


def canon(a):
    """NaN -> 0x7fc00000 in a float32 array (a copy); other dtypes pass through."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    a = a.copy()
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def hashes(arrays, O):
    return {k: "%016x" % O.fnv1a(canon(v)) for k, v in arrays.items()}


# ------------------------------------------------------------------------------------------------ case list
def _cases():
    c = []
    # AD-Census cost, both views + WTA.  D edges on small images (the reference rebuilds the 9x7 census for every
    # (i, j, d)); W < D, one row, one column.
    for k, D in enumerate(D_EDGES):
        H, W = (7, 40) if D <= 100 else (5, 24)
        c.append(dict(kind="adcensus", name=f"adc_D{D}", H=H, W=W, D=D, seed=20 + k, noise=bool(k & 1)))
    c += [dict(kind="adcensus", name="adc_row", H=1, W=37, D=16, seed=3, noise=False),
          dict(kind="adcensus", name="adc_col", H=23, W=1, D=5, seed=4, noise=True),
          dict(kind="adcensus", name="adc_px", H=1, W=1, D=3, seed=5, noise=True),
          dict(kind="adcensus", name="adc_mid", H=24, W=70, D=60, seed=6, noise=False)]

    # arms: ARM_CASES of tests/test_pipeline_gpu.py, main.cpp's order; 3-channel; single calls in other orders
    for (H, W, kind, seed) in [(72, 160, "synth", 3), (72, 160, "noise", 4), (64, 150, "smooth", 5),
                               (40, 200, "smooth", 6), (30, 64, "flat", 0)]:
        c.append(dict(kind="arms", name=f"arms_{kind}{seed}", H=H, W=W, img=kind, seed=seed, ch=1, tau=30,
                      dirs=(0, 1, 2, 3), single=False))
    c += [dict(kind="arms", name="arms_bgr", H=50, W=120, img="smooth", seed=9, ch=3, tau=30, dirs=(0, 1, 2, 3),
               single=False),
          dict(kind="arms", name="arms_square", H=41, W=41, img="smooth", seed=10, ch=1, tau=30, dirs=(0, 1, 2, 3),
               single=False),
          dict(kind="arms", name="arms_row", H=1, W=90, img="smooth", seed=11, ch=1, tau=30, dirs=(0, 1, 2, 3),
               single=False),
          # single calls: the threshold flips in whichever call comes first and stays for the later ones
          dict(kind="arms", name="arms_seq_3201", H=64, W=150, img="smooth", seed=5, ch=1, tau=30, dirs=(3, 2, 0, 1),
               single=True),
          dict(kind="arms", name="arms_seq_2", H=40, W=200, img="smooth", seed=6, ch=1, tau=30, dirs=(2,),
               single=True),
          dict(kind="arms", name="arms_seq_bgr_10", H=50, W=120, img="smooth", seed=9, ch=3, tau=30, dirs=(1, 0),
               single=True),
          dict(kind="arms", name="arms_seq_0123", H=64, W=150, img="smooth", seed=12, ch=1, tau=30,
               dirs=(0, 1, 2, 3), single=True)]

    # rectangle aggregation: AGG_CASES of tests/test_pipeline_gpu.py at reduced D where the plane count only
    # repeats work, plus the D edges on one small landscape image.  order 0 AggregationVertical, 2 Aggregation
    # (exclusive bounds), 1 costAggregationV5 (CBLSM build).
    agg = [(72, 160, 16, "synth", 3), (64, 150, 64, "smooth", 5), (72, 160, 100, "noise", 4),
           (48, 180, 192, "synth", 8), (50, 183, 128, "smooth", 9), (40, 200, 256, "flat", 0),
           (70, 155, 60, "smooth", 12), (66, 149, 7, "synth", 13)]
    agg += [(40, 90, D, "smooth", 30 + k) for k, D in enumerate(D_EDGES)]
    for (H, W, D, kind, seed) in agg:
        for order in (0, 1, 2):
            if order == 2 and D > 100:
                continue
            c.append(dict(kind="agg", name=f"agg{order}_{H}x{W}x{D}_{kind}{seed}", H=H, W=W, D=D, img=kind,
                          seed=seed, order=order))
    c.append(dict(kind="agg", name="agg1_portrait", H=96, W=61, D=22, img="smooth", seed=21, order=1))
    c.append(dict(kind="agg", name="agg2_square", H=41, W=41, D=12, img="smooth", seed=10, order=2))   # main.cpp's arms

    # scanline.  Inputs of kind "term" make every term of min(l1, l2, l3, l4) win often: costs uniform in
    # [0, 5) * scale, gray = 100 + 3 * randint(0, 4), small penalties.  (With p1 = 10 against costs in [0, 2), the
    # inputs of tests/test_pipeline_gpu.py, the neighbour terms l2 / l3 practically never win.)  `terms` marks the
    # cases that must meet TERM_SHARE: all of kind "term" with finite costs, except the shapes where a term cannot
    # win by construction -- D < 5 (at D = 1 both neighbours are pads), or a single row / column (a pass
    # without steps).  The shapes are SCAN_CASES of tests/test_pipeline_gpu.py, the D edges, W < D.
    def scan(name, H, W, D, seed, p1=1, p2=6, gen="term", scale=1.0, nonfinite=None):
        terms = gen == "term" and nonfinite is None and D >= 5 and H >= 3 and W >= 3
        c.append(dict(kind="scan", name=name, H=H, W=W, D=D, seed=seed, p1=p1, p2=p2, gen=gen, scale=scale,
                      nonfinite=nonfinite, terms=terms))
    for (H, W, D, seed) in [(20, 40, 16, 3), (12, 70, 64, 4), (9, 33, 100, 5), (10, 50, 192, 6), (7, 21, 256, 7),
                            (3, 5, 8, 8), (1, 9, 5, 9), (9, 1, 5, 10), (2, 2, 1, 11), (1, 1, 3, 12)]:
        scan(f"scan_{H}x{W}x{D}", H, W, D, seed)
    scan("scan_u2_12x70x64", 12, 70, 64, 4, p1=10, p2=150, gen="u2")          # the older inputs, once
    for k, D in enumerate(D_EDGES):
        H, W = (12, 40) if D <= 100 else (13, 24)
        scan(f"scan_D{D}", H, W, D, 40 + k)
    scan("scan_14x30x256", 14, 30, 256, 60)
    scan("scan_p2_10", 14, 30, 100, 61, p1=2, p2=10, scale=8.0)
    # the reference's own penalties (main.cpp:28-29), costs scaled so that p1 = 10 is comparable with their spread
    scan("scan_ref_penalties", 12, 40, 64, 62, p1=10, p2=150, scale=10.0)
    scan("scan_W_lt_D", 6, 9, 64, 63)
    # non-finite costs
    for k, (D, nf) in enumerate([(64, "nan_first_low"), (64, "nan_first_high"), (256, "nan_first_high"),
                                 (100, "nan_first_row"), (64, "interior"), (320, "interior"), (64, "inf_pixel"),
                                 (192, "inf_pixel")]):
        scan(f"scan_{nf}_D{D}", 11, 26, D, 70 + k, nonfinite=nf)

    # LR checks: the test_lrcheck cases, one row, one column
    for (H, W, seed, gate) in [(20, 60, 1, 2), (9, 200, 2, 1), (30, 31, 3, 5), (1, 50, 4, 2), (40, 1, 5, 1)]:
        c.append(dict(kind="lrcheck", name=f"lr_{H}x{W}", H=H, W=W, seed=seed, gate=gate))
        c.append(dict(kind="lrvariant", name=f"lrv_{H}x{W}", H=H, W=W, seed=seed, gate=gate))

    # the in-place LR check on hostile maps (hostile_lr_maps): fractions and x.5 ties, negative, non-finite and
    # out-of-int disparities, columns landing on -1, 0, W - 1 and W; the shapes and gates of
    # tests/test_consistency_hostile_gpu.py, one gate per shape here
    for (H, W, seed, gate) in HOSTILE_LR:
        c.append(dict(kind="lrcheck", name=f"lr_hostile_{H}x{W}", H=H, W=W, seed=seed, gate=gate, hostile=True))

    # FillTheHole: lists in LeftRightConsistency's own (row, col) form need row >= col to stay inside the swapped
    # extents; the generator draws pairs inside them
    for (row, col, D, seed, n_mis_extra) in [(40, 40, 16, 0, 20), (61, 37, 32, 1, 20), (37, 61, 32, 2, 20),
                                             (48, 100, 5, 3, 20), (33, 33, 1, 5, 20), (32, 48, 16, 12, None)]:
        c.append(dict(kind="fill", name=f"fill_{row}x{col}x{D}", row=row, col=col, D=D, seed=seed,
                      extra=n_mis_extra))

    for (H, W, seed, diff, area, inv) in [(60, 90, 1, 1, 30, INT_MIN), (60, 90, 2, 0, 5, INT_MIN),
                                          (60, 90, 3, 2, 80, INT_MIN), (60, 90, 1, 1, 30, 65535), (1, 70, 4, 1, 4, INT_MIN),
                                          (50, 1, 5, 1, 4, 65535)]:
        c.append(dict(kind="speckle", name=f"speckle_{H}x{W}_{seed}_{diff}_{area}_{inv & 0xffff}", H=H, W=W, seed=seed,
                      diff=diff, area=area, inv=inv))
    for (H, W, wnd) in [(37, 53, 1), (37, 53, 3), (37, 53, 5), (37, 53, 7), (1, 20, 3), (20, 1, 5), (2, 2, 7)]:
        c.append(dict(kind="median", name=f"median_{H}x{W}_{wnd}", H=H, W=W, seed=3, wnd=wnd))

    # CBLSM.h live functions
    for (H, W, kind, seed, ch) in [(72, 160, "synth", 3, 1), (64, 150, "smooth", 5, 1), (96, 61, "smooth", 21, 1),
                                   (50, 120, "smooth", 9, 3), (1, 80, "smooth", 7, 1), (60, 1, "smooth", 8, 1)]:
        c.append(dict(kind="cblsm_arms", name=f"cblsm_arms_{H}x{W}_{kind}{seed}_{ch}", H=H, W=W, img=kind, seed=seed,
                      ch=ch, tau=25))
    for k, D in enumerate(D_EDGES):
        c.append(dict(kind="cblsm_ad", name=f"cblsm_ad_D{D}", H=6, W=70, D=D, seed=80 + k))
        c.append(dict(kind="cblsm_disp", name=f"cblsm_disp_D{D}", H=9, W=31, D=D, seed=100 + k))
    c += [dict(kind="cblsm_ad", name="cblsm_ad_col", H=12, W=1, D=5, seed=95),
          dict(kind="cblsm_ad", name="cblsm_ad_20x70x60", H=20, W=70, D=60, seed=5)]
    for (H, W, D, seed) in [(40, 90, 16, 1), (33, 70, 64, 2), (25, 50, 100, 3), (12, 20, 257, 4)]:
        c.append(dict(kind="choose", name=f"choose_{H}x{W}x{D}", H=H, W=W, D=D, seed=seed))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = _cases()
TERM_SHARE = 0.02      # every term of min(l1, l2, l3, l4) that can win is the strict minimum at least this often


# ------------------------------------------------------------------------------------------------ inputs
def _scan_inputs(case):
    H, W, D = case["H"], case["W"], case["D"]
    rng = np.random.default_rng(case["seed"])
    if case["gen"] == "u2":
        cost = rng.random((H, W, D), dtype=np.float32) * 2
        gray = rng.integers(0, 256, (H, W)).astype(np.float32)
    else:
        cost = rng.random((H, W, D), dtype=np.float32) * np.float32(5.0 * case["scale"])
        gray = (100 + 3 * rng.integers(0, 4, (H, W))).astype(np.float32)
    nf = case["nonfinite"]
    if nf in ("nan_first_low", "nan_first_high"):
        # first pixel of every left-pass and right-pass line: the true minimum lies BEFORE the NaN
        dn = 2 if nf == "nan_first_low" else D - 3
        for x in (0, W - 1):
            cost[:, x, dn] = np.nan
            cost[:, x, 0] = -1.0            # smallest entry of the pixel, in front of the NaN
    elif nf == "nan_first_row":
        for y in (0, H - 1):               # first pixel of every up-pass and down-pass line
            cost[y, ::2, D // 2] = np.nan
            cost[y, ::2, 1] = -1.0
            cost[y, 1::2, D - 1] = np.nan   # NaN as the very last entry: nothing after it but the pad
    elif nf == "interior":
        for _ in range(10):
            i, j, d = int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1)), int(rng.integers(0, D))
            cost[i, j, d] = [np.nan, np.inf][int(rng.integers(0, 2))]
        cost[H // 2, W // 2, 0] = np.nan
        cost[H // 2 + 1, W // 3, D - 1] = np.inf
    elif nf == "inf_pixel":
        cost[H // 2, W // 2, :] = np.inf
        cost[1, W - 2, :] = np.inf
    return dict(cost=cost, gray=gray)


def _fill_inputs(case):
    row, col, D = case["row"], case["col"], case["D"]
    rng = np.random.default_rng(case["seed"])
    d = rng.integers(0, D, (row, col)).astype(np.float32)
    holes = rng.random((row, col)) < 0.12
    d[holes] = 65535
    d[rng.random((row, col)) < 0.02] = np.inf
    n = row * col

    def pairs(k):
        flat = rng.integers(0, n, k)
        return np.stack([flat // row, flat % row], 1).astype(np.int32)      # inside the swapped extents
    occ = pairs(50)
    if case["extra"] is None:
        mis = np.empty((0, 2), np.int32)                                   # third pass does not run
    else:
        mis = pairs(int(holes.sum()) + case["extra"])
        mis[len(mis) // 3, 0] = col // 2                                   # angle switch in the middle of the list
        mis[-1] = mis[0]                                                   # a duplicate: the later entry wins
    return dict(disp=d, occ=occ, mis=mis)


def inputs(case, O):
    k = case["kind"]
    if k == "adcensus":
        L, R = O.synth_pair(case["H"], case["W"], case["D"], case["seed"], case["noise"])
        return dict(L=L.astype(np.float32), R=R.astype(np.float32))
    if k in ("arms", "cblsm_arms"):
        g = image(case["H"], case["W"], case["img"], case["seed"], O)
        return dict(img=O.synth_bgr(g, 4) if case["ch"] == 3 else g)
    if k == "agg":
        H, W, D = case["H"], case["W"], case["D"]
        img = image(H, W, case["img"], case["seed"], O)
        vol = np.random.default_rng(case["seed"]).random((H, W, D), dtype=np.float32) * 2
        if case["order"] == 1:
            arms = O.arms_all(img, 25, 6, 17, 34, chain=False, right_row_bug=False)
        elif case["order"] == 2 and H != W:
            # with the stride bug's right-arm map some rectangles of the exclusive form are empty (0 / 0, counted
            # by the oracle as undefined): the arm maps are only an input here, so take them without it
            arms = O.arms_all(img, 30, 6, 17, 34, chain=True, right_row_bug=False)
        else:
            arms = O.arms_all(img)
        return dict(vol=vol, armL=arms[0], armR=arms[1], armT=arms[2], armB=arms[3])
    if k == "scan":
        return _scan_inputs(case)
    if k in ("lrcheck", "lrvariant"):
        H, W = case["H"], case["W"]
        if case.get("hostile"):
            dL, dR = hostile_lr_maps(H, W, case["seed"])
            return dict(dL=dL, dR=dR)
        rng = np.random.default_rng(case["seed"])
        dL = rng.integers(0, 24, (H, W)).astype(np.float32)
        dR = rng.integers(0, 24, (H, W)).astype(np.float32)
        if k == "lrcheck":
            dL[rng.random((H, W)) < 0.05] = np.inf          # already-invalid inputs (PostProcessing.h:90-93)
        return dict(dL=dL, dR=dR)
    if k == "fill":
        return _fill_inputs(case)
    if k == "speckle":
        H, W = case["H"], case["W"]
        rng = np.random.default_rng(case["seed"])
        d = (np.add.outer(np.arange(H) // 11, np.arange(W) // 13) * 3).astype(np.float32)
        d += rng.integers(0, 2, (H, W)).astype(np.float32)
        d[rng.random((H, W)) < 0.03] += 20
        d[rng.random((H, W)) < 0.04] = np.inf if case["inv"] == INT_MIN else 65535.0
        return dict(disp=d)
    if k == "median":
        H, W = case["H"], case["W"]
        rng = np.random.default_rng(case["seed"])
        d = rng.integers(0, 60, (H, W)).astype(np.float32)
        d[rng.random((H, W)) < 0.1] = np.inf
        return dict(disp=d)
    if k == "cblsm_ad":
        L, R = O.synth_pair(case["H"], case["W"], case["D"], case["seed"])
        return dict(L=L, R=R)
    if k == "cblsm_disp":
        rng = np.random.default_rng(case["seed"])
        vol = rng.integers(0, 7, (case["H"], case["W"], case["D"])).astype(np.float32)     # many ties
        vol[rng.random(vol.shape) < 0.01] = np.nan
        return dict(vol=vol)
    if k == "choose":
        row, col = case["H"], case["W"]
        rng = np.random.default_rng(case["seed"])
        jj = np.arange(col)[None, :].repeat(row, 0)
        ii = np.arange(row)[:, None].repeat(col, 1)
        r = lambda lim: np.minimum(rng.integers(0, 9, (row, col)), lim).astype(np.int32)
        return dict(LL=r(jj), LR=r(col - 1 - jj), RL=r(jj), RR=r(col - 1 - jj), LU=r(ii), LD=r(row - 1 - ii),
                    RU=r(ii), RD=r(row - 1 - ii))
    raise KeyError(k)


def admitted(case, inp, O):
    """False where the reference itself is undefined on the case (asked of the oracle)."""
    k = case["kind"]
    if k == "arms":
        return case["H"] <= case["W"] or 1 not in case["dirs"]
    if k == "agg":
        arms = [inp[n] for n in ("armL", "armR", "armT", "armB")]
        return O.aggregate_rect(inp["vol"], arms, case["order"])[1] == 0
    if k == "fill":
        try:
            O.fill_the_hole(inp["disp"], case["D"], inp["occ"], inp["mis"])
        except ValueError:
            return False
    return True


# ------------------------------------------------------------------------------------------------ run
def _pairs(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 2))


def run(case, inp, O, impl):
    """Outputs of one case as an ordered dict of arrays.  impl: "oracle" or "ref"."""
    k = case["kind"]
    ref = impl == "ref"
    if k == "adcensus":
        D = case["D"]
        if ref:
            vl, vr, dl, dr = O.ref_adcensus_both(inp["L"], inp["R"], D, 10.0, 30.0)
        else:
            vl = O.adcensus_view(inp["L"], inp["R"], D, 10.0, 30.0, 0)
            vr = O.adcensus_view(inp["L"], inp["R"], D, 10.0, 30.0, 1)
            dl, dr = O.wta(vl), O.wta(vr)
        return dict(volL=vl, volR=vr, dispL=dl, dispR=dr)
    if k == "arms":
        img, tau, dirs = inp["img"], case["tau"], case["dirs"]
        if ref and not case["single"]:
            maps, t = O.ref_arms_all(img, tau), -1
        elif ref and len(dirs) == 1:
            maps = [np.zeros(img.shape[:2], np.int32) for _ in range(4)]
            maps[dirs[0]], t = O.ref_arms_dir(img, dirs[0], tau)
        elif ref:
            maps, t = O.ref_arms_seq(img, tau, dirs)
        elif not case["single"]:
            maps = O.arms_all(img, tau, 6, 17, 34, chain=True, right_row_bug=True)
            t = -1
        else:
            maps = [np.zeros(img.shape[:2], np.int32) for _ in range(4)]
            t = tau
            for d in dirs:
                maps[d], t = O.arms_dir(img, d, t, out=maps[d])
        out = dict(armL=maps[0], armR=maps[1], armT=maps[2], armB=maps[3])
        if case["single"]:
            out["tau"] = np.array([t], np.int32)
        return out
    if k == "agg":
        arms = [inp[n] for n in ("armL", "armR", "armT", "armB")]
        order = case["order"]
        if not ref:
            out, oob = O.aggregate_rect(inp["vol"], arms, order)
            assert oob == 0
            return dict(out=out, disp=O.wta(out))
        if order == 1:
            out = O.ref_cblsm_aggregate_v5(inp["vol"], arms)
            return dict(out=out, disp=O.ref_cblsm_disp(out))
        out, disp = O.ref_aggregate_rect(inp["vol"], arms, order)
        return dict(out=out, disp=disp)
    if k == "scan":
        p1, p2 = case["p1"], case["p2"]
        if ref:
            return O.ref_scanline_all(inp["cost"], inp["gray"], p1, p2)
        o = {w: O.scan_pass(inp["cost"], inp["gray"], p1, p2, w) for w in ("left", "right", "up", "down")}
        o["sum"] = O.scanline(inp["cost"], inp["gray"], p1, p2)
        o["disp"] = O.wta(o["sum"])
        return o
    if k == "lrcheck":
        d, cls, no, nm = (O.ref_lrcheck if ref else O.lrcheck)(inp["dL"], inp["dR"], case["gate"])
        return dict(dL=d, cls=cls, counts=np.array([no, nm], np.int32))
    if k == "lrvariant":
        d, cls, no, nm = (O.ref_lrcheck_variant if ref else O.lrcheck_variant)(inp["dL"], inp["dR"], case["gate"])
        return dict(last=d, cls=cls, counts=np.array([no, nm], np.int32))
    if k == "fill":
        d, third = (O.ref_fill_the_hole if ref else O.fill_the_hole)(inp["disp"], case["D"], inp["occ"], inp["mis"])
        return dict(disp=d, mismatch=_pairs(inp["mis"] if third is None else third))
    if k == "speckle":
        f = O.ref_remove_speckles if ref else O.remove_speckles
        return dict(disp=f(inp["disp"], case["diff"], case["area"], case["inv"]))
    if k == "median":
        return dict(out=(O.ref_median if ref else O.median)(inp["disp"], case["wnd"]))
    if k == "cblsm_arms":
        if ref:
            maps = [O.ref_cblsm_arms_dir(inp["img"], d, case["tau"]) for d in range(4)]
        else:
            maps = [O.arms_dir(inp["img"], d, case["tau"], right_row_bug=False)[0] for d in range(4)]
        return dict(armL=maps[0], armR=maps[1], armT=maps[2], armB=maps[3])
    if k == "cblsm_ad":
        f = O.ref_cblsm_ad if ref else O.cblsm_ad
        return dict(left=f(inp["L"], inp["R"], case["D"], 0), right=f(inp["L"], inp["R"], case["D"], 1))
    if k == "cblsm_disp":
        return dict(disp=(O.ref_cblsm_disp if ref else O.wta)(inp["vol"]))
    if k == "choose":
        f = O.ref_choose_arm_length if ref else O.choose_arm_length
        D = case["D"]
        return dict(left=f(0, inp["LL"], None, inp["RL"], inp["RR"], D), right=f(1, inp["LR"], None, inp["RL"], inp["RR"], D),
                    up=f(2, inp["LU"], inp["RU"], inp["RL"], inp["RR"], D), down=f(3, inp["LD"], inp["RD"], inp["RL"], inp["RR"], D))
    raise KeyError(k)


# ------------------------------------------------------------------------------------------------ term shares
def term_shares(case, inp, paths):
    """Share of hypotheses in which each term of min(l1, l2, l3, l4) (ScanlineOptimizer.h:176-180, :237-241) is the
    STRICT minimum, per pass, counted from the path volumes `paths` (name -> [H][W][D]; the reference build's, or
    the oracle's where those are absent -- never the HIP output).  A small numpy restatement: the previous pixel's
    path costs are read from the volume, 65535 pads on both sides, and the step is recomputed and compared with
    the volume before anything is counted.  Returns {pass: (s1, s2, s3, s4)}."""
    p1 = np.float32(case["p1"])
    p2i = np.float32(case["p2"])
    gray = inp["gray"]
    res = {}
    for name in ("left", "right", "up", "down"):
        v = paths[name]
        c = inp["cost"]
        horiz = name in ("left", "right")
        if not horiz:
            v = v.transpose(1, 0, 2)                      # lines along axis 0, steps along axis 1
            c = c.transpose(1, 0, 2)
            g = gray.T
        else:
            g = gray
        if name in ("right", "down"):
            v = v[:, ::-1]
            c = c[:, ::-1]
            g = g[:, ::-1]
        prev = v[:, :-1].astype(np.float32)               # last path costs at every step
        if prev.shape[1] == 0:
            res[name] = (0.0, 0.0, 0.0, 0.0)
            continue
        pad = np.full(prev.shape[:2] + (1,), 65535.0, np.float32)
        ext = np.concatenate([pad, prev, pad], 2)
        mn = ext.min(2, keepdims=True)                    # finite inputs only (terms cases hold no NaN)
        if horiz:
            dg = np.abs(g[:, 1:] - g[:, :-1])
        else:
            # ScanLineUpDown compares with the line's FIRST pixel and steps the gray pointer by one ELEMENT
            # (:210, :221, :250): the restatement follows the flat index
            flat = gray.reshape(-1)
            H, W = gray.shape
            L = v.shape[0]
            first = (np.arange(L) if name == "up" else (H - 1) * W + np.arange(L))
            sgn = 1 if name == "up" else -1
            idx = first[:, None] + sgn * (1 + np.arange(v.shape[1] - 1))[None, :]
            dg = np.abs(flat[idx] - flat[first][:, None])
        p2 = np.maximum(p1, p2i / (dg.astype(np.float32) + np.float32(1)))[..., None]
        l1 = ext[..., 1:-1]
        l2 = (ext[..., :-2] + p1) if horiz else (ext[..., 1:-1] + p1)
        l3 = ext[..., 2:] + p1
        l4 = np.broadcast_to(mn + p2, l1.shape)
        t = np.stack([l1, l2, l3, l4])
        # the restatement reproduces the given path volume bit for bit, or the shares mean nothing
        again = c[:, 1:] + np.minimum(np.minimum(l1, l2), np.minimum(l3, l4)) - mn
        assert np.array_equal(again.view(np.uint32), np.ascontiguousarray(v[:, 1:]).view(np.uint32)), name
        n = l1.size
        out = []
        for k in range(4):
            others = np.delete(t, k, 0).min(0)
            out.append(float((t[k] < others).sum()) / n)
        res[name] = tuple(out)
    return res
