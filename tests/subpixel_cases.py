"""Sub-pixel disparities (csrc/subpixel_rule.h, include/smt.h "Sub-pixel disparities"): the rule restated in NumPy
float32, and the case table that tests/test_subpixel_cpu.py (host twin) and tests/test_subpixel_gpu.py (kernels) share.

The rule, for one cost row c[0..D) and min_den: w = the winner by smt_wta's rule (oracle.wta); w == 0 or w == D - 1 ->
(float)w; else s = (c[w-1] + c[w+1]) - 2 c[w], den = min_den < s ? s : min_den, off = (c[w-1] - c[w+1]) / (2 den), result
= isfinite(off) ? w + off : w.  One float32 operation per step.

The table: TABLE rows are (D, min_den, shape); volume(D, shape) is a prefix of pool(D), whose first rows are the
constructions below, one per row, and whose rest alternates random rows of the two scales:
  planted winners at 1, D - 2 and k C - 1, k C, k C + 1 (C = ceil(D / 64) hypotheses per lane: the neighbour sits in the
  next register, the next lane, or both), exact ties (c[w+1] == c[w]; two equal minima, the first wins), w = 0 and
  w = D - 1, NaN at d = 0 / w - 1 / w + 1 / everywhere, +inf at one / both neighbours / everywhere, negative costs,
  -0 against +0 both ways round, random costs in [0, 2) and integer-valued costs up to 181^2 255 (the SAD scale, where
  min_den = 1 does not clamp).
Shapes 1x1 (a planted mid-range winner), 5x7 and 37x53 (the last workgroup of four pixels is partial)."""
import numpy as np

DS = (1, 2, 3, 60, 64, 65, 128, 192, 200, 256, 257, 512)
MIN_DENS = (1.0, 2.0 ** -20, 64.0)
SHAPES = ((1, 1), (5, 7), (37, 53))
TABLE = [(D, m, s) for D in DS for m in MIN_DENS for s in SHAPES]
SAD_MAX = 181 * 181 * 255


def restate(O, vol, min_den):
    """the rule on a [H][W][D] float32 volume -> [H][W] float32"""
    vol = np.ascontiguousarray(vol, np.float32)
    H, W, D = vol.shape
    w = O.wta(vol).astype(np.int64)
    fw = w.astype(np.float32)
    if D < 3:
        return fw
    inner = (w > 0) & (w < D - 1)
    wi = np.clip(w, 1, D - 2)

    def take(idx):
        return np.take_along_axis(vol, idx[..., None], axis=2)[..., 0]

    c1, cm, c2 = take(wi - 1), take(wi), take(wi + 1)
    two, md = np.float32(2), np.float32(min_den)
    with np.errstate(all="ignore"):
        s = (c1 + c2) - two * cm
        den = np.where(md < s, s, md).astype(np.float32)
        off = (c1 - c2) / (two * den)
        res = np.where(np.isfinite(off), fw + off, fw).astype(np.float32)
    assert s.dtype == off.dtype == np.float32
    return np.where(inner, res, fw).astype(np.float32)


def planted_positions(D):
    C = (D + 63) // 64
    pos = {1, D - 2}
    for k in (1, 2, 31, 63):
        pos |= {k * C - 1, k * C, k * C + 1}
    return sorted(p for p in pos if 0 <= p < D)


def special_rows(D):
    """[(name, row)]: the constructions, each a float32 row of D costs"""
    rng = np.random.default_rng([7, D])
    base = lambda: (rng.random(D, dtype=np.float32) * np.float32(1.5) + np.float32(0.5)).astype(np.float32)   # [0.5, 2)
    mid = D // 2
    rows = []

    def add(name, r):
        rows.append((name, np.asarray(r, np.float32)))

    def plant(p, v=0.25, r=None):
        r = base() if r is None else r
        r[min(max(p, 0), D - 1)] = v
        return r

    add("planted-mid", plant(mid))                       # first: the 1x1 case
    for p in planted_positions(D):
        add(f"planted-{p}", plant(p))
    r = plant(mid); r[min(mid + 1, D - 1)] = 0.25; add("tie-next", r)
    r = plant(max(mid - 1, 0)); r[min(mid + 2, D - 1)] = 0.25; add("tie-apart", r)
    add("w-first", plant(0, 0.125)); add("w-last", plant(D - 1, 0.125))
    r = plant(mid); r[0] = np.nan; add("nan-at-0", r)
    r = plant(mid); r[max(mid - 1, 0)] = np.nan; add("nan-at-w-1", r)
    r = plant(mid); r[min(mid + 1, D - 1)] = np.nan; add("nan-at-w+1", r)
    add("all-nan", np.full(D, np.nan))
    r = plant(mid); r[max(mid - 1, 0)] = np.inf; add("inf-left", r)
    r = plant(mid); r[min(mid + 1, D - 1)] = np.inf; add("inf-right", r)
    r = plant(mid); r[max(mid - 1, 0)] = np.inf; r[min(mid + 1, D - 1)] = np.inf; r[mid] = 0.25; add("inf-both", r)
    add("all-inf", np.full(D, np.inf))
    add("negative", plant(mid, -5.0, base() - np.float32(3)))
    r = plant(max(mid - 1, 0), 0.0); r[min(mid + 1, D - 1)] = -0.0; add("zero-then-negzero", r)
    r = plant(max(mid - 1, 0), -0.0); r[min(mid + 1, D - 1)] = 0.0; add("negzero-then-zero", r)
    add("random", rng.random(D, dtype=np.float32) * np.float32(2))
    add("sad-scale", rng.integers(0, SAD_MAX + 1, D).astype(np.float32))
    r = rng.integers(0, SAD_MAX + 1, D).astype(np.float32); r[mid] = -1.0; add("sad-scale-planted", r)
    return rows


_POOLS = {}


def pool(D):
    """[37 * 53][D] float32: the constructions, then random rows of both scales"""
    if D not in _POOLS:
        n = SHAPES[-1][0] * SHAPES[-1][1]
        sp = np.stack([r for _, r in special_rows(D)])
        rng = np.random.default_rng([11, D])
        rest = n - len(sp)
        assert rest > 100
        rnd = rng.random((rest, D), dtype=np.float32) * np.float32(2)
        sad = rng.integers(0, SAD_MAX + 1, (rest, D)).astype(np.float32)
        rnd[1::2] = sad[1::2]
        p = np.concatenate([sp, rnd]).astype(np.float32)
        p.setflags(write=False)
        _POOLS[D] = p
    return _POOLS[D]


def volume(D, shape):
    H, W = shape
    return pool(D)[:H * W].reshape(H, W, D)


def nan_free(vol):
    return ~np.isnan(vol).any(axis=-1)


# ------------------------------------------------------------------------- rows for the bounds suite's rules
# The setters get their reasons in the bounds table on import, as tests/ncc_whole_cases.py does.  The two entries that
# take caller buffers are declared here in the table's own form (make(A, X, **params) -> (call, verify)) and run through
# run_case below by tests/test_subpixel_cpu.py (host twin) and tests/test_subpixel_gpu.py (device): the tables of
# tests/test_bounds_gpu.py and tests/test_stream_order_gpu.py are built when those files are collected, which is before
# this module is imported, so a row added to them from here would be decided and never run.
import ctypes as C  # noqa: E402

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402

BC.NOT_CALLER_BUFFER.update({
    "smt_subpixel_default_params": "host struct out", "smt_scanline_set_subpixel": "setter",
    "smt_crossarm_set_subpixel": "setter", "smt_pipeline_set_subpixel": "setter",
    "smt_wta_subpixel": "caller buffers: its rows are BOUNDS of tests/subpixel_cases.py, run by tests/test_subpixel_gpu.py "
                        "under the arena's rules, and that file holds it to the caller's busy stream",
    "smt_wta_subpixel_host": "host twin: the same rows on a host arena, run by tests/test_subpixel_cpu.py",
})


def wta_subpixel_entry(host):
    def f(A, X, H, W, D, min_den=1.0, null=False):
        vol = np.array(pool(D)[:H * W].reshape(H, W, D))
        A.inp("vol", vol); A.out("disp", (H, W), np.float32)

        def call():
            p = None if null else C.byref(X.L.SubpixelParams(min_den))
            if host:
                return X.lib.smt_wta_subpixel_host(A.ptr("vol"), H, W, D, p, A.ptr("disp"))
            return X.lib.smt_wta_subpixel(A.ptr("vol"), H, W, D, p, A.ptr("disp"), X.st())
        return call, lambda o: BC.bits_eq(o["disp"], restate(X.O, vol, min_den), "disp")
    return f


BOUNDS = [dict(H=1, W=9, D=1), dict(H=3, W=65, D=64, min_den=2.0 ** -20), dict(H=5, W=33, D=65), dict(H=2, W=17, D=257, min_den=64.0),
          dict(H=5, W=7, D=192, null=True), dict(H=1, W=1, D=512)]


def run_case(X, host, params):
    """bounds_cases.run_case for an entry that is not in its table: one call per prefill seed in a fresh arena (guards,
    inputs, status), the two outputs bit-identical, the first held to the restatement"""
    outs = []
    for seed in arena.SEEDS:
        A = arena.Arena(seed, X.device)
        call, verify = wta_subpixel_entry(host)(A, X, **params)
        A.build()
        rc = call()
        X.sync()
        assert rc == 0, (params, rc)
        outs.append((A.check(), verify))
    BC.assert_same(outs[0][0], outs[1][0], f"smt_wta_subpixel{params} depends on the prefill or on what lies beside its tensors")
    outs[0][1](outs[0][0])
