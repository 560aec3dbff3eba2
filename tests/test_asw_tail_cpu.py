"""The tail of ASW/ASWeight.cpp (:67-78) without a GPU: smt_fill_image_new_host (the rules of csrc/fill_image_rules.h on
host memory) against the loop-for-loop restatement of tests/asw_tail_cases.py, the restatements of the OpenCV steps
against independent formulations, the selection networks of csrc/median_net.h, argument rejection and exports."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import asw_tail_cases as TC  # noqa: E402

ERR_ARG = -1
FILL = TC.fill_maps()


@pytest.fixture(scope="module")
def L():
    from stereo_match_traditional_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def fill_refs():
    """computed once: name -> (faithful result, counts, classes), (fixed result, counts, classes)"""
    return {n: (TC.ref_fill(m, 0), TC.ref_fill(m, TC.FIX_ROW_END)) for n, m in FILL}


def host_fill(L, maps, fix, stride=0):
    H, W = maps[0].shape
    if stride:
        buf, stride = TC.batch_with_gaps(maps)
    else:
        buf = np.concatenate([m.reshape(-1) for m in maps]).copy()
    counts = np.full((len(maps), 2), -7, np.int32)
    rc = L.smt_fill_image_new_host(buf.ctypes.data, len(maps), stride, H, W, fix, counts.ctypes.data)
    assert rc == 0
    return buf, counts


def test_the_table_hits_every_class_in_faithful_mode(fill_refs):
    total = dict.fromkeys(TC.CLASSES, 0)
    for (faithful, _fixed) in fill_refs.values():
        for k, v in faithful[2].items():
            total[k] += v
    assert all(total[k] > 0 for k in TC.CLASSES), total


@pytest.mark.parametrize("fix", [0, TC.FIX_ROW_END])
@pytest.mark.parametrize("name,m", FILL, ids=[n for n, _ in FILL])
def test_host_fill_against_the_restatement(L, fill_refs, name, m, fix):
    want, counts, _ = fill_refs[name][1 if fix else 0]
    buf, got_counts = host_fill(L, [m], fix)
    assert np.array_equal(buf.reshape(m.shape), want)
    assert tuple(got_counts[0]) == counts


@pytest.mark.parametrize("name,m", FILL, ids=[n for n, _ in FILL])
def test_fixed_mode_gives_every_hole_its_own_value(L, fill_refs, name, m):
    buf, counts = host_fill(L, [m], TC.FIX_ROW_END)
    assert np.array_equal(buf.reshape(m.shape), TC.ref_fill_own(m))
    assert tuple(counts[0]) == (0, 0)
    assert fill_refs[name][1][1] == (0, 0)


def test_host_fill_batch_with_a_stride_gap(L, fill_refs):
    names = ["rand33x65d0.3", "rand33x65d0.6", "rand33x65d0.9"]
    maps = [dict(FILL)[n] for n in names]
    buf, counts = host_fill(L, maps, 0, stride=1)
    got, gaps = TC.split_with_gaps(buf, 3, 33, 65)
    assert np.all(gaps == TC.GUARD)
    for b, n in enumerate(names):
        assert np.array_equal(got[b], fill_refs[n][0][0]), n
        assert tuple(counts[b]) == fill_refs[n][0][1]


def test_counts_may_be_null(L):
    m = dict(FILL)["zero_rows_above_9"].copy()
    assert L.smt_fill_image_new_host(m.ctypes.data, 1, 0, 4, 7, 0, None) == 0
    assert np.array_equal(m, TC.ref_fill(dict(FILL)["zero_rows_above_9"])[0])


# ---------------------------------------------------------------------------------------------- the OpenCV restatements
def test_median_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7611)
    for (H, W) in TC.SHAPES[:6]:
        m = rng.integers(0, 256, (H, W)).astype(np.uint8)
        m[rng.random((H, W)) < 0.3] = 0
        for k in (3, 5):
            assert np.array_equal(TC.ref_median(m, k), ndi.median_filter(m, size=k, mode="nearest")), (H, W, k)


def test_median_networks_select_the_median(L):
    assert L.smt_median_blur_selftest_nets() == 0


def _rn(x, p, emin):
    """Fraction -> the nearest binary floating-point value of precision p (ties to even, gradual underflow below
    2^emin), as a Fraction"""
    num, den = x.numerator, x.denominator
    if num == 0:
        return Fraction(0)
    s, num = (-1 if num < 0 else 1), abs(num)
    e = num.bit_length() - den.bit_length()              # 2^e <= num / den < 2^(e + 1), after the correction
    if (num < (den << e)) if e >= 0 else ((num << -e) < den):
        e -= 1
    k = max(e, emin) - p + 1                             # the values around num / den are the multiples of 2^k
    n, d = (num, den << k) if k >= 0 else (num << -k, den)
    f, rem = divmod(n, d)
    if 2 * rem > d or (2 * rem == d and f % 2):
        f += 1
    return Fraction(s * f << k) if k >= 0 else Fraction(s * f, 1 << -k)


def _rn64(x):
    return _rn(x, 53, -1022)


def _rn32(x):
    return _rn(x, 24, -126)


def _round_half_even(x):
    f = x.numerator // x.denominator
    rem = x - f
    return f + 1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2) else f


def test_normalize_restatement_against_exact_rationals():
    """every (smin, smax) pair of a uint8 map: each of the rule's roundings done on exact rationals"""
    rows = TC.minmax_table()
    got = TC.ref_normalize_rows(rows)
    for row, g in zip(rows[::1], got):
        smin, smax = int(row.min()), int(row.max())
        scale = _rn64(255 * _rn64(Fraction(1, smax - smin)))
        shift = _rn64(-(_rn64(smin * scale)))
        sf, hf = _rn32(scale), _rn32(shift)
        for v, gv in zip(row, g):
            t = _rn32(_rn32(int(v) * sf) + hf)
            assert min(max(_round_half_even(t), 0), 255) == int(gv), (smin, smax, int(v))
    const = np.full((2, 3), 9, np.uint8)
    assert np.array_equal(TC.ref_normalize(const), np.zeros((2, 3), np.uint8))
    # the vectorised table form is the per-map form
    for i in range(0, rows.shape[0], 997):
        assert np.array_equal(TC.ref_normalize(rows[i:i + 1]), got[i:i + 1])


def test_speckle_restatement_on_the_crafted_map():
    m = TC.speckle_crafted(0)
    out = TC.ref_speckles(m, 0, 40, 2)
    assert out[1:6, 1:9].max() == 0 and np.all(out[1:6, 11:19] == 100) and out[6, 11] == 101      # 40 goes, 41 stays
    assert out[8:18, 1:11].max() == 0                                                             # diagonal: two of 25
    assert np.array_equal(out[21], m[21]) and out[23].max() == 0                                  # steps of 2 and 3
    assert out[25:31, 20:28].max() == 0 and np.all(out[25:66, 40] == 77) and out[30:34, 30:40].max() == 0


# ----------------------------------------------------------------------------------------------------- the C interface
def test_new_symbols_are_exported(L):
    for s in ("smt_minmax_normalize_u8_batch", "smt_minmax_normalize_f32_u8_batch", "smt_filter_speckles_u8_batch",
              "smt_median_blur_u8_batch", "smt_median_blur_selftest_nets", "smt_fill_image_new_batch",
              "smt_fill_image_new_host", "smt_asw_post_default_params", "smt_asw_tail_batch",
              "smt_asw_flow_run_batch_post", "smt_asw_flow_status"):
        assert hasattr(L, s), s
    import stereo_match_traditional_amd as smt
    from stereo_match_traditional_amd import shard
    for s in ("MinMaxNormalizeU8", "FilterSpecklesU8", "MedianBlurU8", "FillImageNew", "ASWTail", "ASW_FIX_FILL_ROW_END"):
        assert hasattr(smt, s), s
    assert hasattr(smt.ASWFlow, "run_post") and hasattr(smt.ASWFlow, "status") and hasattr(shard, "asw_post_batch")


def test_default_post_params(L):
    from stereo_match_traditional_amd._lib import ASWPostParams
    q = ASWPostParams()
    L.smt_asw_post_default_params(C.byref(q))
    assert (q.speckle_newval, q.speckle_max_size, q.speckle_max_diff, q.median_first, q.median_last, q.fix) == \
        (0, 40, 2, 5, 3, 0)


def test_argument_rejection(L):
    """SMT_ERR_ARG before any device work (there is no device here): NULLs, non-positive sizes, short strides,
    H*W >= 2^28, and each entry's own limits.  The pointers are never followed."""
    from stereo_match_traditional_amd._lib import ASWPostParams
    a = np.zeros(64, np.uint8)
    p, q = a.ctypes.data, a.ctypes.data + 32
    big = (1 << 14, 1 << 14)
    shapes_bad = [(0, 4), (4, 0), (-1, 4), big]

    def every(call):
        """call(in, out, pairs, stride, H, W) must reject each generic defect"""
        assert call(None, q, 1, 0, 2, 2) == ERR_ARG
        assert call(p, q, 0, 0, 2, 2) == ERR_ARG
        assert call(p, q, -1, 0, 2, 2) == ERR_ARG
        assert call(p, q, 2, 3, 2, 2) == ERR_ARG                       # stride below H*W
        for (H, W) in shapes_bad:
            assert call(p, q, 1, 0, H, W) == ERR_ARG, (H, W)

    every(lambda i, o, n, s, H, W: L.smt_minmax_normalize_u8_batch(i, o, n, s, H, W, None))
    assert L.smt_minmax_normalize_u8_batch(p, None, 1, 0, 2, 2, None) == ERR_ARG
    every(lambda i, o, n, s, H, W: L.smt_minmax_normalize_f32_u8_batch(i, o, n, s, H, W, None))
    assert L.smt_minmax_normalize_f32_u8_batch(p, None, 1, 0, 2, 2, None) == ERR_ARG
    every(lambda i, o, n, s, H, W: L.smt_filter_speckles_u8_batch(i, n, s, W, H, 0, 40, 2, None, None))
    every(lambda i, o, n, s, H, W: L.smt_median_blur_u8_batch(i, o, n, s, W, H, 3, None))
    assert L.smt_median_blur_u8_batch(p, None, 1, 0, 2, 2, 3, None) == ERR_ARG
    assert L.smt_median_blur_u8_batch(p, p, 1, 0, 2, 2, 3, None) == ERR_ARG          # in == out
    for k in (0, 1, 2, 4, 7):
        assert L.smt_median_blur_u8_batch(p, q, 1, 0, 2, 2, k, None) == ERR_ARG
    for fill in (lambda i, n, s, H, W, f: L.smt_fill_image_new_batch(i, n, s, H, W, f, None, None),
                 lambda i, n, s, H, W, f: L.smt_fill_image_new_host(i, n, s, H, W, f, None)):
        every(lambda i, o, n, s, H, W: fill(i, n, s, H, W, 0))
        assert fill(p, 1, 0, 1, 65536, 0) == ERR_ARG                                 # W > 65535
        assert fill(p, 1, 0, 2, 2, 2) == ERR_ARG                                     # unknown fix bit
    post = ASWPostParams()
    L.smt_asw_post_default_params(C.byref(post))

    def tail(i, n, s, H, W, pp=post):
        return L.smt_asw_tail_batch(i, n, s, H, W, C.byref(pp), None, None, None, None, None)
    assert tail(None, 1, 0, 2, 2) == ERR_ARG
    assert tail(p, -1, 0, 2, 2) == ERR_ARG
    assert tail(p, 2, 3, 2, 2) == ERR_ARG
    for (H, W) in shapes_bad:
        assert tail(p, 1, 0, H, W) == ERR_ARG
    assert tail(p, 1, 0, 1, 65536) == ERR_ARG
    for field, bad in (("median_first", 7), ("median_last", 1), ("fix", 4)):
        pp = ASWPostParams()
        L.smt_asw_post_default_params(C.byref(pp))
        setattr(pp, field, bad)
        assert tail(p, 1, 0, 2, 2, pp) == ERR_ARG, field
    assert L.smt_asw_flow_run_batch_post(None, p, p, 1, None, None, p, None, None, None, None, None, None) == ERR_ARG
    assert L.smt_asw_flow_status(None) == ERR_ARG
