"""Shared by the in-place median tests: the maps, the oracle called with in == out, and the discrimination condition.

MedianFilter(d, d, ...) (PostProcessing.h:314-344) is a recurrence in raster order.  The expected bits come from the
oracle library called through ctypes with ONE pointer for `in` and `out` (oracle.median() allocates a separate output),
and from the reference build's ref_median called the same way where oracle/_ref exists.  orc_median sizes its buffer
wnd * wnd while the window holds (2 * (wnd / 2) + 1)^2 values, so it is never called with an even wnd: an even window
is compared against wnd + 1, the same arithmetic in the reference (:317-318: `size` only feeds reserve)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

_cache = {}


def rand_map(H, W, seed, pairs=None):
    """integers 0..59 with 15 % +inf"""
    rng = np.random.default_rng(seed)
    shp = (H, W) if pairs is None else (pairs, H, W)
    m = rng.integers(0, 60, shp).astype(np.float32)
    m[rng.random(shp) < 0.15] = np.inf
    return m


def odd(wnd):
    return wnd if wnd % 2 else wnd + 1


def oracle_inplace(m, wnd):
    """orc_median(p, p) on a copy of the [H][W] map (and ref_median(p, p), which must agree, where the reference build
    exists).  Cached per (bytes, wnd): computed once, shared, returned read-only."""
    m = np.ascontiguousarray(m, np.float32)
    H, W = m.shape
    key = (m.tobytes(), H, W, odd(wnd))
    if key not in _cache:
        a = m.copy()
        p = a.ctypes.data_as(C.c_void_p)
        O.lib().orc_median(p, p, W, H, odd(wnd))
        if O.have_ref_adcensus():
            b = m.copy()
            q = b.ctypes.data_as(C.c_void_p)
            assert O._ref(O._REF_ADC).ref_median(q, q, W, H, odd(wnd)) == 0
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "oracle and reference build disagree in place"
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def discriminates(m, wnd):
    """Whether the discrimination condition applies to this random map."""
    H, W = m.shape
    return H >= 5 and W >= 5 and wnd >= 3


def check_discrimination(m, wnd, got):
    """The in-place result differs from the out-of-place median in at least 20 % of the pixels (the reference alone:
    69-94 %), so a filter that reads only unfiltered, or only filtered, values cannot pass for the in-place one."""
    out_of_place = O.median(m, odd(wnd))
    frac = float(np.mean(got.view(np.uint32) != out_of_place.view(np.uint32)))
    assert frac >= 0.20, (m.shape, wnd, frac)
    return frac


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
