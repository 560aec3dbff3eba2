"""smt_median_filter_inplace_batch (api.MedianFilterInPlace) on the device: both formulations against the oracle called
with in == out, bit for bit, over the shape grid, batches whose maps lie further apart than H*W (guard elements
checked), the band seams and CBLSM.cpp's own size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import median_inplace_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

HS = (1, 2, 63, 64, 65, 130)
WS = (1, 2, 3, 4, 64, 65, 300)
GUARD = -123.0
NBASE = 5                       # distinct maps per shape; map b of a batch is base map b % NBASE


def _run(smt, maps, wnd, impl, gap=7):
    """maps [P][H][W] (numpy) -> filtered copies, run in one flat device buffer with `gap` guard elements after every
    map; asserts the guards come back untouched."""
    import torch
    P, H, W = maps.shape
    stride = H * W + gap
    host = np.full(P * stride, GUARD, np.float32)
    for b in range(P):
        host[b * stride:b * stride + H * W] = maps[b].ravel()
    buf = torch.from_numpy(host).to("cuda:0")
    view = buf.as_strided((P, H, W), (stride, W, 1))
    smt.median_inplace_set_impl(impl)
    try:
        assert smt.MedianFilterInPlace(view, wnd) is view
    finally:
        smt.median_inplace_set_impl(0)
    out = buf.cpu().numpy().reshape(P, stride)
    assert np.all(out[:, H * W:] == GUARD), "guard elements"
    return out[:, :H * W].reshape(P, H, W)


def _check(smt, base, P, wnd):
    maps = np.stack([base[b % len(base)] for b in range(P)])
    want = [MC.oracle_inplace(m, wnd) for m in base]
    got0, got1 = _run(smt, maps, wnd, 0), _run(smt, maps, wnd, 1)
    assert MC.same_bits(got0, got1), "impl 0 against impl 1"
    for b in range(P):
        assert MC.same_bits(got0[b], want[b % len(base)]), ("impl 0", maps.shape, wnd, b)
        assert MC.same_bits(got1[b], want[b % len(base)]), ("impl 1", maps.shape, wnd, b)
    return want


@pytest.mark.parametrize("wnd", (1, 3, 5, 7, 2, 4, 6))
def test_grid_against_oracle_in_place(smt, wnd):
    """H x W x pairs of the issue's grid; even windows against wnd + 1; the discrimination condition is asserted on the
    oracle's result wherever it applies."""
    for H in HS:
        for W in WS:
            base = [MC.rand_map(H, W, 7919 * H + 31 * W + k) for k in range(NBASE)]
            for P in (1, 3, 70):
                want = _check(smt, base[:min(P, NBASE)], P, wnd)
            if MC.discriminates(base[0], wnd):
                MC.check_discrimination(base[0], wnd, want[0])


@pytest.mark.parametrize("H,W", ((1025, 5), (2050, 9)))
def test_band_seams(smt, H, W):
    """Taller than a band under every radius: 1024-row bands plain; 1022, 1020 and 506 rows in the ring form."""
    m = MC.rand_map(H, W, H + W)
    for wnd in (3, 5, 7):
        _check(smt, [m], 1, wnd)
        MC.check_discrimination(m, wnd, MC.oracle_inplace(m, wnd))


def test_cblsm_cpp_size(smt):
    m = MC.rand_map(375, 450, 162)
    _check(smt, [m], 1, 3)
    MC.check_discrimination(m, 3, MC.oracle_inplace(m, 3))


def test_more_maps_than_workgroups_and_single_map_forms(smt):
    """1030 maps stride the grid of 1024 workgroups; [H][W] tensors and the constant / all-inf maps."""
    import torch
    base = [MC.rand_map(6, 7, 300 + k) for k in range(NBASE)]
    _check(smt, base, 1030, 3)
    for m in (MC.rand_map(9, 17, 1), np.full((9, 17), np.inf, np.float32), np.full((9, 17), 7.0, np.float32)):
        for wnd in (3, 5):
            t = torch.from_numpy(m.copy()).to("cuda:0")
            assert smt.MedianFilterInPlace(t, wnd) is t
            assert MC.same_bits(t.cpu().numpy(), MC.oracle_inplace(m, wnd))
    with pytest.raises(smt.SmtError):
        smt.MedianFilterInPlace(torch.zeros((4, 4), device="cuda:0"), 8)
