"""Aggregation placement, host side: the workgroup-to-pixel maps the kernels and launchers of csrc/crossarm.hip share are
enumerated by smt_crossarm_selftest_grid (no GPU), and the case table of test_agg_grid_gpu.py (agg_grid_cases.py) is held
to the conditions that keep those GPU tests from passing vacuously."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_grid_cases as G  # noqa: E402
import bounds_cases  # noqa: E402

SMT_OK, SMT_ERR_ARG, SMT_ERR_STATE = 0, -1, -6


def _lib():
    from stereo_match_traditional_amd._lib import lib
    return lib()


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_selftest_grid_every_pixel_owned_once(variant):
    """Every variant, 16 heights x 20 widths x 10 strip widths x both sweeps: each pixel has exactly one owner, no wave
    reaches past the image, strips and bands sit on their XCDs."""
    f = _lib().smt_crossarm_selftest_grid
    bad = [(H, W, w, s) for H in G.SELFTEST_H for W in G.SELFTEST_W for w in G.SELFTEST_WIDTHS for s in G.SWEEPS
           if f(variant, H, W, w, s) != SMT_OK]
    assert not bad, (variant, len(bad), bad[:8])


def test_selftest_grid_large_and_extreme_shapes():
    f = _lib().smt_crossarm_selftest_grid
    for variant in G.VARIANTS:
        for H, W, w in ((1080, 1920, 0), (1, 5000, 4096), (3000, 1, 4096), (4100, 4104, 0), (375, 1242, 100)):
            for s in G.SWEEPS:
                assert f(variant, H, W, w, s) == SMT_OK, (variant, H, W, w, s)


def test_selftest_grid_rejects_bad_arguments():
    f = _lib().smt_crossarm_selftest_grid
    assert f(13, 8, 8, 0, 0) == SMT_OK
    for args in ((-1, 8, 8, 0, 0), (14, 8, 8, 0, 0), (13, 0, 8, 0, 0), (13, 8, 0, 0, 0), (13, -3, 8, 0, 0),
                 (13, 8, 8, 0, 2), (13, 8, 8, 0, -1), (13, 8, 8, 2, 0), (13, 8, 8, 6, 0), (13, 8, 8, -4, 0),
                 (13, 8, 8, G.MAX_STRIP_WIDTH + 4, 0), (2, 8, 8, 1 << 20, 0), (13, 1 << 16, 1 << 16, 0, 0)):
        assert f(*args) == SMT_ERR_ARG, args
    assert f(2, 8, 8, G.MAX_STRIP_WIDTH, 0) == SMT_OK


def test_new_export_is_classified():
    assert bounds_cases.NOT_CALLER_BUFFER["smt_crossarm_selftest_grid"] == "host-only selftest"


def test_case_geometry_restates_the_header():
    """The table's own geometry (tile per variant, width rounding) against the values include/smt.h names."""
    assert [G.effective_width(13, w) for w in (0, 4, 8, 12, 16, 20, 32, 36, 64, 100)] == [8, 8, 8, 16, 16, 32, 32, 64, 64, 128]
    assert [G.effective_width(0, w) for w in (0, 4, 16, 20, 100)] == [16, 16, 16, 32, 112]
    assert G.effective_width(2, 12) == 12 and G.effective_width(6, 0) == 16 and G.effective_width(7, 0) == 8
    assert G.tile_shape(3) == (1, 8) and G.tile_shape(9) == (2, 8) and G.tile_shape(10) == (4, 4)
    g = G.geometry(13, 67, 131, 8)
    assert (g["wx"], g["wy"], g["nband"], g["nstrips"]) == (2, 2, 9, 17)


def test_placement_table_has_every_property():
    seen = G.placement_properties()
    assert seen == set(G.PLACEMENT_PROPERTIES), set(G.PLACEMENT_PROPERTIES) - seen


@pytest.mark.parametrize("case", G.PLACEMENT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_placement_cases_stay_inside_the_plane(O, case):
    H, W, D, max_arm = case
    arms = G.random_arms(H, W, max_arm, 100 + max_arm)
    assert max(int(a.max()) for a in arms) <= max_arm
    vol = np.zeros((H, W, 1), np.float32)
    for order in (0, 1):
        assert O.aggregate_rect(vol, arms, order)[1] == 0
    if max_arm == 34:
        # arms of the reference's own range: some tile's common box is wider than one 64-position batch, where the
        # per-axis membership tables give way to pixel-by-pixel classification
        for v in (3, 7, 13):
            th, tw = G.tile_shape(v)
            assert G.max_tile_box_width(arms, th, tw) > 64, v


def test_long_arm_case_a_areas(O):
    arms = G.long_a_arms()
    area = G.rect_area(arms)
    got = sorted(int(area[p]) for p in G.LONG_A_PIXELS)
    assert got == [65535, 65536, 257 * 257, 262 * 254]
    assert 65535 in got and 65536 in got and max(got) > 65536
    wh = sorted((int(arms[0][p] + arms[1][p] + 1), int(arms[2][p] + arms[3][p] + 1)) for p in G.LONG_A_PIXELS)
    assert wh == [(255, 257), (256, 256), (257, 257), (262, 254)]
    i, j = 100, 40                                     # the off-centre one touches the left, right and top edges
    assert j - arms[0][i, j] == 0 and j + arms[1][i, j] == G.LONG_A_HW[1] - 1 and i - arms[2][i, j] == 0
    mask = np.ones(G.LONG_A_HW, bool)
    for p in G.LONG_A_PIXELS:
        mask[p] = False
    assert int(area[mask].max()) <= 13 * 13
    vol = np.zeros(G.LONG_A_HW + (1,), np.float32)
    for order in (0, 1):
        assert O.aggregate_rect(vol, arms, order)[1] == 0


def test_long_arm_volumes_take_both_quotient_paths():
    """Variant 13 leaves its fast quotient when a pixel's sums leave [2^-60, 2^61) or its area exceeds 65535: the ordinary
    volume keeps every sum of the four long rectangles inside that range, the spread one does not."""
    H, W = G.LONG_A_HW
    for D in G.LONG_A_D:
        a = G.ordinary_volume(H, W, D, 5)
        assert a.min() >= 0.5 and a.max() < 2.5 and 0.5 * 65535 >= 2.0 ** -60 and 2.5 * 262 * 254 < 2.0 ** 61
        b = G.spread_volume(H, W, D, 6)
        assert np.isfinite(b).all() and b.min() > 0
        plane_max = b.reshape(-1, D).max(0).astype(np.float64)
        plane_min = b.reshape(-1, D).min(0).astype(np.float64)
        # a plane whose every sum is above the range, or whose every sum is below it, whatever the rectangle
        assert (plane_min * 65535 >= 2.0 ** 61).any() or (plane_max * 262 * 254 < 2.0 ** -60).any()
        assert float(plane_max.max()) * 262 * 254 < 3.0e38          # no sum overflows: no infinity, no NaN


def test_long_arm_case_b_box(O):
    H, W, D = G.LONG_B_HWD
    arms = G.long_b_arms()
    area = G.rect_area(arms)
    assert int(area.max()) == 4097 * 4097 > 1 << 24 and int((area > 1).sum()) == 1
    i, j = G.LONG_B_PIXEL
    assert i - G.LONG_B_ARM >= 0 and i + G.LONG_B_ARM < H and j - G.LONG_B_ARM >= 0 and j + G.LONG_B_ARM < W
    assert O.aggregate_rect(np.zeros((H, W, 1), np.float32), arms, 0)[1] == 0
