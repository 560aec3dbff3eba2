"""Case table of the aggregation placement / long-arm tests (test_agg_grid_cpu.py holds the table to the conditions the
GPU cases rely on, test_agg_grid_gpu.py runs it).  numpy only: nothing here needs a GPU or the library.

The geometry below restates, independently of csrc/crossarm.hip, what include/smt.h promises about the placement hooks:
which tile a wave owns per variant, how a requested strip width is rounded, and how many strips and bands of workgroup
rows an image then has."""
import numpy as np

VARIANTS = tuple(range(14))

# ---- host-only selftest sweep (smt_crossarm_selftest_grid) --------------------------------------------------------
SELFTEST_H = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 65, 70)
SELFTEST_W = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 70, 129, 137, 257, 260)
SELFTEST_WIDTHS = (0, 4, 8, 12, 16, 20, 32, 36, 64, 100)
SWEEPS = (0, 1)
MAX_STRIP_WIDTH = 4096

# ---- GPU placement cases ----------------------------------------------------------------------------------------------
PLACEMENT_SHAPES = ((1, 1, 5), (3, 5, 64), (5, 70, 100), (9, 137, 64), (37, 9, 7), (67, 131, 64), (33, 260, 192))
PLACEMENT_WIDTHS = (4, 8, 12, 16, 20, 32, 64, 100)
# (H, W, D, largest arm): arms <= 6 everywhere, one more case with the reference's own arm range
PLACEMENT_CASES = tuple(s + (6,) for s in PLACEMENT_SHAPES) + ((67, 131, 64, 34),)
OCCUPANCY_SHAPE = (67, 131, 64)
OCCUPANCY_VALUES = (0, 3, 4, 5)
OCCUPANCY_BAD = (1, 2, 6)
OCCUPANCY_VARIANTS = (3, 6, 10, 13)


def tile_shape(variant):
    """(rows, columns) of the pixel tile one wave owns; None for the one-pixel-per-wave walks (1, 2)."""
    if variant == 0:
        return (1, 4)
    if variant in (1, 2):
        return None
    if variant == 3:
        return (1, 8)
    return (2, 8) if variant <= 9 else (4, 4)


def default_width(variant):
    return 8 if variant >= 7 else 16


def effective_width(variant, requested):
    """Strip width the launch uses for smt_crossarm_set_strip_width(requested) (0: the variant's default)."""
    w = requested or default_width(variant)
    if variant == 0:
        return -(-w // 16) * 16
    if variant in (1, 2):
        return w
    return 8 if w <= 8 else 16 if w <= 16 else -(-w // 32) * 32


def geometry(variant, H, W, requested):
    """dict(SW, nstrips, wx, wy, nband) of a tiled variant (3 .. 13): a workgroup is wx x wy tiles, nband bands of
    workgroup rows cover the image."""
    th, tw = tile_shape(variant)
    SW = effective_width(variant, requested)
    wx = min(4, SW // tw)
    wy = 4 // wx
    return dict(SW=SW, nstrips=-(-W // SW), wx=wx, wy=wy, nband=-(-H // (wy * th)), th=th, tw=tw)


def placement_properties():
    """Which of the properties the placement table is there for occur in it, over shapes x variants x widths."""
    seen = set()
    for H, W, D in PLACEMENT_SHAPES:
        if W % 4:
            seen.add("W % 4 != 0")
        for v in VARIANTS:
            if tile_shape(v) is None or v == 0:
                continue
            for w in PLACEMENT_WIDTHS:
                g = geometry(v, H, W, w)
                if H < g["th"]:
                    seen.add("H < tile height")
                if W < g["tw"]:
                    seen.add("W < tile width")
                if g["nband"] < 8:
                    seen.add("nband < 8")
                if g["nband"] % 8:
                    seen.add("nband % 8 != 0")
                if g["nstrips"] > 8:
                    seen.add("nstrips > 8")
                if g["nstrips"] % 8:
                    seen.add("nstrips % 8 != 0")
    return seen


PLACEMENT_PROPERTIES = ("H < tile height", "W < tile width", "nband < 8", "nband % 8 != 0", "nstrips > 8",
                        "nstrips % 8 != 0", "W % 4 != 0")


# ---- inputs ---------------------------------------------------------------------------------------------------------
def random_arms(H, W, max_arm, seed):
    """Four int32 [H][W] maps, uniform in 0 .. max_arm and clamped to the plane: every rectangle stays inside the image."""
    rng = np.random.default_rng(seed)
    ii = np.arange(H)[:, None].repeat(W, 1)
    jj = np.arange(W)[None, :].repeat(H, 0)
    lim = (jj, W - 1 - jj, ii, H - 1 - ii)
    return [np.minimum(rng.integers(0, max_arm + 1, (H, W)), l).astype(np.int32) for l in lim]


def ordinary_volume(H, W, D, seed):
    """Finite, positive, one magnitude: every sum and every mean is an ordinary number, never a NaN."""
    rng = np.random.default_rng(seed)
    return (0.5 + 2.0 * rng.random((H, W, D), dtype=np.float32)).astype(np.float32)


def spread_volume(H, W, D, seed):
    """Positive values whose exponents run from -75 to 75: per value on the odd planes, one exponent per plane on the
    even ones (as test_aggregation_fast_quotient_is_the_ieee_quotient does, without the signs: the unwritten-pixel
    sentinel of the GPU tests is a NaN, which sums of non-negative finite values never are)."""
    rng = np.random.default_rng(seed)
    vol = (1.0 + rng.random((H, W, D))) * np.exp2(rng.integers(-75, 76, (H, W, D)).astype(np.float64))
    plane = np.exp2(rng.integers(-75, 76, D).astype(np.float64))
    vol[:, :, ::2] = (1.0 + rng.random((H, W, (D + 1) // 2))) * plane[::2]
    return vol.astype(np.float32)


def rect_area(arms):
    L, R, T, B = arms
    return (L.astype(np.int64) + R + 1) * (T.astype(np.int64) + B + 1)


# ---- long arms, case A: areas on both sides of 65535 / 65536 --------------------------------------------------------------
LONG_A_HW = (260, 262)
LONG_A_D = (64, 5)
# pixel (i, j) -> (left, right, top, bottom): 255 x 257, 256 x 256 and 257 x 257 (width x height) around the centre,
# 262 x 254 off-centre touching the left, right and top edges of the image
LONG_A_PIXELS = {
    (130, 130): (127, 127, 128, 128),
    (128, 131): (128, 127, 127, 128),
    (129, 132): (128, 128, 128, 128),
    (100, 40): (40, 221, 100, 153),
}


def long_a_arms():
    H, W = LONG_A_HW
    arms = random_arms(H, W, 6, 71)
    for (i, j), lens in LONG_A_PIXELS.items():
        for a, v in zip(arms, lens):
            a[i, j] = v
    return arms


# ---- long arms, case B: one bounding box of more than 2^24 positions ------------------------------------------------------
LONG_B_HWD = (4100, 4104, 1)
LONG_B_PIXEL = (2050, 2052)
LONG_B_ARM = 2048
LONG_B_VARIANTS = (13, 6, 2, 1)       # the kernels with the float index split, and the plain walk


def long_b_arms():
    H, W, _ = LONG_B_HWD
    arms = [np.zeros((H, W), np.int32) for _ in range(4)]
    for a in arms:
        a[LONG_B_PIXEL] = LONG_B_ARM
    return arms


def max_tile_box_width(arms, th, tw):
    """Widest bounding box (in columns) of the rectangles of one th x tw tile."""
    L, R = arms[0], arms[1]
    H, W = L.shape
    jj = np.arange(W)[None, :]
    lo, hi = jj - L, jj + R
    best = 0
    for r0 in range(0, H, th):
        for c0 in range(0, W, tw):
            best = max(best, int(hi[r0:r0 + th, c0:c0 + tw].max() - lo[r0:r0 + th, c0:c0 + tw].min() + 1))
    return best
