"""The bilateral image filter (include/smt_bilateral.h, csrc/bilateral_rule.h): the case table and
a NumPy restatement of ASW/BiliteralFilter.h:49-142 -- pad with mode='edge', loop over the taps in raster order, vectorise
over the pixels, one NumPy operation per reference operation.  float64 throughout: NumPy's add, multiply and divide round
once, so the restatement's sums are the reference's sums bit for bit up to the one step OpenCV owns, Mask / S, which has
the two forms of the header.  Shared by tests/test_bilateral_cpu.py and tests/test_bilateral_gpu.py; a plain helper module.

A window is (height, width) everywhere, as wsize_h, wsize_w of the C ABI."""
import functools
import math

import numpy as np

RECIPROCAL, DIVIDE = 0, 1
NORMS = (RECIPROCAL, DIVIDE)
DIRECT, STAGED = 1, 2

# H x W: tile (64 columns x 4 or 16 rows), wave and image edges inside the image and on its border
SHAPES = ((1, 1), (1, 70), (7, 1), (9, 33), (8, 32), (17, 65), (20, 31))
CHANNELS = (1, 3)
# (wsize, sigma_space, sigma_color); the two widest run on the 9 x 33 image only: the window is wider than the image and
# the whole halo is replicated
WINDOWS = (((1, 1), 10, 30), ((3, 3), 10, 30), ((5, 5), 10, 30), ((4, 6), 10, 30), ((3, 7), 10, 30), ((7, 3), 10, 30),
           ((23, 23), 10, 30), ((25, 25), 50, 25))
WIDE = (((63, 63), 10, 30), ((64, 64), 10, 30))
WIDE_SHAPE = (9, 33)

# flat image value, window, expected byte (sigma 10 / 30): the normalised weights add up to just under 1 and the
# truncation drops a grey level; the order of the sums decides where
FLAT = ((200, (4, 6), 199), (255, (23, 23), 254), (255, (5, 5), 254), (255, (1, 5), 254), (7, (23, 23), 6), (7, (7, 7), 6),
        (1, (3, 3), 0), (200, (23, 23), 200))
FLAT_SHAPE = (6, 9)


def masks(wsize, sigma_space, sigma_color):
    """getGausssianMask (:12-31) and getColorMask (:36-43) with math.exp; what smt_bilateral_masks must give within 1 ulp"""
    h, w = wsize
    ch, cw = (h - 1) // 2, (w - 1) // 2
    space = np.array([[math.exp(-(float((j - cw) ** 2) + float((i - ch) ** 2)) / (2 * sigma_space * sigma_space)) for j in range(w)]
                      for i in range(h)], np.float64)
    color = np.array([math.exp(-(i * i) / (2 * sigma_color * sigma_color)) for i in range(256)], np.float64)
    return space, color


def noise(H, W, C, seed):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    return a if C == 3 else a[:, :, 0]


def staircase(H, W, C):
    """four levels across the columns, 0 / 85 / 170 / 255: differences 0 and 255 reach both ends of the colour table; the
    channels of a colour image are rotated so that they differ"""
    levels = np.array([0, 85, 170, 255], np.uint8)
    row = levels[(np.arange(W) * 4) // max(W, 1)]
    a = np.repeat(row[None, :], H, 0)
    if C == 1:
        return a
    return np.stack([a, a[:, ::-1], np.roll(a, W // 3, 1)], -1).copy()


def flat(value, C):
    H, W = FLAT_SHAPE
    return np.full((H, W, C) if C == 3 else (H, W), value, np.uint8)


def restate_with(img, wsize, space, color, norm):
    """-> (dst uint8, acc float64), shaped like img.  space [h][w], color [256]."""
    img = np.asarray(img)
    a = img.reshape(img.shape[0], img.shape[1], -1)
    H, W, _ = a.shape
    h, w = wsize
    hh, ww = (h - 1) // 2, (w - 1) // 2
    P = np.pad(a, ((hh, hh), (ww, ww), (0, 0)), mode="edge").astype(np.int64)        # copyMakeBorder, :63
    centre = a.astype(np.int64)
    taps = [(r, c) for r in range(2 * hh + 1) for c in range(2 * ww + 1)]            # :71-72, raster order
    with np.errstate(all="ignore"):
        S = np.zeros(a.shape, np.float64)
        for r, c in taps:
            q = P[r:r + H, c:c + W]
            wt = color[np.abs(q - centre)] * space[r, c]                              # :78
            S = S + wt                                                                # :79
        rS = 1.0 / S
        acc = np.zeros(a.shape, np.float64)
        for r, c in taps:
            q = P[r:r + H, c:c + W]
            wt = color[np.abs(q - centre)] * space[r, c]
            wn = wt / S if norm == DIVIDE else wt * rS                                # :101, the MatExpr
            acc = acc + q.astype(np.float64) * wn                                     # :113
        v = np.where(acc < 0, 0.0, np.where(acc > 255, 255.0, acc))                   # :124-129
        dst = np.where(np.isnan(v), 0.0, np.trunc(v)).astype(np.uint8)                # :132; NaN -> 0, the decided defect
    return dst.reshape(img.shape), acc.reshape(img.shape)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def image(kind, H, W, C):
    """the table's images: 'noise', 'stairs' or ('flat', value); read-only, shared"""
    if kind == "noise":
        a = noise(H, W, C, 1000 * H + 10 * W + C)
    elif kind == "stairs":
        a = staircase(H, W, C)
    else:
        a = flat(kind[1], C)
    return _ro(np.ascontiguousarray(a))[0]


@functools.lru_cache(maxsize=None)
def tables(wsize, sigma_space, sigma_color):
    return _ro(*masks(wsize, sigma_space, sigma_color))


@functools.lru_cache(maxsize=None)
def restate(kind, H, W, C, wsize, sigma_space, sigma_color, norm):
    """the restatement of a table case, computed once per process"""
    space, color = tables(wsize, sigma_space, sigma_color)
    return _ro(*restate_with(image(kind, H, W, C), wsize, space, color, norm))


def windows_for(shape):
    return WINDOWS + (WIDE if tuple(shape) == WIDE_SHAPE else ())


def groups():
    """[(id, kind, H, W, C)]: every shape on 1 and 3 channels of noise (each runs windows_for(shape)), and the staircase on
    two shapes"""
    out = [(f"noise-{H}x{W}x{C}", "noise", H, W, C) for H, W in SHAPES for C in CHANNELS]
    out += [(f"stairs-{H}x{W}x{C}", "stairs", H, W, C) for H, W in ((9, 33), (17, 65)) for C in CHANNELS]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint8)


def first_diff(got, ref):
    bad = np.argwhere(bits(got) != bits(ref))
    return f"{len(bad)} of {got.size} differ; " + "; ".join(
        f"{tuple(int(x) for x in ix)}: got {got[tuple(ix)]!r}, want {ref[tuple(ix)]!r}" for ix in bad[:4])
