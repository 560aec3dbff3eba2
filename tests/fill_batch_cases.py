"""Cases shared by tests/test_fill_batch_cpu.py and tests/test_fill_batch_gpu.py: LR-checked maps with their class maps,
the lists LeftRightConsistency would have produced from them, and the oracle's FillTheHole on those lists."""
import numpy as np
import pytest

HOLE = np.float32(65535.0)
UB_LIST, UB_THIRD = 1, 2
# (row, col, D): D is FillTheHole's ray length
SHAPES = [(40, 40, 16), (37, 61, 32), (64, 150, 24), (48, 100, 5), (1, 50, 4), (30, 45, 2), (33, 33, 1), (50, 70, 24),
          (90, 120, 12)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lr_case(O, row, col, seed, hole_frac=None):
    """dL: 7 x 9 blocks of constant disparity 1..7 with a seeded 8 % already invalid (+inf: mismatches, :90-93);
    dR = dL with a seeded 15 % redrawn; the oracle's LR check gives the map (+inf where rejected) and cls; then a
    seeded 0-10 % (or hole_frac) of the map becomes 65535.  Some 20 % of the pixels end as mismatches, so the third
    pass's holes stay below the mismatch count (the reference's defined behaviour)."""
    rng = np.random.default_rng(1000 + seed)
    i, j = np.mgrid[0:row, 0:col]
    dL = ((i // 7 + j // 9) % 7 + 1).astype(np.float32)
    dL[rng.random((row, col)) < 0.08] = np.inf
    dR = dL.copy()
    redraw = rng.random((row, col)) < 0.15
    dR[redraw] = rng.integers(0, 12, int(redraw.sum())).astype(np.float32)
    d, cls, _, _ = O.lrcheck(dL, dR, 2)
    frac = rng.uniform(0.0, 0.10) if hole_frac is None else hole_frac
    d[rng.random((row, col)) < frac] = HOLE
    return d, cls


def lists(cls):
    """LeftRightConsistency's two vectors: the class pixels in row-major order."""
    return np.argwhere(cls == 1).astype(np.int32), np.argwhere(cls == 2).astype(np.int32)


def expected(O, d, cls, D):
    """(filled map, status) of the oracle on the lists of cls."""
    occ, mis = lists(cls)
    ref, third = O.fill_the_hole(d, D, occ, mis)
    return ref, [len(occ), len(mis), -1 if third is None else len(third), 0], third


def aliased(cls):
    """Number of list entries whose address i*row + j another entry of the same list also has."""
    row, col = cls.shape
    n = 0
    for k in (1, 2):
        ij = np.argwhere(cls == k)
        a = ij[:, 0] * row + ij[:, 1]
        _, cnt = np.unique(a, return_counts=True)
        n += int(cnt[cnt > 1].sum())
    return n


def mids(cls, third):
    """(mid_0, mid_1, mid_2): a class-1 / class-2 pixel in image row col/2, a third-pass hole on line col/2."""
    row, col = cls.shape
    m = col // 2
    in_row = lambda k: bool(m < row and (cls[m] == k).any())
    return in_row(1), in_row(2), bool(third is not None and len(third) and (third[:, 0] == m).any())


def mid_case(O, which):
    """50 x 70 (col/2 = 35 < row): `which` = 0 keeps class 1 but no class 2 in row 35 (mid_0 only), 1 the other way
    round (mid_1 only), 2 clears both and leaves a hole on line 35 of the swapped view that no target writes (a switch
    in pass 2 only)."""
    row, col, D = 50, 70, 24
    d, cls = lr_case(O, row, col, 40 + which, 0.05)
    m = col // 2
    if which == 0:
        cls[m][cls[m] == 2] = 0
        cls[m, 3] = 1
    elif which == 1:
        cls[m][cls[m] == 1] = 0
        cls[m, 3] = 2
    else:
        cls[m] = 0
        a = m * row + 7                                  # address on line 35 of the swapped view
        for i in range(row):                             # no class pixel (i, j) may have this address
            if 0 <= a - i * row < col:
                cls[i, a - i * row] = 0
        d.reshape(-1)[a] = HOLE
    return d, cls, D


def batch_of_five(O, row, col, seed):
    maps, clss = [], []
    for b in range(3):
        d, cls = lr_case(O, row, col, seed + b)
        maps.append(d); clss.append(cls)
    d, cls = lr_case(O, row, col, seed + 3, 0.05)
    maps.append(d); clss.append(np.zeros_like(cls))                          # nothing to do
    d, cls = lr_case(O, row, col, seed + 4, 0.05)
    cls[cls == 2] = 0                                                        # n_mis == 0: pass 2 is skipped (:174)
    maps.append(d); clss.append(cls)
    return maps, clss


def portrait_batch(O):
    """61 x 37: pair 1 has class pixels in rows >= 37, whose address i*61 + j leaves the buffer; its neighbours do not."""
    row, col = 61, 37
    maps, clss = [], []
    for b in range(3):
        d, cls = lr_case(O, row, col, 500 + b, 0.04)
        if b != 1:
            cls[col:] = 0
        maps.append(d); clss.append(cls)
    return maps, clss, 16


def third_overrun_batch(O):
    """40 x 40: pair 1 keeps three mismatches against some 80 holes."""
    row, col = 40, 40
    maps, clss = [], []
    for b in range(3):
        d, cls = lr_case(O, row, col, 600 + b, 0.05)
        if b == 1:
            keep = np.argwhere(cls == 2)[[3, 40, 90]]
            cls[cls == 2] = 0
            cls[keep[:, 0], keep[:, 1]] = 2
        maps.append(d); clss.append(cls)
    return maps, clss, 16


def check_third_overrun(O, d, cls, D, got, st):
    """got must be the oracle's map after passes 0 and 1.  The oracle is run with the last mismatch repeated until the
    list is long enough for pass 2 to stay in bounds: a repeated last entry is filled with the same value at the same
    address under the same angle set, so passes 0 and 1 are unchanged, and pass 2 then replaces the holes and nothing
    else.  Compared: every pixel that is not a hole after pass 1."""
    occ, mis = lists(cls)
    with pytest.raises(ValueError):
        O.fill_the_hole(d, D, occ, mis)
    holes = got == HOLE
    n_holes = int(holes.sum())
    assert n_holes > len(mis)
    assert st.tolist() == [len(occ), len(mis), n_holes, UB_THIRD]
    padded = np.concatenate([mis, np.repeat(mis[-1:], n_holes, 0)])
    ref, third = O.fill_the_hole(d, D, occ, padded)
    assert len(third) == n_holes and np.array_equal(third[:, 0] * cls.shape[0] + third[:, 1],
                                                   np.flatnonzero(holes.reshape(-1)))
    assert np.array_equal(bits(got)[~holes], bits(ref)[~holes])
    assert (bits(got) != bits(d)).sum() > 0


FULL = (1080, 1920, 192)


def full_size_inputs(b):
    """Pair b of the 1920 x 1080 case: (dL, dR, rng) before the LR check; 5 % of dL already invalid, 15 % of dR redrawn."""
    row, col, _ = FULL
    rng = np.random.default_rng(70 + b)
    i, j = np.mgrid[0:row, 0:col]
    dL = ((i // 37 + j // 53 + b) % 23 + 2).astype(np.float32)
    dL[rng.random((row, col)) < 0.05] = np.inf
    dR = dL.copy()
    redraw = rng.random((row, col)) < 0.15
    dR[redraw] = rng.integers(0, 64, int(redraw.sum())).astype(np.float32)
    return dL, dR, rng
