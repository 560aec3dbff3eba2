"""Volumes of 4 GiB to 8 GiB held to the oracle through periodic inputs: the case table, the input builders, the oracle
compositions and the comparison helpers of test_large_volume_cpu.py (which proves the method on the oracle alone, at
small sizes) and test_large_volume_gpu.py (which runs the table).  Nothing here needs a GPU or the library: numpy, and
torch on whatever device the tensors handed in live on.

The method.  Every volume stage is local along at least one image axis.  The large input is K copies of a small block
along that axis, so the output is block-periodic except for the first and the last block, which see the image edge.
  * every element, on the device: block 1 is compared with each of blocks 2 .. K-2 (integer views of the same width,
    in pieces of at most CHUNK bytes); outputs are prefilled with 0xFF bytes, so an unwritten element differs;
  * bit for bit against the oracle: blocks 0, 1 and K-1 are the oracle's, from a problem of two or three blocks (the
    rows [0, 2 h0) and [H - h0, H) of the full image where the oracle takes a row range, else the three-block problem
    [P; P; P]).
Stages whose lines along the periodic axis are independent (the scanline passes) have no edge block: every block is the
oracle's.

Aliasing.  An addressing error that wraps by 2^32 bytes must not land on identical data.  A block of h0 W D elements
with an odd factor is never a divisor of 2^29, 2^30 or 2^31 elements, W D with an odd factor puts each of these
thresholds strictly inside a row, and every row of a block holds different values from a seeded generator
(test_large_volume_cpu.py asserts all three per case)."""
import collections
import functools

import numpy as np
import torch

GiB = 1 << 30
W, H0, W0 = 517, 13, 11                            # 517 = 11 * 47: a narrow image, a block the oracle evaluates in a second
K_A, K_B, K_C = 624, 625, 1249                     # blocks of H0 rows at D = 256: 3.9996 GiB, 4.0060 GiB, 8.0056 GiB
THRESHOLDS = (1 << 29, 1 << 30, 1 << 31)           # elements: 4 GiB of float64; 4 GiB of float32 = 8 GiB of float64; 8 GiB
CHUNK = 256 << 20                                  # bytes of one compared piece (its temporaries stay below 1 GiB)
EXTRA = 2 * GiB                                    # comparison pieces and expected blocks, beside the volumes
PER_PIXEL = 160                                    # images, maps, arm maps and the handles' per-pixel planes, bytes
LIMIT = 32 * GiB
HEADROOM = 2 * GiB                                 # a case skips only below device_bytes + HEADROOM of free memory
MAX_ARM = 4
P1, P2 = 10, 150
SIGMA_C, SIGMA_S = 10.0, 30.0
VARIANTS = tuple(range(14))

# regime: what H W D 4 bytes reaches
#   A  the largest under 2^32 bytes with H a multiple of h0: the tuned aggregation kernels, 32-bit byte offsets of the taps
#      with the top bit set in the second half of the volume, the buffer resource at its widest
#   B  the smallest at or above 2^32 bytes with H a multiple of h0: the plain walk, whatever set_variant asked for
#   C  just above 2^31 elements: element indices past int, byte offsets past 2^32, both crossed inside one launch
Case = collections.namedtuple("Case", "id stage regime H W D h0 w0 axis itemsize volumes params")


def _case(id, stage, regime, H, D, axis="rows", itemsize=4, volumes=2, **params):
    return Case(id, stage, regime, H, W, D, H0, W0, axis, itemsize, volumes, params)


def _table():
    t = []
    HA, HB, HC = H0 * K_A, H0 * K_B, H0 * K_C
    # smt_crossarm_aggregate with smt_crossarm_load_arm_maps, the fused WTA map on, arms <= 4
    for v in VARIANTS:
        for o in (0, 1):
            t.append(_case(f"agg-A-v{v}-o{o}", "agg", "A", HA, 256, variant=v, order=o))
    t.append(_case("agg-A-o2", "agg", "A", HA, 256, variant=None, order=2))
    for o in (0, 1):
        t.append(_case(f"agg-A-D250-o{o}", "agg", "A", H0 * 639, 250, variant=None, order=o))      # ragged D, 3.9997 GiB
    for v in (13, 6):
        for o in (0, 1):
            t.append(_case(f"agg-B-v{v}-o{o}", "agg", "B", HB, 256, variant=v, order=o))
    for o in (0, 1):
        t.append(_case(f"agg-C-o{o}", "agg", "C", HC, 256, variant=None, order=o))
    # smt_adcensus_compute, both views and maps; two-pair batches with the volumes lent beforehand / deferred
    t.append(_case("adc-C-D256", "adc", "C", HC, 256, mode="compute"))
    t.append(_case("adc-C-D512", "adc", "C", H0 * K_B, 512, mode="compute"))        # the table-lookup kernel, half the pixels
    t.append(_case("adc-C-batch-lent", "adc", "C", HC, 256, mode="lent"))
    t.append(_case("adc-C-batch-deferred", "adc", "C", HC, 256, mode="deferred"))
    # smt_wta
    t.append(_case("wta-C-D256", "wta", "C", HC, 256, volumes=1))
    t.append(_case("wta-C-D250", "wta", "C", H0 * 1279, 250, volumes=1))
    # smt_scanline_pass 0 .. 3 (2 / 3 faithful and under SMT_QUIRK_FIX_SCAN_VERTICAL), smt_scanline_run with its WTA
    for p in (0, 1):
        t.append(_case(f"scan-C-pass{p}", "scan_rows", "C", HC, 256, scan_pass=p))
    for p in (2, 3):
        for fixed in (False, True):
            t.append(_case(f"scan-C-pass{p}-{'fixed' if fixed else 'faithful'}", "scan_cols", "C", HC, 256, axis="cols",
                           scan_pass=p, fixed=fixed))
    t.append(_case("scan-C-run", "scan_run", "C", HC, 256, axis="both", volumes=3))
    # smt_cblsm_ad, both views
    for view in (0, 1):
        t.append(_case(f"cblsm-ad-C-view{view}", "cblsm_ad", "C", HC, 256, volumes=1, view=view))
    # smt_ncc with costs (float64), 3 x 3: V just above 2^29 (the volume crosses 4 GiB) and just above 2^30 (8 GiB)
    for impl in (2, 3):
        t.append(_case(f"ncc-4GiB-impl{impl}", "ncc", "ncc4", H0 * 313, 256, itemsize=8, volumes=1, impl=impl, win=1))
        t.append(_case(f"ncc-8GiB-impl{impl}", "ncc", "ncc8", H0 * K_B, 256, itemsize=8, volumes=1, impl=impl, win=1))
    # smt_sad_both with costL, 3 x 3
    t.append(_case("sad-C", "sad", "C", HC, 256, volumes=1, winsize=0))
    return tuple(t)


CASES = _table()


def elements(c):
    return c.H * c.W * c.D


def device_bytes(c):
    """Bytes the case holds on the device at its peak: its full-size volumes (inputs, outputs, a handle's own), the
    per-pixel planes, and EXTRA for the compared pieces and the expected blocks."""
    return c.volumes * elements(c) * c.itemsize + PER_PIXEL * c.H * c.W + EXTRA


def period_elements(c):
    """Elements after which the case's data repeats along the flat output index (the in-row period for columns)."""
    return c.w0 * c.D if c.axis == "cols" else c.h0 * c.W * c.D


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def image_block(h0, w, seed):
    """uint8 [h0][w] noise: every row different (checked by rows_differ)."""
    return _rng(seed, h0, w).integers(0, 256, (h0, w)).astype(np.uint8)


def cost_block(shape, seed, levels=None):
    """float32 costs: ordinary positive numbers of one magnitude (every sum an ordinary number), or with `levels` small
    integers, so that a minimum is tied several times per pixel."""
    r = _rng(seed, *shape)
    if levels:
        return r.integers(0, levels, shape).astype(np.float32)
    return (0.5 + 2.0 * r.random(shape, dtype=np.float32)).astype(np.float32)


def arm_block(h0, w, seed, lo=1, hi=MAX_ARM):
    """Four int32 [h0][w] maps (left, right, top, bottom) in lo .. hi, the horizontal ones clipped to the row: the same
    in every block.  lo = 1 keeps the exclusive rectangles of order 2 non-empty."""
    r = _rng(seed, h0, w)
    jj = np.arange(w)[None, :]
    a = [r.integers(lo, hi + 1, (h0, w)).astype(np.int32) for _ in range(4)]
    a[0] = np.minimum(a[0], jj).astype(np.int32)
    a[1] = np.minimum(a[1], w - 1 - jj).astype(np.int32)
    return a


def tile_rows(a, K):
    return np.ascontiguousarray(np.tile(a, (K,) + (1,) * (a.ndim - 1)))


def tile_cols(a, K):
    return np.ascontiguousarray(np.tile(a, (1, K) + (1,) * (a.ndim - 2)))


def full_arms(block_arms, K):
    """The block's maps K times down the rows, the vertical arms clipped to the plane in the first and the last block:
    up = min(up, i), dn = min(dn, H - 1 - i).  Every rectangle stays inside the plane."""
    l, r, t, b = [tile_rows(a, K) for a in block_arms]
    H = l.shape[0]
    ii = np.arange(H)[:, None]
    return [l, r, np.minimum(t, ii).astype(np.int32), np.minimum(b, H - 1 - ii).astype(np.int32)]


def flat_guide(H, w, w0, seed):
    """float32 [H][w] guide with gray.flat[k] = g0[k % w0] (w a multiple of w0): constant down a column, so the faithful
    up / down passes, which read gray.flat[j +- s], see the same guide in every column block and in the strip."""
    assert w % w0 == 0
    g0 = _rng(seed, w0).integers(0, 256, w0).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(np.tile(g0, w // w0), (H, w)))


def column_guide(H, w0, seed):
    """float32 [H][w0] strip of a guide that differs from row to row (the fixed vertical passes read it at the pixel)."""
    return _rng(seed, H, w0).integers(0, 256, (H, w0)).astype(np.float32)


def rows_differ(block):
    rows = np.ascontiguousarray(block).reshape(block.shape[0], -1)
    return len({r.tobytes() for r in rows}) == rows.shape[0]


def is_ramp(block):
    """True when consecutive entries of the flattened block differ by one constant."""
    d = np.diff(np.asarray(block, np.float64).reshape(-1))
    return d.size > 0 and bool((d == d[0]).all())


# --------------------------------------------------------------------------------------------------- oracle compositions
def split3(a, h0):
    """(first, second, last) block of h0 rows"""
    return a[:h0].copy(), a[h0:2 * h0].copy(), a[-h0:].copy()


def adcensus_expected(O, Lb, Rb, K, D, view):
    """ComputeADcensus (view 0) / ComputeADcensusRight (view 1) of the block tiled K times: (top, middle, bottom) volumes
    from the rows [0, 2 h0) and [H - h0, H) of the full image."""
    h0 = Lb.shape[0]
    H = K * h0
    L, R = tile_rows(Lb, K).astype(np.float32), tile_rows(Rb, K).astype(np.float32)
    head = O.adcensus_view(L, R, D, SIGMA_C, SIGMA_S, view, 0, 2 * h0)
    top, mid = head[:h0].copy(), head[h0:2 * h0].copy()
    del head
    tail = O.adcensus_view(L, R, D, SIGMA_C, SIGMA_S, view, H - h0, H)
    bot = tail[H - h0:].copy()
    return top, mid, bot


def aggregate_expected(O, vb, block_arms, order):
    """smt_crossarm_aggregate on [P; P; P] with the clipped arms: ((top, middle, bottom) volumes, the same of the maps)"""
    h0 = vb.shape[0]
    out, oob = O.aggregate_rect(tile_rows(vb, 3), full_arms(block_arms, 3), order)
    assert oob == 0, "a rectangle leaves the plane or is empty"
    return split3(out, h0), split3(O.wta(out), h0)


def scan_rows_expected(O, cb, gb, which):
    """left / right pass of one block of rows: rows are independent, so every block of the full result is this one"""
    return O.scan_pass(cb, gb, P1, P2, which)


def scan_cols_expected(O, strip, gstrip, which, fixed):
    """up / down pass of the strip [H][w0][D]: columns are independent, so every column block of the full result is this
    one.  fixed (SMT_QUIRK_FIX_SCAN_VERTICAL): the horizontal pass of the transposed strip and guide."""
    if not fixed:
        return O.scan_pass(strip, gstrip, P1, P2, which)
    t = O.scan_pass(np.ascontiguousarray(strip.transpose(1, 0, 2)), np.ascontiguousarray(gstrip.T), P1, P2,
                    {"up": "left", "down": "right"}[which])
    return np.ascontiguousarray(t.transpose(1, 0, 2))


def scan_run_parts(O, cb, g0row, H, w):
    """The four path volumes of smt_scanline_run for the cost cb [h0][w0][D] tiled over [H][w] and the flat guide whose
    row is g0row [w]: (left, right) of one block of rows [h0][w][D], (up, down) of the strip [H][w0][D]."""
    h0, w0, _ = cb.shape
    rows = tile_cols(cb, w // w0)
    grow = np.ascontiguousarray(np.broadcast_to(g0row, (h0, w)))
    strip = tile_rows(cb, H // h0)
    gstrip = np.ascontiguousarray(np.broadcast_to(g0row[:w0], (H, w0)))
    return (O.scan_pass(rows, grow, P1, P2, "left"), O.scan_pass(rows, grow, P1, P2, "right"),
            O.scan_pass(strip, gstrip, P1, P2, "up"), O.scan_pass(strip, gstrip, P1, P2, "down"))


def compose_scan_run(lr, u, d, r0, r1, kc):
    """Rows [r0, r1) (whole blocks) of ((left + right) + up) + down in float32 torch adds: lr = left + right of one block
    of rows, u / d the strips; kc = column blocks."""
    g = (r1 - r0) // lr.shape[0]
    x = lr.repeat(g, 1, 1)
    x = x + u[r0:r1].repeat(1, kc, 1)
    return x + d[r0:r1].repeat(1, kc, 1)


def first_min(v):
    """The reference's WinTakeAll on a float32 tensor [..., D] as float32 indices: `cost = v[0]; if (cost > v[d])`, so the
    first of tied minima wins, a NaN at d > 0 never wins and a NaN at d = 0 freezes the result at 0.  Not argmin: its tie
    rule is not the reference's."""
    D = v.shape[-1]
    nan0 = v[..., 0].isnan()
    w = torch.where(v.isnan(), torch.full((), float("inf"), dtype=v.dtype, device=v.device), v)
    idx = torch.where(w == w.amin(-1, keepdim=True), torch.arange(D, dtype=torch.int32, device=v.device),
                      torch.full((), D, dtype=torch.int32, device=v.device)).amin(-1)
    return torch.where(nan0, torch.zeros((), dtype=torch.int32, device=v.device), idx).to(torch.float32)


# ------------------------------------------------------------------------------------------------------------ comparison
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """integer view of the same width (what a uint32 view compares for float32)"""
    return t if not t.is_floating_point() else t.view(_INT[t.element_size()])


def prefilled(shape, dtype, device):
    """an output whose every byte is 0xFF"""
    t = torch.empty(shape, dtype=dtype, device=device)
    t.view(_INT[t.element_size()]).fill_(-1)
    return t


def _as(expect, like):
    e = expect if isinstance(expect, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(expect))
    assert e.dtype == like.dtype and tuple(e.shape[1:]) == tuple(like.shape[1:]), (e.dtype, like.dtype, e.shape, like.shape)
    return e.to(like.device)


def row_chunks(H, h0, row_bytes, chunk=None):
    """[r0, r1) pieces of whole blocks of h0 rows, each at most `chunk` bytes (at least one block)"""
    per = max(1, (chunk or CHUNK) // (h0 * row_bytes)) * h0
    return [(r, min(r + per, H)) for r in range(0, H, per)]


def differing_blocks(out, h0, first=2, last=None, ref=None, chunk=None):
    """Blocks first .. last (inclusive) of `out` [K h0][...] that differ from `ref` (default: block 1) in any bit."""
    K = out.shape[0] // h0
    assert out.shape[0] == K * h0 and out.is_contiguous()
    b = bits(out).reshape(K, -1)
    r = b[1] if ref is None else bits(_as(ref, out)).reshape(-1)
    last = K - 2 if last is None else last
    per = max(1, (chunk or CHUNK) // (b.shape[1] * out.element_size()))
    bad = []
    for s in range(first, last + 1, per):
        e = min(s + per, last + 1)
        ne = (b[s:e] != r).any(1)
        bad += [s + int(i) for i in ne.nonzero().flatten().tolist()]
    return bad


def check_rows(out, h0, top, mid, bot, what="", chunk=None):
    """`out` [K h0][...]: blocks 0, 1 and K - 1 equal the oracle's top, middle and bottom bit for bit, and blocks
    2 .. K - 2 equal block 1."""
    K = out.shape[0] // h0
    assert K >= 3 and out.shape[0] == K * h0, (what, out.shape, h0)
    for name, k, e in (("first", 0, top), ("second", 1, mid), ("last", K - 1, bot)):
        g, w = bits(out[k * h0:(k + 1) * h0]), bits(_as(e, out))
        n = int((g != w).sum())
        assert n == 0, f"{what}: the {name} block differs from the oracle in {n} of {g.numel()} elements"
    bad = differing_blocks(out, h0, chunk=chunk)
    assert not bad, f"{what}: {len(bad)} of the blocks 2 .. {K - 2} differ from block 1, the first at block {bad[0]}"


def check_cols(out, w0, strip, what="", chunk=None):
    """`out` [H][Kc w0][D]: every column block equals the oracle's strip [H][w0][D] bit for bit."""
    H, w, D = out.shape
    kc = w // w0
    assert w == kc * w0 and out.is_contiguous()
    s = bits(_as(strip, out[:, :w0]))
    b = bits(out).view(H, kc, w0 * D)
    for r0, r1 in row_chunks(H, 1, w * D * out.element_size(), chunk):
        ne = (b[r0:r1] != s[r0:r1].reshape(r1 - r0, 1, w0 * D)).any(2)
        n = int(ne.sum())
        if n:
            i, k = [int(x) for x in ne.nonzero()[0]]
            raise AssertionError(f"{what}: {n} (row, column block) runs of the rows {r0} .. {r1 - 1} differ from the oracle's "
                                 f"strip, the first at row {r0 + i}, column block {k}")


def check_pieces(out, h0, expected_piece, what="", chunk=None, row_bytes=None):
    """`out` [H][...] against expected_piece(r0, r1) -> tensor of the rows [r0, r1), piece by piece, bit for bit.
    row_bytes: what a row of the piece's largest operand holds (default: a row of `out`)."""
    H = out.shape[0]
    row_bytes = row_bytes or out[0].numel() * out.element_size()
    for r0, r1 in row_chunks(H, h0, row_bytes, chunk):
        e = expected_piece(r0, r1)
        ne = bits(out[r0:r1]) != bits(e)
        n = int(ne.sum())
        if n:
            at = [int(x) for x in ne.nonzero()[0]]
            at[0] += r0
            raise AssertionError(f"{what}: {n} elements of the rows {r0} .. {r1 - 1} differ, the first at {at}")


@functools.lru_cache(maxsize=None)
def left_costs_fn():
    """tests/test_sad_both_cpu.py's numpy box sums of smt_sad_both's costL"""
    from test_sad_both_cpu import left_costs
    return left_costs
