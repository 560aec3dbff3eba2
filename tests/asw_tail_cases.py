"""Cases and references shared by tests/test_asw_tail_cpu.py and tests/test_asw_tail_gpu.py: the tail of ASW/ASWeight.cpp
(:67-78).  The references are plain Python restatements of the rules in include/smt.h, written without looking at
csrc/fill_image_rules.h or the kernels: FillImageNew loop for loop as ASW/ASW.h:434-511 runs (with the two undefined reads
defined as the header defines them), and the three OpenCV steps as the header states them (parity with OpenCV itself is
unpinned: there is no OpenCV to hold them against)."""
import numpy as np

FIX_ROW_END = 0x1
DBL_EPSILON = 2.220446049250313e-16
CLASSES = ("left", "right", "past_end", "row_end_nonzero", "row_end_zero", "shifted", "starved")
# 1x1, 1x7, 7x1, 3x4: windows wider than the image, H = 1 (the row-end read is the undefined one); 33x65, 70x45: speckle
# tiles of 32 crossed both ways, W no multiple of 4; 40x137: walks of 16 probes (T(16) = 136)
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 4), (33, 65), (70, 45), (40, 137)]
GAP = 5            # guard bytes between the maps of a batch
GUARD = 0xA5


# ------------------------------------------------------------------------------------------------------ FillImageNew
def ref_fill(m, fix=0):
    """-> (filled map, (holes that pushed nothing, holes left 0 for want of an entry), {class: holes})"""
    H, W = m.shape
    flat = m.reshape(-1)
    holes = [(r, c) for r in range(H) for c in range(W) if m[r, c] == 0]
    values, owner = [], []
    cls = dict.fromkeys(CLASSES, 0)
    for i, (r, c) in enumerate(holes):
        col, offset, found = c, 0, False
        while col >= 0:                                    # :465
            col = col - offset
            if col < 0:
                break                                      # abandoned, :469-475
            v = int(m[r, col])
            if v:
                values.append(v); owner.append(i); cls["left"] += 1; found = True
                break
            offset += 1
        if found:
            continue                                       # pixel_col = 0xffff >= col, :480
        col, offset = c, 0
        while col < W:                                     # :485
            col = col + offset
            if col > W or (col == W and (fix & FIX_ROW_END)):
                values.append(0); owner.append(i); cls["past_end"] += 1
                break
            if col == W:                                   # disp.at<uchar>(r, W): the next row's first byte; 0 below the map
                v = int(flat[(r + 1) * W]) if r + 1 < H else 0
                if v:
                    values.append(v); owner.append(i); cls["row_end_nonzero"] += 1
                    break
                cls["row_end_zero"] += 1                   # ++offset, then col < W fails: nothing pushed
                break
            v = int(m[r, col])
            if v:
                values.append(v); owner.append(i); cls["right"] += 1
                break
            offset += 1
    out = m.copy()
    starved = 0
    for i, (r, c) in enumerate(holes):                     # :504-510
        if i < len(values):
            out[r, c] = values[i]
            if owner[i] != i:
                cls["shifted"] += 1
        else:
            starved += 1                                   # past the list's end: keeps 0
    cls["starved"] = starved
    return out, (len(holes) - len(values), starved), cls


def ref_fill_own(m):
    """every hole's own search result under FIX_ROW_END (where every hole pushes): what fixed mode must assign"""
    H, W = m.shape
    out = m.copy()
    for r in range(H):
        for c in range(W):
            if m[r, c]:
                continue
            k, val = 0, None
            while c - k * (k + 1) // 2 >= 0:
                if m[r, c - k * (k + 1) // 2]:
                    val = int(m[r, c - k * (k + 1) // 2])
                    break
                k += 1
            if val is None:
                k, val = 0, 0
                while c + k * (k + 1) // 2 < W:
                    if m[r, c + k * (k + 1) // 2]:
                        val = int(m[r, c + k * (k + 1) // 2])
                        break
                    k += 1
            out[r, c] = val
    return out


def fill_maps():
    """[(name, uint8 map)]: seeded random maps at hole densities 0.3, 0.6, 0.9 on every shape, and the crafted ones"""
    rng = np.random.default_rng(7601)
    out = []
    for (H, W) in SHAPES:
        for dens in (0.3, 0.6, 0.9):
            m = rng.integers(1, 256, (H, W)).astype(np.uint8)
            m[rng.random((H, W)) < dens] = 0
            out.append((f"rand{H}x{W}d{dens}", m))
    z = np.zeros((4, 7), np.uint8)
    a = z.copy(); a[3, 1:] = 5                            # all-zero rows above a row starting with 0
    out.append(("zero_rows_above_0", a))
    b = z.copy(); b[2, 0] = 9; b[3, 3] = 4                # all-zero rows above a row starting with 9
    out.append(("zero_rows_above_9", b))
    c = np.zeros((5, 11), np.uint8); c[1, 0] = 9; c[2, 4] = 3; c[4, 10] = 8   # a missing push in row 0 shifts the rest
    out.append(("shift_then_values", c))
    out.append(("all_zero", np.zeros((6, 9), np.uint8)))
    out.append(("all_zero_1row", np.zeros((1, 7), np.uint8)))
    out.append(("no_holes", rng.integers(1, 256, (9, 13)).astype(np.uint8)))
    w = np.zeros((3, 137), np.uint8); w[0, 136] = 200; w[1, 0] = 17; w[2, 70] = 1   # walks of 16 probes from column 0
    out.append(("long_walks", w))
    return out


# --------------------------------------------------------------------------------------------------------- normalize
def _scale_shift(smin, smax):
    d = float(smax) - float(smin)
    scale = 255.0 * (1.0 / d if d > DBL_EPSILON else 0.0)
    shift = 0.0 - float(smin) * scale
    return np.float32(scale), np.float32(shift)


def _sat_u8(t):
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)     # rint: half to even


def ref_normalize(m):
    """uint8 or finite float32 map -> uint8: min-max to 0..255 in float32 steps, rounded half to even"""
    sf, hf = _scale_shift(m.min(), m.max())
    t = m.astype(np.float32) * sf                           # float32 product, rounded
    t = t + hf                                              # float32 sum, rounded
    return _sat_u8(t)


def ref_normalize_rows(rows):
    """ref_normalize on every row of a [n][k] uint8 array at once (the exhaustive (min, max) table)"""
    smin = rows.min(axis=1).astype(np.float64)
    smax = rows.max(axis=1).astype(np.float64)
    d = smax - smin
    inv = np.divide(1.0, d, out=np.zeros_like(d), where=d > DBL_EPSILON)
    scale = 255.0 * inv
    shift = 0.0 - smin * scale
    t = rows.astype(np.float32) * scale.astype(np.float32)[:, None]
    t = t + shift.astype(np.float32)[:, None]
    return _sat_u8(t)


def minmax_table():
    """32 640 maps of 1 x 4 holding every uint8 (min, max) pair with min < max and two seeded values between them"""
    lo, hi = np.triu_indices(256, 1)
    rng = np.random.default_rng(7602)
    mid = lo[:, None] + (rng.random((lo.size, 2)) * (hi - lo + 1)[:, None]).astype(np.int64)
    rows = np.stack([hi, mid[:, 0], lo, mid[:, 1]], axis=1).astype(np.uint8)
    assert rows.shape == (32640, 4)
    return rows


# --------------------------------------------------------------------------------------------------------- medianBlur
def ref_median(m, k):
    """the true median of the k x k window under BORDER_REPLICATE, pixel by pixel"""
    H, W = m.shape
    r = k // 2
    out = np.empty_like(m)
    for y in range(H):
        for x in range(W):
            win = [m[min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)]
                   for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
            out[y, x] = sorted(win)[k * k // 2]
    return out


# ----------------------------------------------------------------------------------------------------- filterSpeckles
def ref_speckles(m, new_val, max_size, max_diff):
    """4-neighbour components over |a - b| <= max_diff with neither end equal to new_val; components of at most max_size
    pixels become new_val"""
    H, W = m.shape
    out = m.copy()
    seen = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if seen[y, x] or int(m[y, x]) == new_val:
                continue
            comp, stack = [], [(y, x)]
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                comp.append((cy, cx))
                for ny, nx in ((cy, cx + 1), (cy, cx - 1), (cy + 1, cx), (cy - 1, cx)):
                    if 0 <= ny < H and 0 <= nx < W and not seen[ny, nx] and int(m[ny, nx]) != new_val \
                            and abs(int(m[ny, nx]) - int(m[cy, cx])) <= max_diff:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            if len(comp) <= max_size:
                for cy, cx in comp:
                    out[cy, cx] = new_val & 0xFF
    return out


def speckle_random(H, W, seed):
    """blocks of a few values (components around the size threshold, many crossing the 32-pixel tiles) with seeded noise"""
    rng = np.random.default_rng(7700 + seed)
    coarse = rng.choice(np.array([0, 20, 22, 25, 60, 63], np.uint8), ((H + 2) // 3, (W + 4) // 5))
    m = np.kron(coarse, np.ones((3, 5), np.uint8))[:H, :W].copy()
    noise = rng.random((H, W)) < 0.06
    m[noise] = rng.integers(0, 256, int(noise.sum())).astype(np.uint8)
    return m


def speckle_crafted(new_val=0):
    """70 x 45, background new_val: components of exactly 40 and 41 pixels; two 5 x 5 blocks joined only diagonally (two
    components of 25, not one of 50); chains of 50 with steps of 2 (one component) and 3 (50 components); a block of 48
    cut in two 24s by a line of new_val; a 41-pixel column crossing the tile border at row 32"""
    m = np.full((70, 45), new_val, np.uint8)
    m[1:6, 1:9] = 100                                      # 40: goes
    m[1:6, 11:19] = 100; m[6, 11] = 101                    # 41: stays
    m[8:13, 1:6] = 150; m[13:18, 6:11] = 150               # diagonal contact only: 25 + 25, both go
    step2 = (10 + 2 * np.arange(44)).astype(np.uint8); m[21, 0:44] = step2    # one chain of 44 > 40: stays
    step3 = (10 + 3 * np.arange(44)).astype(np.uint8); m[23, 0:44] = step3    # 44 components of 1: go
    m[25:31, 20:28] = 200; m[25:31, 24] = new_val          # 48 cut into 24 + 18 by a column of new_val: both go
    m[25:66, 40] = 77                                      # 41 pixels down across rows 32 and 64: stays
    m[30:34, 30:40] = 90                                   # 40 across the tile border at row 32: goes
    return m


def speckle_maps():
    out = [("crafted0", speckle_crafted(0), (0, 40, 2)), ("crafted7", speckle_crafted(7), (7, 40, 2))]
    for i, (H, W) in enumerate(SHAPES):
        out.append((f"rand{H}x{W}", speckle_random(H, W, i), (0, 40, 2)))
    out.append(("rand33x65_diff0_size3", speckle_random(33, 65, 20), (0, 3, 0)))
    return out


# ------------------------------------------------------------------------------------------------------------- tail
def ref_tail(m, speckle=(0, 40, 2), median_first=5, median_last=3, fix=0):
    """:69 + :72-78 -> (after_median, after_fill, final, fill counts)"""
    a = ref_normalize(m)
    a = ref_speckles(a, *speckle)
    a = ref_median(a, median_first)
    f, counts, _ = ref_fill(a, fix)
    return a, f, ref_median(f, median_last), counts


def tail_maps():
    """crosscheck-like maps: smooth disparities 0..59 with rejected (0) patches and isolated survivors"""
    out = []
    for i, (H, W) in enumerate(SHAPES):
        rng = np.random.default_rng(7800 + i)
        y, x = np.mgrid[0:H, 0:W]
        m = (5 + (x * 40) // max(W, 1) + (y * 14) // max(H, 1)).astype(np.uint8)
        m[rng.random((H, W)) < 0.25] = 0
        if W > 8:
            m[:, : W // 6] = 0                              # the occluded band at the left edge
            m[H // 2, 0] = 31
        out.append((f"tail{H}x{W}", m))
    return out


def batch_with_gaps(maps, dtype=np.uint8):
    """[k maps of one shape] -> (flat buffer prefilled with GUARD holding the maps `stride` apart, stride)"""
    H, W = maps[0].shape
    stride = H * W + GAP
    buf = np.full(len(maps) * stride, GUARD, dtype)
    for b, m in enumerate(maps):
        buf[b * stride: b * stride + H * W] = m.reshape(-1)
    return buf, stride


def split_with_gaps(buf, k, H, W):
    """-> ([k maps], all guard elements of the gaps)"""
    stride = H * W + GAP
    maps = [buf[b * stride: b * stride + H * W].reshape(H, W) for b in range(k)]
    gaps = np.concatenate([buf[b * stride + H * W: (b + 1) * stride] for b in range(k)])
    return maps, gaps


# ------------------------------------------------------------------------- rows of the bounds and stream-order suites
# Registered on import, as tests/ncc_both_cases.py does: a reason in NOT_CALLER_BUFFER for the three entries without
# caller buffers, real entries with cases for the others (the host twin among the HOST_ENTRIES), and their decisions in
# SYNCHRONISING (all asynchronous).  test_asw_tail_cpu.py and test_asw_tail_gpu.py import this module, so the
# completeness tests see the rows whenever the suite is collected as a whole.
import ctypes as C  # noqa: E402

import bounds_cases as BC  # noqa: E402
import stream_order_cases as SC  # noqa: E402

BC.NOT_CALLER_BUFFER.update({
    "smt_asw_post_default_params": "host struct out", "smt_asw_flow_status": "status",
    "smt_median_blur_selftest_nets": "host-only selftest",
})
BC.HOST_ENTRIES = tuple(BC.HOST_ENTRIES) + ("smt_fill_image_new_host",)


def _holey(H, W, seed, P=3):
    rng = np.random.default_rng([seed, H, W])
    d = rng.integers(1, 256, (P, H, W)).astype(np.uint8)
    d[rng.random((P, H, W)) < 0.6] = 0
    return d


@BC.entry("smt_minmax_normalize_u8_batch", dict(H=5, W=67, gap=0), dict(H=1, W=63, gap=1), dict(H=33, W=34, gap=1))
def _b_norm_u8(A, X, H, W, gap, P=3):
    d = np.stack([BC.rb((H, W), 300 + b, 10 + 20 * b, 200) for b in range(P)])
    s = BC._strided(gap, H * W)
    A.inp("in", d, stride=s); A.out("out", (P, H, W), np.uint8, stride=s)

    def verify(o):
        for b in range(P):
            BC.bits_eq(o["out"][b], ref_normalize(d[b]), f"out[{b}]")
    return (lambda: X.lib.smt_minmax_normalize_u8_batch(A.ptr("in"), A.ptr("out"), P, BC.sz(s), H, W, X.st()), verify)


@BC.entry("smt_minmax_normalize_f32_u8_batch", dict(H=5, W=67, gap=0), dict(H=1, W=63, gap=1), dict(H=33, W=34, gap=1))
def _b_norm_f32(A, X, H, W, gap, P=3):
    d = np.stack([BC.rf((H, W), 310 + b, 60.0) - np.float32(7 * b) for b in range(P)])
    s = BC._strided(gap, H * W)
    A.inp("in", d, stride=s); A.out("out", (P, H, W), np.uint8, stride=s)

    def verify(o):
        for b in range(P):
            BC.bits_eq(o["out"][b], ref_normalize(d[b]), f"out[{b}]")
    return (lambda: X.lib.smt_minmax_normalize_f32_u8_batch(A.ptr("in"), A.ptr("out"), P, BC.sz(s), H, W, X.st()), verify)


@BC.entry("smt_filter_speckles_u8_batch", dict(H=9, W=65, gap=0), dict(H=1, W=63, gap=1, err=False), dict(H=33, W=34, gap=1))
def _b_speckles(A, X, H, W, gap, err=True, P=3):
    d = np.stack([speckle_random(H, W, 40 + b) for b in range(P)])
    s = BC._strided(gap, H * W)
    A.inout("maps", d, stride=s)
    if err:
        A.inout("err", np.zeros(1, np.int32))

    def verify(o):
        for b in range(P):
            BC.bits_eq(o["maps"][b], ref_speckles(d[b], 0, 12, 2), f"maps[{b}]")
        assert not err or int(o["err"][0]) == 0
    return (lambda: X.lib.smt_filter_speckles_u8_batch(A.ptr("maps"), P, BC.sz(s), W, H, 0, 12, 2,
                                                       A.ptr("err" if err else None), X.st()), verify)


@BC.entry("smt_median_blur_u8_batch", dict(H=5, W=67, gap=0, k=3), dict(H=1, W=63, gap=1, k=5), dict(H=17, W=65, gap=1, k=5),
          dict(H=17, W=1, gap=1, k=3))
def _b_median(A, X, H, W, gap, k, P=3):
    d = _holey(H, W, 320)
    s = BC._strided(gap, H * W)
    A.inp("in", d, stride=s); A.out("out", (P, H, W), np.uint8, stride=s)

    def verify(o):
        for b in range(P):
            BC.bits_eq(o["out"][b], ref_median(d[b], k), f"out[{b}]")
    return (lambda: X.lib.smt_median_blur_u8_batch(A.ptr("in"), A.ptr("out"), P, BC.sz(s), W, H, k, X.st()), verify)


def _fill_entry(host):
    def f(A, X, H, W, gap, fix=0, counts=True, P=3):
        d = _holey(H, W, 330)
        d[0, 0] = 0                                        # row 0 of map 0 all holes: a missing push where (1, 0) is 0
        s = BC._strided(gap, H * W)
        A.inout("maps", d, stride=s)
        if counts:
            A.out("counts", (P, 2), np.int32)

        def call():
            args = (A.ptr("maps"), P, BC.sz(s), H, W, C.c_uint(fix), A.ptr("counts" if counts else None))
            return X.lib.smt_fill_image_new_host(*args) if host else X.lib.smt_fill_image_new_batch(*args, X.st())

        def verify(o):
            for b in range(P):
                want, cnt, _ = ref_fill(d[b], fix)
                BC.bits_eq(o["maps"][b], want, f"maps[{b}]")
                assert not counts or tuple(o["counts"][b]) == cnt
        return call, verify
    return f


_FILL_CASES = (dict(H=5, W=67, gap=0), dict(H=1, W=63, gap=1), dict(H=9, W=34, gap=1, fix=FIX_ROW_END),
               dict(H=7, W=1, gap=1, counts=False))
BC.entry("smt_fill_image_new_batch", *_FILL_CASES)(_fill_entry(False))
BC.entry("smt_fill_image_new_host", *_FILL_CASES)(_fill_entry(True))


@BC.entry("smt_asw_tail_batch", dict(H=9, W=65, gap=0), dict(H=9, W=65, gap=1, stages=False, counts=False, err=False),
          dict(H=1, W=63, gap=1), dict(H=33, W=34, gap=1, fix=FIX_ROW_END))
def _b_tail(A, X, H, W, gap, fix=0, stages=True, counts=True, err=True, P=3):
    rng = np.random.default_rng([340, H, W])
    y, x = np.mgrid[0:H, 0:W]
    d = np.stack([(5 + (x * 40) // W + (y * 14) // H + b).astype(np.uint8) for b in range(P)])
    d[rng.random((P, H, W)) < 0.3] = 0
    s = BC._strided(gap, H * W)
    A.inout("lastDisp", d, stride=s)
    if stages:
        A.out("after_median", (P, H, W), np.uint8, stride=s); A.out("after_fill", (P, H, W), np.uint8, stride=s)
    if counts:
        A.out("counts", (P, 2), np.int32)
    if err:
        A.inout("err", np.zeros(1, np.int32))

    def call():
        q = X.L.ASWPostParams()
        X.lib.smt_asw_post_default_params(C.byref(q))
        q.speckle_max_size, q.fix = 6, fix
        return X.lib.smt_asw_tail_batch(A.ptr("lastDisp"), P, BC.sz(s), H, W, C.byref(q),
                                        A.ptr("after_median" if stages else None), A.ptr("after_fill" if stages else None),
                                        A.ptr("counts" if counts else None), A.ptr("err" if err else None), X.st())

    def verify(o):
        for b in range(P):
            am, af, fin, cnt = ref_tail(d[b], speckle=(0, 6, 2), fix=fix)
            BC.bits_eq(o["lastDisp"][b], fin, f"lastDisp[{b}]")
            if stages:
                BC.bits_eq(o["after_median"][b], am, f"after_median[{b}]"); BC.bits_eq(o["after_fill"][b], af, f"after_fill[{b}]")
            assert not counts or tuple(o["counts"][b]) == cnt
        assert not err or int(o["err"][0]) == 0
    return call, verify


_POST_OUTS = ("dispL", "dispR", "lastDisp", "dispL8", "dispR8", "after_median", "after_fill", "counts")


@BC.entry("smt_asw_flow_run_batch_post", dict(H=2, W=17, D=65, ws=1, P=2), dict(H=3, W=33, D=8, ws=1, P=3),
          dict(H=1, W=15, D=4, ws=2, P=2, outs=("lastDisp",)), dict(H=3, W=33, D=8, ws=1, P=1, outs=("dispL", "lastDisp", "dispL8")))
def _b_flow_post(A, X, H, W, D, ws, P, outs=_POST_OUTS):
    imgs = [BC._padded(H, W, ws + 1, 350 + 3 * b) for b in range(P)]
    A.inp("L", np.stack([i[0] for i in imgs])); A.inp("R", np.stack([i[1] for i in imgs]))
    for nm in outs:
        A.out(nm, (P, 2) if nm == "counts" else (P, H, W),
              np.int32 if nm == "counts" else np.float32 if nm in ("dispL", "dispR") else np.uint8)
    sp, cm = X.O.asw_masks(ws, 50.0, 30.0)

    def call():
        p, h = X.L.ASWParams(), C.c_void_p()
        X.lib.smt_asw_default_params(C.byref(p))
        p.winSize, p.T, p.sigma_space, p.sigma_color = ws, 40, 50.0, 30.0
        rc = X.lib.smt_asw_flow_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
        if rc:
            return rc
        try:
            rc = X.lib.smt_asw_flow_set_stream(h, X.st())
            ptr = {nm: A.ptr(nm if nm in outs else None) for nm in _POST_OUTS}
            rc = rc or X.lib.smt_asw_flow_run_batch_post(h, A.ptr("L"), A.ptr("R"), P, ptr["dispL"], ptr["dispR"], ptr["lastDisp"],
                                                         ptr["dispL8"], ptr["dispR8"], None, ptr["after_median"],
                                                         ptr["after_fill"], ptr["counts"])
            X.sync()
            return rc or X.lib.smt_asw_flow_status(h)
        finally:
            X.lib.smt_asw_flow_destroy(h)

    def verify(o):
        for b in range(P):
            Lp, Rp = imgs[b][2], imgs[b][3]
            rl, rr = (X.O.asw(Lp, Rp, D, ws, sp, cm, 40, v) for v in (0, 1))
            for nm, v in (("dispL", 0), ("dispR", 1)):
                if nm in outs:
                    BC._asw_map_check(X, o[nm][b], Lp, Rp, D, ws, sp, cm, v, f"{nm}[{b}]")
            if "dispL" in outs and "dispR" in outs:
                rl, rr = o["dispL"][b], o["dispR"][b]          # the call's own maps
                am, af, fin, cnt = ref_tail(X.O.asw_crosscheck(rl, rr))
                for nm, ref in (("lastDisp", fin), ("after_median", am), ("after_fill", af)):
                    if nm in outs:
                        BC.bits_eq(o[nm][b], ref, f"{nm}[{b}]")
                assert "counts" not in outs or tuple(o["counts"][b]) == cnt
            for nm, src in (("dispL8", "dispL"), ("dispR8", "dispR")):
                if nm in outs:
                    BC.bits_eq(o[nm][b], ref_normalize(o[src][b]), f"{nm}[{b}]")
    return call, verify


SC.SYNCHRONISING.update({name: SC.ASYNC for name in (
    "smt_minmax_normalize_u8_batch", "smt_minmax_normalize_f32_u8_batch", "smt_filter_speckles_u8_batch",
    "smt_median_blur_u8_batch", "smt_fill_image_new_batch", "smt_asw_tail_batch", "smt_asw_flow_run_batch_post")})
