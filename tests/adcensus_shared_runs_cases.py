"""Shapes of the run-walk tests of the shared maps-only form (test_adcensus_shared_runs_cpu.py / _gpu.py) and a Python
recomputation of the walk's run structure, independent of the library: which runs a workgroup walks, how long they are
and how many ring columns are live, so that the tests can assert that a shape reaches what it is there for.

The chunks of a launch are cut into 8 slices of per = ceil(nbx * H / 8) chunks and a workgroup takes K consecutive
chunks of one slice, so a workgroup never holds more than `per` chunks: a run of 4 chunks, a sub-run or a row change
inside a workgroup need nbx * H >= 33 or so, whatever K is."""
SH_RUN = 4

# H, W, D, SMT_MAPS_SHARED.  The first nine are short (nbx * H <= 22: at most 3 chunks per workgroup, so runs of 1..3
# chunks); the tall ones reach runs of 4 chunks, sub-runs and, with both, row changes inside a workgroup.
SHAPES = [(3, 330, 192, None),         # runs of 1..3 chunks
          (2, 259, 192, None),         # the row's last chunk has 3 pixels: a wave's walk is cut by W
          (2, 700, 192, None),         # 11 chunks per row
          (3, 390, 64, None),          # C = 1; runs longer than D, complete columns
          (2, 460, 100, None),         # C = 2; D no multiple of 64; XPAD entries in use
          (2, 520, 256, "force"),      # C = 4
          (1, 500, 192, None),         # H = 1
          (5, 198, 192, None),         # one identity column (W-3-D == 3); columns 0..2 at H = 5
          (2, 261, 192, None),         # W-3-D == 66: the edge columns start in the second chunk
          (6, 330, 192, None),         # per = 5: a 4-chunk run (64 pixels per wave) and a row change inside a workgroup
          (7, 259, 192, None),         # per = 5: a 4-chunk run and the 3-pixel chunk in one run
          (6, 700, 192, None),         # per = 9: K = 8 and 64 give runs longer than SH_RUN, so sub-runs
          (6, 390, 64, None),          # C = 1 with 4-chunk runs and row changes
          (5, 460, 100, None),         # C = 2, D no multiple of 64, with 4-chunk runs and row changes
          (8, 700, 256, "force")]      # C = 4; K = 5: the run S = 320 .. E = 575 has 511 live columns, the ring's bound
CHUNKS = [None, "1", "2", "3", "5", "8", "64"]     # SMT_MAPS_CHUNKS; unset is 4


def workgroup_runs(H, W, K):
    """for every left-pass workgroup that has chunks: its runs [(row, first chunk, chunks)], in walking order"""
    nbx = (W + 63) // 64
    nb = nbx * H
    per = (nb + 7) >> 3
    out = []
    for b in range(8 * ((per + K - 1) // K)):
        cl = (b >> 3) * K
        c = (b & 7) * per + cl
        if cl >= per or c >= nb:
            continue
        left = min(K, per - cl, nb - c)
        i, bx = divmod(c, nbx)
        runs = []
        while left > 0:
            n = min(SH_RUN, nbx - bx, left)
            runs.append((i, bx, n))
            left -= n
            bx += n
            if bx == nbx:
                i, bx = i + 1, 0
        out.append(runs)
    return out


def features(H, W, D, K):
    """what the run walk meets at this shape and K"""
    f = {"run4": False, "subrun": False, "row_change": False, "cut_by_W": False, "live": 0, "chunks": 0}
    for runs in workgroup_runs(H, W, K):
        for r, (i, bx, n) in enumerate(runs):
            S, E = 64 * bx, 64 * (bx + n) - 1
            f["chunks"] += n
            f["run4"] |= n == SH_RUN
            f["cut_by_W"] |= E > W - 1
            f["live"] = max(f["live"], min(W - 4, E) - max(3, S - D + 1) + 1)
            if r:
                pi, pbx, pn = runs[r - 1]
                f["subrun"] |= pi == i and pbx + pn == bx
                f["row_change"] |= pi != i
    return f
