// FillImageNew (ASW/ASW.h:434-511) as three data-parallel steps, shared by the kernels of csrc/asw_tail.hip and the host
// twin smt_fill_image_new_host, the way fill_rules.h and median_schedule.h are.  What the reference does (DESIGN.md
// section 5.9): a pixel is a hole when it is 0; the holes are listed in raster order; hole i at (r, c) probes the
// UNMODIFIED map at columns c - T(k), then c + T(k), T(k) = k (k + 1) / 2, and may push one value to a list; afterwards
// hole i receives list[i].  A hole that pushes nothing therefore shifts the value of every later hole of the map.
//   fin_search    one hole: did it push, and what
//   fin_find_row  the row that holds push number i, from the exclusive scan of the rows' push counts
// The two reads the reference leaves undefined are defined here: the byte at (H - 1, W) reads as 0 (the caller passes
// row_end = 0 for the last row), and a hole whose index is at or past the list's length keeps 0.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FIN_HD __host__ __device__ static inline
#else
#define FIN_HD static inline
#endif

// Hole at column c of a row of W bytes (row[c] == 0, W <= 65535 so that :480's 0xffff ends the right walk).  row_end is
// the byte the reference reads at column W: the first byte of the next row, 0 below the last row.  fix_row_end != 0
// (SMT_ASW_FIX_FILL_ROW_END): column W is outside like every column past it.  Returns 1 and the pushed value, or 0 when
// the hole pushes nothing (the right walk read a 0 at column W and :485's loop condition ended it).
FIN_HD int fin_search(const uint8_t *row, int W, int c, int row_end, int fix_row_end, int *value)
{
    int col = c, off = 0;
    for (;;) {                                   // :465-484; the first probe is the hole itself
        col -= off;
        if (col < 0) break;                      // :469-475 abandons the walk
        const int v = row[col];
        if (v) { *value = v; return 1; }         // :477-482
        ++off;
    }
    col = c; off = 0;
    for (;;) {                                   // :485-501
        col += off;
        if (col > W || (fix_row_end && col == W)) { *value = 0; return 1; }   // :489-493
        const int v = col == W ? row_end : row[col];                          // :494 reads column W
        if (v) { *value = v; return 1; }
        ++off;
        if (col >= W) return 0;                  // :485: pixel_col < col fails after the read of column W
    }
}

// pp[0 .. H]: exclusive scan of the rows' push counts, pp[0] = 0 <= i < pp[H].  The row r with pp[r] <= i < pp[r + 1].
FIN_HD int fin_find_row(const int *pp, int H, int i)
{
    int lo = 0, hi = H;                          // pp[lo] <= i < pp[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pp[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
