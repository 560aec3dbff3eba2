// The index rules and the cost expression of smt_whole_ncc (NCC.h:117-272, csrc/ncc_whole.hip), shared word for word by the
// kernels and by the host twin of smt_whole_ncc_selftest_box.
//
// Pixel (y, x), k = kernel_size: rows sy = max(0, y-k) .. ey = min(H-1, y+k), columns sx .. ex likewise (NCC.h:186-189).
// N = (ey-sy+1)(ex-sx+1) taps are visited; the reference's count is n = (ey-sy)(ex-sx) (:190), one short per axis.
// Offset o = 1 .. O compares two byte images over that window:
//   SMT_VIEW_LEFT   a = L,  b = T  with T[y][c]  = R[y][c]     for c < o      (the fill: :149-152), R[y][c-o] otherwise;
//   SMT_VIEW_RIGHT  a = T', b = R  with T'[y][c] = L[y][c+o]   for c < W - o,  L[y][c] otherwise (the fill: :169-172).
// One image of the pair is read as it is ("plain"), the other through the shift ("shifted").
//
// Exact form.  With m = S/n the mean the reference uses, sum (v-m)^2 over N taps = Svv - 2 S^2/n + N S^2/n^2
// = (n^2 Svv - q S^2) / n^2 with q = 2n - N, and likewise for the cross term; the three divisions by n (:221-223) and the
// last one (:224) leave
//   res = Ci / (n sqrt(Ai) sqrt(Bi)),  Ai = n^2 Saa - q Sa^2,  Bi = n^2 Sbb - q Sb^2,  Ci = n^2 Sab - q Sa Sb,
// evaluated as (double)Ci / ((double)n * (sqrt((double)Ai) * sqrt((double)Bi))): symmetric in a and b bit for bit.
// Ai = n^2 sum (v-m)^2 >= 0, and 0 only where every tap equals m = S/n: a constant window c has m = N c / n != c unless
// c = 0 (N != n), so only the all-zero window.  res is NaN exactly where Ai Bi = 0 (then Ci = 0 too: 0 / 0).
//
// Integer limit.  With h = ey-sy+1, w = ex-sx+1 <= s = 2k+1: q = hw - 2h - 2w + 2 grows with h and w (h, w >= 2), and so do
// n and the bounds of the sums, so the full window is the worst case: q = 4k^2 - 4k - 1, n = 4k^2, S <= 255 s^2,
// Svv <= 255^2 s^2.
//   k = 35:  q S^2   <= 4759 * 65025 * 71^4 = 7 863 745 696 881 975  < 2^53 = 9 007 199 254 740 992
//            n^2 Svv <= 4900^2 * 65025 * 71^2 = 7 870 262 510 250 000  < 2^53
//   k = 36:  q S^2   <= 5039 * 65025 * 73^4 = 9 304 995 334 344 975  > 2^53
// Where q < 0 (h = 2 or w = 2 with the other side small) the two terms add, at sizes far below the limit.  So for
// k <= NW_INT_MAX_K = 35 every product, Ai, Bi and |Ci| is an integer below 2^53: int64 arithmetic is exact and so is each
// conversion to double.  The uint32 window sums hold 255^2 * 71^2 = 327 791 025 < 2^32.  Beyond k = 35 only the loop nest runs.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define NW_INT_MAX_K 35

__host__ __device__ inline int nw_lo(int c, int k) { return c - k < 0 ? 0 : c - k; }
__host__ __device__ inline int nw_hi(int c, int k, int len) { return c + k > len - 1 ? len - 1 : c + k; }

// the source column of column c of the shifted image (view LEFT: in R; view RIGHT: in L); 1 <= o <= W
__host__ __device__ inline int nw_shift_col(int view_right, int c, int o, int W)
{
    if (view_right) return c < W - o ? c + o : c;
    return c < o ? c : c - o;
}

// Columns sx .. ex of the shifted image as at most two ranges of SOURCE columns: the fill part [f0, f1], read where it
// stands, and the moved part [m0, m1]; a range with first > last is empty.
__host__ __device__ inline void nw_shift_ranges(int view_right, int sx, int ex, int o, int W, int &f0, int &f1, int &m0, int &m1)
{
    if (view_right) {
        const int last = ex < W - o - 1 ? ex : W - o - 1;      // last moved column
        m0 = sx + o; m1 = last + o;
        f0 = sx > W - o ? sx : W - o; f1 = ex;
    } else {
        f0 = sx; f1 = ex < o - 1 ? ex : o - 1;
        const int first = sx > o ? sx : o;                     // first moved column
        m0 = first - o; m1 = ex - o;
    }
}

// a range sum from a row of prefix sums P[c] = sum of the columns below c, uint32 modulo 2^32 (every true range sum is below 2^32)
__host__ __device__ inline uint32_t nw_range(const uint32_t *P, int c0, int c1) { return c0 > c1 ? 0u : P[c1 + 1] - P[c0]; }

// the cost from the integer window sums, h x w taps visited (h, w >= 2); see the head of this file
__host__ __device__ inline double nw_int_cost(int h, int w, uint32_t Sa, uint32_t Saa, uint32_t Sb, uint32_t Sbb, uint32_t Sab)
{
    const long long n = (long long)(h - 1) * (w - 1), q = 2 * n - (long long)h * w, n2 = n * n;
    const long long Ai = n2 * (long long)Saa - q * ((long long)Sa * Sa);
    const long long Bi = n2 * (long long)Sbb - q * ((long long)Sb * Sb);
    const long long Ci = n2 * (long long)Sab - q * ((long long)Sa * Sb);
    return (double)Ci / ((double)n * (sqrt((double)Ai) * sqrt((double)Bi)));
}

// Run g of G consecutive runs of the offsets 1 .. O, ceil(O / G) offsets each (the last ones may be short or empty:
// o_lo > o_hi).  The runs tile 1 .. O once, in order.
__host__ __device__ inline void nw_group(int O, int G, int g, int &o_lo, int &o_hi)
{
    const int per = (O + G - 1) / G;
    o_lo = 1 + g * per;
    o_hi = o_lo + per - 1 < O ? o_lo + per - 1 : O;
}

// The winner rule (NCC.h:261-266) over an ordered run of offsets: the running maximum starts at -2.0, o wins when
// res > max (a NaN never does, the first of equal costs stays).  The same statement combines the winners of consecutive
// runs of offsets in their order, which is how the kernels split the offsets over workgroups.
__host__ __device__ inline void nw_offer(double res, int o, double &best, int &best_o)
{
    if (res > best) { best = res; best_o = o; }
}
