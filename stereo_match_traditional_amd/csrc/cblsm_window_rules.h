// ComputeDispLeft / ComputeDispRight / ComputeDispV4 (CBLSM/CBLSM.h:451-489, :409-447, :494-532) and their helpers
// sadvalueMean (:17-22) and sadvalueMeanV4 (:24-63) as host/device inline functions: the one text that the kernels of
// cblsm_window.hip and the host twin smt_cblsm_window_cost_host both run -- which hypothesis an entry repeats (the
// `cost = last` chains), the quotient, and V4's channel minimum and uchar wrap.
//
// Names: w = winSize + 1, side = 2 w + 1, n = side^2; (y, x) an unpadded pixel, d >= 0 the hypothesis; the images are
// replicate-padded by w, so the window of column c covers padded columns c .. c + 2 w.
#pragma once
#include <stdint.h>

namespace cwrule {

#define CW_HD __host__ __device__ __forceinline__

enum { MAX_SIDE = 181 };   // 255 * 181^2 = 8 354 055 < 2^24: (float)S is exact

// LEFT and V4 (:476-481, :519-524): `j - win_r - d < 0`, that is d > x, copies the element before it, which is in the
// same pixel's vector (d >= 1 there), so entry d holds hypothesis min(d, x).
CW_HD int left_src(int x, int d) { return d < x ? d : x; }

// RIGHT (:434-439): `j + d + win_r + 1 > colrange` with j = x + w, colrange = W + w (the padded width less winsize + 1)
// is x + d > W - 1 - w: the view stops w columns before its data does.  lim = W - 1 - w - x.
//   lim >= 0: entry d holds hypothesis min(d, lim) of the pixel's own column;
//   lim <  0: d = 0 copies too, from the element BEFORE the pixel's vector, the previous pixel's entry D - 1; walking
//             back along the row, every entry of the last w columns holds hypothesis 0 of column W - 1 - w.
// W <= w has no such column (the walk leaves the buffer): the callers reject it as SMT_ERR_REF_UB.
CW_HD void right_src(int x, int d, int W, int w, int &xs, int &ds)
{
    const int lim = W - 1 - w - x;
    if (lim >= 0) { xs = x; ds = d < lim ? d : lim; }
    else { xs = W - 1 - w; ds = 0; }
}
CW_HD bool right_defined(int W, int w) { return W > w; }

// sadvalueMean: the float nearest to S / n.  cv::mean is a double sum times a double reciprocal, narrowed to float;
// for integer S <= 255 n, n <= 181^2 that equals (float)((double)S / n) and the IEEE float quotient below for every S
// (tests/test_cblsm_window_cpu.py sweeps all three).  (float)S is exact: S < 2^24.
CW_HD float quotient(uint32_t S, int n) { return (float)S / (float)n; }

// minValue (:24-44): the smallest of the three channel differences (its T is unused)
CW_HD unsigned min3(unsigned a, unsigned b, unsigned c)
{
    const unsigned m = a < b ? a : b;
    return m < c ? m : c;
}

// sadvalueMeanV4 (:46-63): the taps add into a uchar (mod 256), the mean is an integer division, returned as float
CW_HD float v4_cost(uint32_t sum, int n) { return (float)((sum & 255u) / (uint32_t)n); }

CW_HD unsigned absdiff_u8(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

// |Lp - Rp| summed over the side x side windows at padded columns xa (left image) and xb (right image) of rows
// y .. y + side - 1; Wp = W + 2 w is the row stride.  The direct formulation: the tap-loop kernel and the host twin.
CW_HD uint32_t window_sum(const uint8_t *Lp, const uint8_t *Rp, int Wp, int y, int xa, int xb, int side)
{
    uint32_t acc = 0;
    for (int r = 0; r < side; r++) {
        const uint8_t *a = Lp + (size_t)(y + r) * Wp + xa, *b = Rp + (size_t)(y + r) * Wp + xb;
        for (int c = 0; c < side; c++) acc += absdiff_u8(a[c], b[c]);
    }
    return acc;
}

// the same for 3-channel images [Hp][Wp][3] with the channel minimum per tap
CW_HD uint32_t window_sum_v4(const uint8_t *Lp, const uint8_t *Rp, int Wp, int y, int xa, int xb, int side)
{
    uint32_t acc = 0;
    for (int r = 0; r < side; r++) {
        const uint8_t *a = Lp + ((size_t)(y + r) * Wp + xa) * 3, *b = Rp + ((size_t)(y + r) * Wp + xb) * 3;
        for (int c = 0; c < side; c++)
            acc += min3(absdiff_u8(a[3 * c], b[3 * c]), absdiff_u8(a[3 * c + 1], b[3 * c + 1]), absdiff_u8(a[3 * c + 2], b[3 * c + 2]));
    }
    return acc;
}

// One entry vol[y][x][d] of a form (SMT_CBLSM_COST_LEFT = 1, _RIGHT = 2, _V4 = 3), by the rules above and the direct sum.
CW_HD float entry(int form, const uint8_t *Lp, const uint8_t *Rp, int W, int w, int y, int x, int d)
{
    const int side = 2 * w + 1, Wp = W + 2 * w, n = side * side;
    if (form == 2) {
        int xs, ds;
        right_src(x, d, W, w, xs, ds);
        return quotient(window_sum(Lp, Rp, Wp, y, xs + ds, xs, side), n);
    }
    const int ds = left_src(x, d);
    if (form == 3) return v4_cost(window_sum_v4(Lp, Rp, Wp, y, x, x - ds, side), n);
    return quotient(window_sum(Lp, Rp, Wp, y, x, x - ds, side), n);
}

}  // namespace cwrule
