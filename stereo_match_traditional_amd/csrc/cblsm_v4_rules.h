// chooseArmLength{Left,Right,Up,Down} (CBLSM/CBLSM.h:65-236) and costAggregationV4's rectangle (:1128-1176) as
// host/device inline functions: the one text that cblsm_v4.hip's fused kernel and its host twin
// (smt_cblsm_selftest_v4, which holds them against the reference's loops) both run.
//
// Names: LL, LR, LUp, LDown are the LEFT image's arms at the pixel (i, j); rl, rr, RUp, RDown the RIGHT image's arms at
// the SAME pixel (column j, not j - d: the reference's indexing); d >= 0 is the hypothesis.  Every comparison keeps the
// reference's strictness, with the `j` both sides carry cancelled.
#pragma once
#include <stdint.h>

namespace v4rule {

#define V4_HD __host__ __device__ __forceinline__

// chooseArmLengthLeft (:65-102).  0 when d > rl or d > rr (:77); otherwise the walk a = 1..LL counts while
// j-a-d >= j-rl (a <= rl - d) and j-a-d <= j+rr (always: a, d, rr >= 0 past the guard) and breaks at the first miss:
// min(LL, rl - d), and rl - d >= 0 past the guard.
V4_HD int arm_left(int LL, int rl, int rr, int d)
{
    if (d > rl || d > rr) return 0;
    const int n = LL < rl - d ? LL : rl - d;
    return n < 0 ? 0 : n;
}

// chooseArmLengthRight (:104-147).  0 when d > rl or -d > rr (:123); otherwise a = 1..LR counts while j+a-d >= j-rl
// (always: d <= rl) and j+a-d < j+rr (a <= rr + d - 1): min(LR, rr + d - 1), floored at 0.
V4_HD int arm_right(int LR, int rl, int rr, int d)
{
    if (d > rl || -d > rr) return 0;
    const int n = LR < rr + d - 1 ? LR : rr + d - 1;
    return n < 0 ? 0 : n;
}

// chooseArmLengthUp (:151-192): rows i-1 .. i-LUp.  A row past RUp resets the count to 0 and stops (:180-184), so the
// whole walk yields 0 whenever LUp > RUp; otherwise every one of the LUp rows is visited -- a miss does not break -- and
// counts when j-d < j+rr' and j-d > j-rl' with rl', rr' the RIGHT image's horizontal arms on that row (strict, :175).
// j - d < 0 breaks at the first row with the count still 0 (:171-174).
V4_HD int up_rows(int LUp, int RUp) { return (LUp > RUp || LUp < 0) ? 0 : LUp; }
V4_HD int up_hit(int d, int rl_row, int rr_row) { return (-d < rr_row && d < rl_row) ? 1 : 0; }

// chooseArmLengthDown (:195-236): rows i+1 .. i+LDown.  A row past RDown stops and KEEPS the count (:225-228), so
// min(LDown, RDown) rows are visited; a row counts when j-d <= j+rr' and j-d >= j-rl' (non-strict, :220).  j - d < 0
// zeroes the count (:215-219).
V4_HD int down_rows(int LDown, int RDown) { const int n = LDown < RDown ? LDown : RDown; return n < 0 ? 0 : n; }
V4_HD int down_hit(int d, int rl_row, int rr_row) { return (-d <= rr_row && d <= rl_row) ? 1 : 0; }

// The two walks for one hypothesis; rl, rr point at the RIGHT image's horizontal arm maps at (i, j), W is the row
// stride.  The fused kernel runs the same rows / hit functions with the row loop shared by a lane's hypotheses.
V4_HD int arm_up(int LUp, int RUp, const int *rl, const int *rr, int W, int j, int d)
{
    if (j - d < 0) return 0;
    int n = 0;
    for (int t = 1, e = up_rows(LUp, RUp); t <= e; t++) n += up_hit(d, rl[-(long)t * W], rr[-(long)t * W]);
    return n;
}
V4_HD int arm_down(int LDown, int RDown, const int *rl, const int *rr, int W, int j, int d)
{
    if (j - d < 0) return 0;
    int n = 0;
    for (int t = 1, e = down_rows(LDown, RDown); t <= e; t++) n += down_hit(d, rl[(long)t * W], rr[(long)t * W]);
    return n;
}

// costAggregationV4's rectangle (:1162-1169): rows [i-Up, i+Down), columns [j-L, j+R), half-open on the far side, as
// corners of a summed-area table S (S[p] = sum over rows <= p's row and columns <= p's column):
// sum = S[c0] - S[c1] - S[c2] + S[c3], c = pixel index or -1 for a row / column before the image (contributes 0);
// n = (Up+Down)(L+R) its tap count, 0 for an empty rectangle (then c is unused and the mean is 0.0f / 0 = NaN).  A
// rectangle that leaves the plane is clipped to it and the function returns true -- never the case for the arms above,
// which are bounded by the left image's own arms.
V4_HD bool box(int i, int j, int L, int R, int Up, int Down, int H, int W, int (&c)[4], int &n)
{
    int r0 = i - Up, r1 = i + Down, c0 = j - L, c1 = j + R;
    n = 0;
    c[0] = c[1] = c[2] = c[3] = -1;
    if (r1 <= r0 || c1 <= c0) return false;
    const bool clip = r0 < 0 || r1 > H || c0 < 0 || c1 > W;
    r0 = r0 < 0 ? 0 : r0; r1 = r1 > H ? H : r1; c0 = c0 < 0 ? 0 : c0; c1 = c1 > W ? W : c1;
    if (r1 <= r0 || c1 <= c0) return true;
    n = (r1 - r0) * (c1 - c0);
    c[0] = (r1 - 1) * W + c1 - 1;
    if (r0 > 0) c[1] = (r0 - 1) * W + c1 - 1;
    if (c0 > 0) c[2] = (r1 - 1) * W + c0 - 1;
    if (r0 > 0 && c0 > 0) c[3] = (r0 - 1) * W + c0 - 1;
    return clip;
}

// hypothesis d of the rectangle whose corners box() gave (n > 0), in uint32 (mod 2^32) arithmetic
V4_HD uint32_t box_sum(const uint32_t *__restrict__ S, size_t D, const int (&c)[4], int d)
{
    uint32_t s = S[(size_t)c[0] * D + d];
    if (c[1] >= 0) s -= S[(size_t)c[1] * D + d];
    if (c[2] >= 0) s -= S[(size_t)c[2] * D + d];
    if (c[3] >= 0) s += S[(size_t)c[3] * D + d];
    return s;
}

}  // namespace v4rule
