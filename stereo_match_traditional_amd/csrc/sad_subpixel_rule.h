// The sub-pixel rule of the SAD family, shared by the kernels (sad_wave_subpixel in
// csrc/sad_select.h: csrc/window.hip, csrc/sad_both.hip) and the host twin smt_sad_subpixel_host, beside subpixel_rule.h
// whose spx_refine it applies.  SAD/Sad.h:76-81 fit the parabola through OptimalDisparity's winner and its two neighbours
// and drop the result; here it is kept.  Every cost is an integer below 2^24, so c1 + c2, 2 cm and their difference are
// exact and only the division and the final add round.
//
// Left view (OptimalDisparity, Sad.h:40-85), r = the integer the rule returns today (sad_optimal, csrc/sad_select.h):
//   r == 0      -> 0.0f       the uniqueness test :66, both ends of the range :71, D <= 2
//   r == 65535  -> 65535.0f   no entry with d >= 1 below 0xffff; the reference would index sad[65534]
//   else        -> spx_refine(r, D, sad[r-1], sad[r], sad[r+1], min_den); sad[0] takes no part in the search (:46), so
//                  sad[r-1] may lie below the minimum and the offset is then not bounded by 1/2: what :76-81 compute.
// Right view (GetMinSadIndex, Sad.h:22-38, on the row of :167-171 with its copied tail): w = the first strict minimum
// from d = 0, spx_refine(w, D, row[w-1], row[w], row[w+1], min_den); an end of the range keeps w.
// Both are one test: a parabola exists iff 0 < r < D - 1 (65535 >= D - 1 for every D the library takes).
#pragma once
#include "subpixel_rule.h"

SPX_HD int sad_spx_has_parabola(int r, int D) { return r > 0 && r < D - 1; }

// c1, cm, c2 are not read unless sad_spx_has_parabola(r, D)
SPX_HD float sad_spx_value(int r, int D, float c1, float cm, float c2, float min_den)
{
    return sad_spx_has_parabola(r, D) ? spx_refine(r, D, c1, cm, c2, min_den) : (float)r;
}

// OptimalDisparity (Sad.h:40-85) on one row in direct loops: what sad_optimal computes across a wave
SPX_HD int sad_optimal_row(const float *sad, int D)
{
    float minv = 65535.0f, best = 65535.0f;
    for (int i = 1; i < D; i++)
        if (minv > sad[i]) { minv = sad[i]; best = (float)i; }                // :46-53
    float sec = sad[0];
    for (int i = 0; i < D; i++)
        if (!(minv == sad[i])) sec = sad[i] < sec ? sad[i] : sec;              // :55-64, std::min(secMin, cost)
    if ((double)(sec - minv) <= 0.01) return 0;                               // :66
    if (best == 0.0f || best == (float)(D - 1)) return 0;                     // :71
    return (int)best;                                                         // :84
}

SPX_HD float sad_spx_row(int r, const float *row, int D, float min_den)
{
    return sad_spx_has_parabola(r, D) ? spx_refine(r, D, row[r - 1], row[r], row[r + 1], min_den) : (float)r;
}
