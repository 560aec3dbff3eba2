// The sub-pixel rule of the library, shared by the kernels (wave_wta_subpixel in smt_common.h:
// csrc/subpixel.hip, csrc/scanline.hip, csrc/crossarm.hip) and the host twin smt_wta_subpixel_host, the way
// fill_image_rules.h is.  It is the parabola through the winner and its two neighbours that SAD/Sad.h:76-81 and
// CBLSM/CBLSM.h:285-290 compute and then drop (they return best_disp):
//   divided = max(min_den, cost1 + cost2 - 2 * min);  final = best + (cost1 - cost2) / (2 * divided)
// with the reference's literal 1 as the parameter min_den.  float32, one rounding per operation, in this order; 2 * cm
// and 2 * den are exact.  Decided cases: a winner at either end of the range has no parabola and is kept; a NaN sum
// takes min_den (std::max(min_den, s) is `min_den < s ? s : min_den`); a non-finite offset keeps the winner.
#pragma once

#ifdef __HIPCC__
#define SPX_HD __host__ __device__ static inline
#else
#define SPX_HD static inline
#endif

// min_den a caller may pass: finite and greater than 0
SPX_HD int spx_min_den_ok(float min_den) { return __builtin_isfinite(min_den) && min_den > 0.0f; }

// w = the winner of the row (smt_wta's rule), c1 = c[w - 1], cm = c[w], c2 = c[w + 1]; c1 and c2 are not read when w is
// 0 or D - 1
SPX_HD float spx_refine(int w, int D, float c1, float cm, float c2, float min_den)
{
    const float fw = (float)w;
    if (w == 0 || w == D - 1) return fw;
    const float s = (c1 + c2) - 2.0f * cm;
    const float den = (min_den < s) ? s : min_den;
    const float off = (c1 - c2) / (2.0f * den);
    return __builtin_isfinite(off) ? fw + off : fw;
}

// the winner of one row by smt_wta's rule (CrossArm.cpp:44-52): the first strict minimum; a NaN never wins, a NaN at
// d = 0 freezes the result at 0; -0 ties +0
SPX_HD int spx_winner(const float *c, int D)
{
    float cost = c[0];
    int best = 0;
    for (int d = 1; d < D; d++)
        if (cost > c[d]) { cost = c[d]; best = d; }
    return best;
}
