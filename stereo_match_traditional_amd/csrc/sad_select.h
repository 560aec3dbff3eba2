// The SAD selection rules shared by the tap-loop kernels (csrc/window.hip) and the box-sum kernel (csrc/sad_both.hip).
#pragma once
#include "smt_common.h"

// wave minimum of non-negative floats (SAD sums, 65535, +inf): for v >= +0 the bit patterns order like
// the values, so this is the DPP integer reduction (no LDS-crossbar shuffles)
__device__ __forceinline__ float wave_min_nonneg(float v) { return __uint_as_float(wave_min_u32(__float_as_uint(v))); }

// OptimalDisparity (Sad.h:40-85) over the wave-distributed vector sad[d], d = lane+64k.  KS = KMAX for D <= 256,
// 8 (the hypothesis slots of SMT_MAX_DISPARITY) beyond.
template <int KS>
__device__ int sad_optimal(const float (&sad)[KS], int D, int lane)
{
    // min over d >= 1, first strict (:46-53), starting from 0xffff
    float lm = 65535.0f; int ld = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < KS; k++) {
        const int d = lane + 64 * k;
        if (d >= 1 && d < D && lm > sad[k]) { lm = sad[k]; ld = d; }
    }
    const float minv = wave_min_nonneg(lm);
    // first d >= 1 whose value equals the minimum (if any value beat 65535)
    int cand = (lm == minv && ld != 0x7fffffff) ? ld : 0x7fffffff;
    cand = (int)wave_min_u32((unsigned)cand);
    const float best = (cand == 0x7fffffff) ? 65535.0f : (float)cand;
    // second minimum: starts at sad[0]; every entry equal to minv is skipped (:55-64)
    float ls = INFINITY;
#pragma unroll
    for (int k = 0; k < KS; k++) {
        const int d = lane + 64 * k;
        if (d < D && !(minv == sad[k])) ls = fminf(ls, sad[k]);
    }
    const float s0 = __shfl(sad[0], 0, WAVE);
    const float sec = fminf(s0, wave_min_nonneg(ls));
    if ((double)(sec - minv) <= 0.01) return 0;                           // :66
    if (best == 0.0f || best == (float)(D - 1)) return 0;                 // :71
    return (int)best;                                                     // :84
}
