// The SAD selection rules shared by the tap-loop kernels (csrc/window.hip) and the box-sum kernel (csrc/sad_both.hip).
#pragma once
#include "smt_common.h"
#include "sad_subpixel_rule.h"
#include "../../include/smt_sad_subpixel.h"

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

// The sub-pixel value of the wave-distributed row for the wave-uniform integer r its selection rule returned
// (sad_subpixel_rule.h; either view: the right view's row holds its copied tail).  The neighbours sit in lane d & 63,
// slot d >> 6: every slot of that lane is read with v_readlane and an unrolled scalar select on the wave-uniform slot
// picks one, as wave_wta_subpixel does (sad[d >> 6] would move the row to LDS).  Returned wave-uniform.
template <int KS>
__device__ __forceinline__ float sad_wave_subpixel(const float (&sad)[KS], int r, int D, float min_den)
{
    r = __builtin_amdgcn_readfirstlane(r);
    if (!sad_spx_has_parabola(r, D)) return (float)r;
    auto at = [&](int d) {
        const int l = d & 63, s = d >> 6;
        int x = __builtin_amdgcn_readlane(__float_as_int(sad[0]), l);
#pragma unroll
        for (int k = 1; k < KS; k++) {
            const int xk = __builtin_amdgcn_readlane(__float_as_int(sad[k]), l);
            x = (s == k) ? xk : x;
        }
        return __int_as_float(x);
    };
    return spx_refine(r, D, at(r - 1), at(r), at(r + 1), min_den);
}

// one pixel's results: the integer map alone (SUB = false: the code of before), or the float map and, when asked for, the
// integer winner
template <bool SUB>
__device__ __forceinline__ void sad_store(size_t p, int lane, int out, float f, int32_t *__restrict__ disp, float *__restrict__ sub)
{
    if (SUB) {
        if (lane == 0) {
            sub[p] = f;
            if (disp) disp[p] = out;
        }
    } else if (lane == 0) disp[p] = out;
}
