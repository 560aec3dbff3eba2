// The arithmetic of ASW/BiliteralFilter.h:49-142 that the kernels of csrc/bilateral.hip and the host twin
// smt_bilateral_filter_host share (include/smt_bilateral.h states the rule).  float64, one
// rounding per operation: the library is built with -ffp-contract=off and nothing here may be reassociated.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BIL_HD __host__ __device__ __forceinline__
#else
#define BIL_HD inline
#endif

// the source position of a tap: copyMakeBorder(BORDER_REPLICATE) (:63) as a clamp of the index
BIL_HD int bil_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

// the colour table's index, :76 / :85
BIL_HD int bil_diff(int q, int centre)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // unsigned: the compiler takes minimum, maximum and difference of the sample bytes as they lie in the loaded words
    return (int)__usad((unsigned)q, (unsigned)centre, 0u);
#else
    const int d = q - centre;
    return d < 0 ? -d : d;
#endif
}

// :78 / :89-91: the weight of a tap before normalisation
BIL_HD double bil_weight(double color_entry, double space_entry) { return color_entry * space_entry; }

// what multiplies or divides every weight of a pixel: 1.0 / S under the reciprocal norm, S itself under the divide norm
BIL_HD double bil_norm_operand(double S, int divide) { return divide ? S : 1.0 / S; }

// :100-106, Mask = Mask / S
BIL_HD double bil_normalise(double wt, double operand, int divide) { return divide ? wt / operand : wt * operand; }

// :113 / :117-119, one step of pass 2
BIL_HD double bil_accumulate(double acc, int q, double wn) { return acc + (double)q * wn; }

// :124-137: clamp, then truncation toward zero; a NaN passes both comparisons and gives 0 (decided defect)
BIL_HD uint8_t bil_output(double acc)
{
    if (acc != acc) return 0;
    if (acc < 0) acc = 0;
    else if (acc > 255) acc = 255;
    return (uint8_t)acc;
}
