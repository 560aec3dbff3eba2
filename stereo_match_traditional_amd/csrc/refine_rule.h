// Region voting and outlier interpolation (include/smt_refine.h has the rule in words; parity unpinned: no reference
// code) as host/device inline functions: the one text that the kernels of refine.hip and the host twins run.
#pragma once
#include <stdint.h>

namespace refinerule {

#if defined(__HIPCC__)
#define RF_HD __host__ __device__ __forceinline__
#else
#define RF_HD static inline
#endif

constexpr int ARM_MAX = 255;                 // every arm length is clamped into 0..ARM_MAX
constexpr int RAYS = 16;

// reliable iff v >= 0.0f && v < (float)D: false for NaN, +-inf and (float)INT_MIN, true for -0.0f
RF_HD bool reliable(float v, int D) { return v >= 0.0f && v < (float)D; }

// min(D-1, (int)(v + 0.5f)) of a reliable v: one float addition, truncation
RF_HD int bin_of(float v, int D)
{
    const int b = (int)(v + 0.5f);
    return b < D - 1 ? b : D - 1;
}

RF_HD bool arm_out_of_range(int a) { return a < 0 || a > ARM_MAX; }
RF_HD int arm_clamp(int a) { return a < 0 ? 0 : (a > ARM_MAX ? ARM_MAX : a); }

// first and last row / column of a region along one axis: centre c, the two clamped arms, extent n
RF_HD int span_lo(int c, int arm) { const int lo = c - arm_clamp(arm); return lo < 0 ? 0 : lo; }
RF_HD int span_hi(int c, int arm, int n) { const int hi = c + arm_clamp(arm); return hi > n - 1 ? n - 1 : hi; }

// M'(p) = (float)d* iff S > irv_ts and (double)h > (double)irv_th * (double)S
RF_HD bool vote_fills(int S, int h, int irv_ts, float irv_th)
{
    return S > irv_ts && (double)h > (double)irv_th * (double)S;
}

// the 16 steps, 3 bits each, value + 2:
//   dy  0 1 1 2  1 2 1 1  0 -1 -1 -2  -1 -2 -1 -1
//   dx  1 2 1 1  0 -1 -1 -2  -1 -2 -1 -1  0 1 1 2
RF_HD int ray_dy(int n)
{
    const unsigned long long t = 2ull | 3ull << 3 | 3ull << 6 | 4ull << 9 | 3ull << 12 | 4ull << 15 | 3ull << 18 | 3ull << 21 |
                                 2ull << 24 | 1ull << 27 | 1ull << 30 | 0ull << 33 | 1ull << 36 | 0ull << 39 | 1ull << 42 | 1ull << 45;
    return (int)((t >> (3 * n)) & 7) - 2;
}
RF_HD int ray_dx(int n)
{
    const unsigned long long t = 3ull | 4ull << 3 | 3ull << 6 | 3ull << 9 | 2ull << 12 | 1ull << 15 | 1ull << 18 | 0ull << 21 |
                                 1ull << 24 | 0ull << 27 | 1ull << 30 | 1ull << 33 | 2ull << 36 | 3ull << 39 | 3ull << 42 | 4ull << 45;
    return (int)((t >> (3 * n)) & 7) - 2;
}

// Ray n of pixel (i, j) on map m: the flat index of its candidate, the first reliable probe, or -1
RF_HD long long ray_candidate(const float *m, int H, int W, int D, int i, int j, int n, int search)
{
    const int dy = ray_dy(n), dx = ray_dx(n);
    int y = i + dy, x = j + dx;
    for (int k = 1; y >= 0 && y < H && x >= 0 && x < W && (search <= 0 || k <= search); k++, y += dy, x += dx)
        if (reliable(m[(long long)y * W + x], D)) return (long long)y * W + x;
    return -1;
}

// The order in which candidates compete, smaller wins, ties go to the lower ray: class 1 (occlusion) by value -- a
// reliable value is >= 0, so its bits order as unsigned once -0.0f has become +0.0f -- every other class by
// |gray(p) - gray(q)|.  0xFFFFFFFF is above every key.
RF_HD unsigned cand_key(bool occlusion, unsigned value_bits, int gray_p, int gray_q)
{
    if (occlusion) return value_bits == 0x80000000u ? 0u : value_bits;
    const int d = gray_p - gray_q;
    return (unsigned)(d < 0 ? -d : d);
}

}  // namespace refinerule
