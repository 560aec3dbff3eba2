// FillTheHole's rules (AD-CensusV1/PostProcessing.h:156-248) as host/device inline functions: the one text that
// fill.hip (list form), fill_batch.hip (class-map form) and its host twin smt_fill_the_hole_batch_host all run.
//
// Geometry: the reference swaps the extents (`width = row`, `height = col`, :158-159); the buffer is addressed as
// `col` lines of `row` entries.  A target (y, x) is written at y * row + x (:244).
#pragma once
#include <cmath>
#include <stdint.h>

namespace fillrule {

#define FILL_HD __host__ __device__ __forceinline__

constexpr float HOLE = 65535.0f;                      // 0xffff, :182, :212

struct FillCfg {
    int width, height, maxlen;
    float sn[2][8], cs[2][8];
};

// sin/cos of the 16 float angles from the host libm (sinf/cosf: `sin(float)` is the float overload in C++)
static inline void cfg_init(FillCfg &c, int row, int col, int dispRange)
{
    c.width = row; c.height = col;                                           // :158-159
    c.maxlen = (int)(1.0 * dispRange);                                       // :168
    const float pi = 3.1415926f;
    const float angle1[8] = {pi, 3 * pi / 4, pi / 2, pi / 4, 0, 7 * pi / 4, 3 * pi / 2, 5 * pi / 4};
    const float angle2[8] = {pi, 5 * pi / 4, 3 * pi / 2, 7 * pi / 4, 0, pi / 4, pi / 2, 3 * pi / 4};
    for (int s = 0; s < 8; s++) {
        c.sn[0][s] = sinf(angle1[s]); c.cs[0][s] = cosf(angle1[s]);
        c.sn[1][s] = sinf(angle2[s]); c.cs[1][s] = cosf(angle2[s]);
    }
}

FILL_HD long lround_f(float v)                        // lround(float): half away from zero
{
    const double d = (double)v;                        // d +- 0.5 is exact in double
    return (long)(d + (d >= 0.0 ? 0.5 : -0.5));
}

// first entry != 65535 along ray s of set `set` from (y, x); false if the ray leaves the buffer first
FILL_HD bool ray(const float *__restrict__ disp, const FillCfg &c, int y, int x, int set, int s, float &val)
{
    const float sina = c.sn[set][s], cosa = c.cs[set][s];
    for (int m = 1; m < c.maxlen; m++) {
        const long yy = lround_f((float)y + (float)m * sina);
        const long xx = lround_f((float)x + (float)m * cosa);
        if (yy < 0 || yy >= c.height || xx < 0 || xx >= c.width) return false;
        const float d = disp[yy * c.width + xx];
        if (d != HOLE) { val = d; return true; }
    }
    return false;
}

// The reference's pick among the finds of the 8 rays (bit s of `found`: ray s found vals[s]): element `1 (or 0)` of
// the sorted finds for kind 0, element ng/2 for kind 1; 0.0f when nothing was found (:177, :218).  Equal values
// keep their ray order (std::sort on at most 8 elements is an insertion sort).
FILL_HD float pick(const float (&vals)[8], unsigned found, int kind)
{
    int ng = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) ng += (int)((found >> j) & 1u);
    const int want = (kind == 0) ? (ng > 1 ? 1 : 0) : ng / 2;
    float out = 0.0f;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (((found >> j) & 1u) && (vals[j] < vals[s] || (vals[j] == vals[s] && j < s))) rank++;
        if (((found >> s) & 1u) && rank == want) out = vals[s];
    }
    return ng == 0 ? 0.0f : out;
}

// ---- the class-map form: what LeftRightConsistency's lists (:86-134, row-major (i, j) with cls == k + 1) make of
// ---- FillTheHole's sequential state

// A class pixel (i, j) of a [row][col] map is written at i * row + j: outside the buffer that is an out-of-bounds
// write in the reference (:244; needs row > col).
FILL_HD bool out_of_buffer(int row, int col, int i, int j) { return (long)i * row + j >= (long)row * col; }

// Winner of address a in pass k (want = k + 1): the targets (i, j) with i * row + j == a are written in list order,
// the later one, i.e. the one with the largest i, stays (:241-246).  At most ceil(col / row) candidates.
FILL_HD bool winner(const uint8_t *__restrict__ cls, int row, int col, long a, int want, int &wi, int &wj)
{
    long i = a / row;
    if (i > row - 1) i = row - 1;
    for (long j = a - i * row; i >= 0 && j < col; i--, j += row)
        if (cls[i * col + j] == want) { wi = (int)i; wj = (int)j; return true; }
    return false;
}

// `angle` (:166) switches to angle2 at the first target whose first coordinate equals height / 2 = col / 2 and stays
// there, across targets and passes (:198-200).  In a row-major list that is every target with i >= col / 2 once the
// list has one in row col / 2 (mid_k), and every target once an earlier pass has switched.
FILL_HD int set_of_list_target(bool switched, bool mid_k, int i, int col) { return (switched || (mid_k && i >= col / 2)) ? 1 : 0; }
// pass 2 walks the holes in the swapped raster order: the same with `a hole on line col / 2` for mid
FILL_HD int set_of_hole(bool switched, bool mid_2, int y, int col) { return (switched || (mid_2 && y >= col / 2)) ? 1 : 0; }

// pass 2 tests the mismatch list (:174); `fill_disps` keeps that list's size (:178) while the hole list replaces it
// (:189): more holes than mismatches is an out-of-bounds write
FILL_HD bool third_pass_tested(int n_mis) { return n_mis > 0; }
FILL_HD bool third_pass_overruns(int n_mis, int n_third) { return n_third > n_mis; }

#ifdef __HIPCC__
// the 8 lanes of a group hold (found, val), lane & 7 = ray: everyone gets the group's pick
__device__ __forceinline__ float pick_group(bool found, float val, int kind)
{
    float vals[8];
    unsigned fm = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        vals[j] = __shfl(val, j, 8);
        fm |= (__shfl((int)found, j, 8) != 0 ? 1u : 0u) << j;
    }
    return pick(vals, fm, kind);
}
#endif

}  // namespace fillrule
