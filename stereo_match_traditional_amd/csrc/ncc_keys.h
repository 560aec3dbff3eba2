// The rank key of the both-view NCC (smt_lrncc, csrc/ncc_both.hip): WinTakeAll (NCC.h:53-67) of a right pixel as the
// MAXIMUM of 64-bit keys that the left view's cost kernels publish, one per real, non-NaN cost, in any order.
//
// WinTakeAll is sequential: m = (float)c[0], best = 0; for d >= 1: if ((double)m < c[d]) { best = d; m = (float)c[d]; }.
// With f[d] = (float)c[d] (round to nearest: monotone) and NaN costs skipped (every test against them is false):
//   * a winner raises m to its own f, and f >= m for it, so m before step d is the maximum of f over the earlier
//     hypotheses; F = max f is reached at d* = the first d with f[d] == F, which wins (f[d*] > m implies c[d*] > m);
//   * after d* a hypothesis wins iff c[d] > (double)F, and then f[d] == F (f[d] <= F, and f[d] < F would put c[d]
//     below F): these are the costs that were rounded DOWN to F.  m stays F.  No such d lies before d*.
// So the answer is the LAST d with c[d] > (double)F if there is one, else the FIRST d with f[d] == F.  The key orders
// exactly that: the order-preserving image of f on top; below it, for a cost rounded down (`up`), bit 31 and d -- the
// largest d wins among them and each of them beats the others -- and otherwise 0x7fffffff - d, the smallest d wins.
// Every key is above 0 (the image of -inf is 0x007fffff): 0 in the map means that nothing was published.
// What the key does not carry is resolved where the map is read (k_lrncc_finish): a NaN at d = 0 gives 0, and a pixel
// with sentinel hypotheses gets the first of them.  smt_lrncc_selftest_keys holds all of it to the sequential loop.
#pragma once
#include <stdint.h>

__host__ __device__ inline unsigned long long ncc_rank_key(double c, int d)
{
    const float f = (float)c + 0.0f;                       // -0 -> +0: equal zeros tie
    unsigned b;
    __builtin_memcpy(&b, &f, 4);
    const unsigned hi = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    const unsigned lo = c > (double)f ? (0x80000000u | (unsigned)d) : (0x7FFFFFFFu - (unsigned)d);
    return ((unsigned long long)hi << 32) | lo;
}

// the hypothesis a key names
__host__ __device__ inline int ncc_rank_key_d(unsigned long long key)
{
    const unsigned lo = (unsigned)key;
    return (int)((lo & 0x80000000u) ? (lo & 0x7FFFFFFFu) : (0x7FFFFFFFu - lo));
}
