// The fused first horizontal pass of smt_crossagg_flow_run_batch, as arithmetic shared by the kernel (k_caf_first,
// crossagg.hip) and the host self-test (smt_crossagg_selftest_first_pass): both instantiate ca1_walk below, the kernel
// with an LDS ring and one hypothesis per lane, the self-test with an array and one hypothesis at a time.
//
// The pass sums ComputeAD / ComputeADRight costs (CBLSM.h:327-381, integers 0..255) along the horizontal arm of every
// pixel (cross_aggregator.cpp:362-364).  Arms are uint8, so a sum has at most 511 taps and stays below 2^24: the
// reference's sequential float adds are exact, in any order, and equal the integer sum converted once.  Per (row,
// hypothesis) the walk keeps the running prefix P[u] = sum of the costs of columns <= u and gives pixel x the difference
// P[x + right] - P[x - left - 1].  The ring holds the prefixes as uint16: a difference of two prefixes is exact modulo
// 2^16 while the true value is below 2^16, which holds for up to 257 taps of 255, not for 511 -- so the difference is
// taken in two halves, (P[x + right] - P[x]) with at most 255 taps and (P[x] - P[x - left - 1]) with at most 256, each
// exact modulo 2^16, and the halves are added in 32 bits.
#pragma once
#include <stdint.h>

constexpr int CA1_SEG = 256;   // output pixels of one walk (the kernel's wave); a walk starts its prefix Lm columns early
constexpr int CA1_G = 4;       // columns per group of a walk

// the largest arm a row of W pixels can hold under the limit L1 (cross_aggregator.cpp's MAX_ARM_LENGTH is 255)
__host__ __device__ inline int ca1_arm_bound(int L1, int W)
{
    const int m = L1 < 255 ? L1 : 255;
    return m < W - 1 ? m : W - 1;
}
// ring entries a walk needs: positions x - Lm - 1 .. x + Lm around the pixel it emits
__host__ __device__ inline int ca1_ring_depth(int Lm) { return 2 * Lm + 2; }

// column of the other image for tap column u and hypothesis d: view 0 pairs L[u] with R[max(u - d, 0)] (the chain of
// CBLSM.h:340-344 copies the cost of d - 1 while u - d < 0, which ends at the hypothesis d = u), view 1 pairs R[u] with
// L[min(u + d, W - 1)] (:368-372).  u -/+ d never leaves the row on the other side, so one clamp serves both; the
// kernel stages the other row's bytes through ca1_clamp once and then indexes them by u -/+ d.
__host__ __device__ inline int ca1_clamp(int c, int W) { return c < 0 ? 0 : (c > W - 1 ? W - 1 : c); }
__host__ __device__ inline int ca1_other(int view, int u, int d, int W) { return ca1_clamp(view == 0 ? u - d : u + d, W); }

__host__ __device__ inline uint32_t ca1_step(uint32_t P, uint32_t own, uint32_t oth)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __usad(own, oth, P);                                         // v_sad_u32: P + |own - oth|
#else
    return P + (own > oth ? own - oth : oth - own);
#endif
}

// hi, mid, lo: the ring's entries for x + right, x and x - left - 1 (uint16 values, zero-extended)
__host__ __device__ inline float ca1_out(uint32_t hi, uint32_t mid, uint32_t lo)
{
    return (float)(((hi - mid) & 0xFFFFu) + ((mid - lo) & 0xFFFFu));
}

// One walk: outputs x in [xs, xe) of one row for one hypothesis (per lane on the device; everything but the values is
// wave-uniform there).  own(u) / oth(u): the two bytes of tap column u; arm(x, l, r): the pixel's left / right arm;
// st(slot, P) / ld(slot): the ring of ca1_ring_depth(Lm) uint16 entries; emit(x, v).  Arms are clipped to the row and
// to Lm, which the arm kernel guarantees anyway and which keeps every ring index inside the ring whatever the map holds.
// Columns go in groups of G: a group's bytes and arms are fetched before its steps, so that on the device one wait
// covers G columns' loads and the ring traffic of the steps queues behind it.
template <int G, class Own, class Oth, class Arm, class St, class Ld, class Emit>
__host__ __device__ inline void ca1_walk(int xs, int xe, int W, int Lm, Own own, Oth oth, Arm arm, St st, Ld ld, Emit emit)
{
    const int RD = ca1_ring_depth(Lm);
    const int ub = xs - Lm > 0 ? xs - Lm : 0;                           // first and last tap column
    const int ue = xe - 1 + Lm < W - 1 ? xe - 1 + Lm : W - 1;
    auto out = [&](int x, int l, int r, int cs, int u) {                // cs: the slot of column u, the newest entry
        l = l < Lm ? l : Lm; l = l < x ? l : x; l = l < 0 ? 0 : l;
        r = r < Lm ? r : Lm; r = r < W - 1 - x ? r : W - 1 - x; r = r < 0 ? 0 : r;
        auto slot = [&](int col) { const int s = cs - (u - col); return s < 0 ? s + RD : s; };
        emit(x, ca1_out(ld(slot(x + r)), ld(slot(x)), ld(slot(x - l - 1))));
    };
    uint32_t P = 0;
    int cs = 0;
    st(cs, P);                                                          // column ub - 1: the empty prefix
    for (int u0 = ub; u0 <= ue; u0 += G) {
        uint32_t a[G], b[G];
        int l[G], r[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            const int u = u0 + k, x = u - Lm;                           // x: the pixel whose window ends at or before u
            a[k] = b[k] = 0; l[k] = r[k] = 0;
            if (u <= ue) {
                a[k] = own(u); b[k] = oth(u);
                if (x >= xs && x < xe) arm(x, l[k], r[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < G; k++) {
            const int u = u0 + k, x = u - Lm;
            if (u <= ue) {
                P = ca1_step(P, a[k], b[k]);
                cs = cs + 1 == RD ? 0 : cs + 1;
                st(cs, P);
                if (x >= xs && x < xe) out(x, l[k], r[k], cs, u);
            }
        }
    }
    for (int x = (ue - Lm + 1 > xs ? ue - Lm + 1 : xs); x < xe; x++) {  // windows cut by the row's end
        int l, r;
        arm(x, l, r);
        out(x, l, r, cs, ue);
    }
}
