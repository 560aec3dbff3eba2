// Median selection by compare-exchange networks for the 3 x 3 and 5 x 5 windows of smt_median_blur_u8_batch: after the
// exchanges (a, b) -> (min, max) in order, slot K * K / 2 holds the median.  19 exchanges for 9 values, 99 for 25 (the
// counts of the classic hand-optimised networks; a selection network is correct for every input if it is correct for
// every input of zeros and ones, which smt_median_blur_selftest_nets checks exhaustively on the host: 2^9 and 2^25).
// Shared by the kernel (on packed pairs of 16-bit lanes) and that check.
#pragma once

#ifdef __HIPCC__
#define MEDNET_HD __host__ __device__
#else
#define MEDNET_HD
#endif

template <int N> struct mednet;

template <> struct mednet<9> {
    static constexpr int NX = 19;
    MEDNET_HD static constexpr int a(int i)
    {
        constexpr int t[NX] = {1, 4, 7, 0, 3, 6, 1, 4, 7, 0, 5, 4, 3, 1, 2, 4, 4, 6, 4};
        return t[i];
    }
    MEDNET_HD static constexpr int b(int i)
    {
        constexpr int t[NX] = {2, 5, 8, 1, 4, 7, 2, 5, 8, 3, 8, 7, 6, 4, 5, 7, 2, 4, 2};
        return t[i];
    }
};

template <> struct mednet<25> {
    static constexpr int NX = 99;
    MEDNET_HD static constexpr int a(int i)
    {
        constexpr int t[NX] = {0, 3, 2, 2, 6, 5, 5, 9, 8, 8, 12, 11, 11, 15, 14, 14, 18, 17, 17, 21, 20, 20, 23, 2, 3,
                               0, 0, 4, 1, 1, 11, 8, 8, 12, 9, 9, 13, 10, 10, 20, 17, 17, 21, 18, 18, 19, 8, 9, 0, 0,
                               10, 1, 1, 11, 2, 2, 12, 3, 3, 13, 4, 4, 14, 5, 5, 15, 6, 6, 7, 7, 13, 15, 7, 7, 1,
                               3, 5, 11, 9, 4, 6, 7, 4, 4, 12, 10, 6, 10, 6, 6, 12, 7, 7, 12, 7, 10, 12, 10, 10};
        return t[i];
    }
    MEDNET_HD static constexpr int b(int i)
    {
        constexpr int t[NX] = {1, 4, 4, 3, 7, 7, 6, 10, 10, 9, 13, 13, 12, 16, 16, 15, 19, 19, 18, 22, 22, 21, 24, 5, 6,
                               6, 3, 7, 7, 4, 14, 14, 11, 15, 15, 12, 16, 16, 13, 23, 23, 20, 24, 24, 21, 22, 17, 18, 18, 9,
                               19, 19, 10, 20, 20, 11, 21, 21, 12, 22, 22, 13, 23, 23, 14, 24, 24, 15, 16, 19, 21, 23, 13, 15, 9,
                               11, 17, 17, 17, 10, 12, 14, 6, 7, 14, 14, 7, 12, 10, 17, 17, 17, 10, 18, 12, 18, 20, 20, 12};
        return t[i];
    }
};

// p[0 .. N-1] -> the median in p[N / 2]; MIN and MAX are the element-wise operations of the value type.
template <int N, class T, class MIN, class MAX>
MEDNET_HD inline void mednet_run(T *p, MIN mn, MAX mx)
{
#pragma unroll
    for (int i = 0; i < mednet<N>::NX; i++) {
        const int a = mednet<N>::a(i), b = mednet<N>::b(i);
        const T lo = mn(p[a], p[b]), hi = mx(p[a], p[b]);
        p[a] = lo;
        p[b] = hi;
    }
}
