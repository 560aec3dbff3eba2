// MedianFilter(d, d, ...) -- AD-CensusV1/PostProcessing.h:314-344 called with in == out -- as a parallel schedule:
// the one text that the kernels of median_inplace.hip and their host twin smt_median_filter_inplace_host all run.
//
// The aliased call is a recurrence in raster order: the window of pixel (i, j) holds filtered values in the rows above
// and to the left on its own row, unfiltered values everywhere else.  With r = wnd_size / 2 pixel (i, j) gets the step
// number t = i * (r + 1) + j.  Row i - k is then at column j + k (r + 1) > j + r: every filtered value (i, j) reads has
// a smaller step number; row i + k is at column j - k (r + 1) < j - r: every unfiltered value it reads is overwritten
// at a larger one.  Steps in order, each step's reads before its writes, give the raster result.
//
// Bands: a workgroup has one thread per row, so maps taller than a band run band after band.  Inside a band the step
// number counts from the band's first row; the rows above the band are final (read after a workgroup barrier), the
// rows below it untouched.
//
// Two formulations:
//   plain (impl 1)  every step reads its window from global memory, barrier, writes, barrier.
//   ring  (impl 0)  every row of the band, and r halo rows above and below it, has a ring of RING columns in LDS,
//                   slot = column & (RING - 1).  A thread keeps its (2r+1)^2 window in registers and slides it: per
//                   step it reads the entering column j + r of its 2r+1 rows from the rings, writes its output into
//                   its own ring (and to global memory), and pushes the unfiltered value of column j + 1 + AHEAD of
//                   its own row from a register run that 16-byte loads refill every fourth step, two refills ahead
//                   (rows are only 4-byte aligned: the compiler splits such a load into 4 + 12 bytes).
//                   Halo threads only push (what they load is final above the band and untouched below it).
//                   AHEAD = r^2 + 2r is what row i - r needs of row i (column j_i + r (r + 1) + r).  In one step the
//                   columns of a row that anybody reads span [j - r^2, j + AHEAD], the columns written are j and
//                   j + 1 + AHEAD: 2 r^2 + 2r + 2 <= RING distinct slots, none both read and written, so one
//                   barrier per step orders everything.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace medsched {

#define MED_HD __host__ __device__ __forceinline__

constexpr int PLAIN_BAND = 1024;                       // rows per band of the plain formulation = its workgroup size

MED_HD int radius(int wnd_size) { return wnd_size / 2; }                              // :317
MED_HD int ahead(int r) { return r * r + 2 * r; }
MED_HD int ring_size(int r) { return r <= 1 ? 8 : (r == 2 ? 16 : 32); }               // >= 2 r^2 + 2r + 2
MED_HD int ring_threads(int r) { return r >= 3 ? 512 : 1024; }                        // RING * threads * 4 B <= 64 KiB
// rows per band: the plain form has a thread per row, the ring form spends 2r threads on the halo rows
MED_HD int band_cap(int impl, int r) { return impl == 1 ? PLAIN_BAND : ring_threads(r) - 2 * r; }
MED_HD int band_count(int band, int H) { return (H + band - 1) / band; }
MED_HD int band_rows(int band, int H, int k) { return H - k * band < band ? H - k * band : band; }
// step -> column of local row li (the row is idle in that step unless 0 <= column < W)
MED_HD int col_at(int s, int li, int r) { return s - li * (r + 1); }
MED_HD int plain_steps(int rows, int W, int r) { return (rows - 1) * (r + 1) + W; }
// ring form: the top halo row -r pushes column 0 in step first_step; steps come in groups of four (one refill each)
MED_HD int first_step(int r) { return -(r * (r + 1) + ahead(r) + 1); }
MED_HD int ring_steps(int rows, int W, int r) { return ((rows - 1) * (r + 1) + W - first_step(r) + 3) / 4 * 4; }
MED_HD bool refill_point(int t) { return t > 0 && (t & 3) == 0; }
// a neighbour row outside the band is fed from global memory (by its halo thread), one inside from its own thread
MED_HD bool from_global(int li, int rows) { return li < 0 || li >= rows; }

MED_HD float pos_inf() { return __builtin_huge_valf(); }

// element [n / 2] of the ascending order of the n valid entries (:339-341).  No NaN, no -0.0 (smt.h).
template <int K>
MED_HD float median_insert(const float (&x)[K], const bool (&ok)[K])
{
    float v[K];
    int n = 0;
    for (int q = 0; q < K; q++)
        if (ok[q]) {
            int k = n++;
            while (k > 0 && v[k - 1] > x[q]) { v[k] = v[k - 1]; k--; }
            v[k] = x[q];
        }
    return v[n / 2];
}

// 3 x 3: entries outside the image become +inf, which sorts behind (or ties bit for bit with) every valid entry, so
// element [n / 2] of the nine is element [n / 2] of the n; a fixed compare-exchange network keeps it all in registers
MED_HD float median9(const float (&x)[9], const bool (&ok)[9])
{
    float a[9];
    int n = 0;
#pragma unroll
    for (int q = 0; q < 9; q++) { a[q] = ok[q] ? x[q] : pos_inf(); n += ok[q] ? 1 : 0; }
#pragma unroll
    for (int i = 1; i < 9; i++)
#pragma unroll
        for (int k = i; k >= 1; k--) {
            const float lo = a[k - 1], hi = a[k];
            const bool sw = hi < lo;
            a[k - 1] = sw ? hi : lo;
            a[k] = sw ? lo : hi;
        }
    const int m = n / 2;                              // n in {1, 2, 3, 4, 6, 9}
    return m == 0 ? a[0] : (m == 1 ? a[1] : (m == 2 ? a[2] : (m == 3 ? a[3] : a[4])));
}

// ---- plain formulation: the window of (i, j) straight from the map -------------------------------------------------
MED_HD float plain_median(const float *m, int W, int H, int i, int j, int r)
{
    float v[49];
    int n = 0;
    for (int a = -r; a <= r; a++)
        for (int c = -r; c <= r; c++) {
            const int row = i + a, col = j + c;
            if (row >= 0 && row < H && col >= 0 && col < W) {
                const float x = m[(size_t)row * W + col];
                int k = n++;
                while (k > 0 && v[k - 1] > x) { v[k] = v[k - 1]; k--; }
                v[k] = x;
            }
        }
    return v[n / 2];
}

// ---- ring formulation: one thread's state and its step --------------------------------------------------------------
struct f32x4_u { float v[4]; } __attribute__((packed, aligned(4)));                   // 16-byte load, 4-byte aligned

template <int R>
struct RingThread {
    int li, gi;                 // local row (-R .. rows + R - 1) and map row
    bool live, real;            // has a ring row / filters a row
    bool rowok[2 * R + 1];      // map row gi + a - R exists
    float win[2 * R + 1][2 * R + 1];
    float cur[4], nxt[4], nx2[4];
};

// columns c .. c + 3 of map row gi (zeros outside the map: never pushed)
MED_HD void load4(const float *m, int W, int gi, bool rowok, int c, float (&out)[4])
{
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (!rowok || c + 3 < 0 || c >= W) return;
    const float *p = m + (size_t)gi * W;
    if (c >= 0 && c + 3 < W) {
        f32x4_u t;
#ifdef __HIP_DEVICE_COMPILE__
        t = *reinterpret_cast<const f32x4_u *>(p + c);
#else
        memcpy(&t, p + c, 16);
#endif
        out[0] = t.v[0]; out[1] = t.v[1]; out[2] = t.v[2]; out[3] = t.v[3];
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (c + q >= 0 && c + q < W) out[q] = p[c + q];
    }
}

template <int R>
MED_HD int push_col(int s, int li) { return col_at(s, li, R) + 1 + ahead(R); }

// thread `tid` of a band of `rows` rows starting at map row i0; loads the first three groups of its run
template <int R>
MED_HD void ring_begin(RingThread<R> &T, const float *m, int W, int H, int tid, int i0, int rows)
{
    T.li = tid - R;
    T.gi = i0 + T.li;
    T.live = tid < rows + 2 * R;
    T.real = T.live && !from_global(T.li, rows);
#pragma unroll
    for (int a = 0; a <= 2 * R; a++) {
        T.rowok[a] = T.gi + a - R >= 0 && T.gi + a - R < H;
#pragma unroll
        for (int c = 0; c <= 2 * R; c++) T.win[a][c] = 0.0f;
    }
    const bool ok = T.live && T.rowok[R];
    const int p = push_col<R>(first_step(R), T.li);
    load4(m, W, T.gi, ok, p, T.cur);
    load4(m, W, T.gi, ok, p + 4, T.nxt);
    load4(m, W, T.gi, ok, p + 8, T.nx2);
}

// at a refill point (step s): the run moves on by four columns, the load for two groups ahead is issued
template <int R>
MED_HD void ring_refill(RingThread<R> &T, const float *m, int W, int s)
{
#pragma unroll
    for (int q = 0; q < 4; q++) { T.cur[q] = T.nxt[q]; T.nxt[q] = T.nx2[q]; }
    load4(m, W, T.gi, T.live && T.rowok[R], push_col<R>(s, T.li) + 8, T.nx2);
}

// step s (u = position in its group of four).  ring: RING slots of `nt` floats; this thread's is ring[slot * nt + tid].
// Reads the entering column of the rings of rows tid - R .. tid + R, then writes ring[tid] only.  The caller puts one
// workgroup barrier after it.
template <int R>
MED_HD void ring_step(RingThread<R> &T, float *m, int W, float *ring, int nt, int tid, int s, int u)
{
    constexpr int N = 2 * R + 1, MASK = (R <= 1 ? 8 : (R == 2 ? 16 : 32)) - 1;
    const int j = col_at(s, T.li, R);
    if (T.real) {
        const int e = j + R;                                   // the entering column
#pragma unroll
        for (int a = 0; a < N; a++) {
#pragma unroll
            for (int c = 0; c < N - 1; c++) T.win[a][c] = T.win[a][c + 1];
            if (e >= 0 && e < W && T.rowok[a]) T.win[a][N - 1] = ring[(e & MASK) * nt + tid + a - R];
        }
        if (j >= 0 && j < W) {
            float x[N * N];
            bool ok[N * N];
#pragma unroll
            for (int a = 0; a < N; a++)
#pragma unroll
                for (int c = 0; c < N; c++) {
                    x[a * N + c] = T.win[a][c];
                    ok[a * N + c] = T.rowok[a] && j + c - R >= 0 && j + c - R < W;
                }
            float o;
            if constexpr (R == 1) o = median9(x, ok);
            else o = median_insert<N * N>(x, ok);
            T.win[R][R] = o;
            ring[(j & MASK) * nt + tid] = o;
            m[(size_t)T.gi * W + j] = o;
        }
    }
    const int p = j + 1 + ahead(R);
    if (T.live && p >= 0 && p < W) ring[(p & MASK) * nt + tid] = T.cur[u];
}

}  // namespace medsched
