// What the two integer-sum NCC kernels share -- k_ncc2 (csrc/window.hip, the cross term by v_dot4) and k_ncc_box
// (csrc/ncc_box.hip, the cross term as a running box sum): the window statistics pass, the cost expression and the pieces of
// the parallel WinTakeAll.  Both kernels hand the same integers to the same float64 expression, so their costs are equal
// bit for bit wherever both exist.
#pragma once
#include "smt_common.h"
#include "ncc_keys.h"

namespace {

constexpr int NCT = 16;                                   // rows per k_ncc_stats tile
constexpr int NCC_INT_MAX_SIDE = 181;                     // 255^2 side^2 < 2^31: Sab, Saa and the int sums below are exact

// Window sums per interior pixel, separable, once per image.  grid (tiles of 64 columns, tiles of NCT rows, 2 * pairs):
// blockIdx.z & 1 picks the image, blockIdx.z >> 1 the pair ([pairs][H][W] images and tables; pairs = 1 in smt_ncc).
__global__ void __launch_bounds__(256) k_ncc_stats(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int H, int W,
                                                   int win, int *__restrict__ sumL, double *__restrict__ rootL,
                                                   int *__restrict__ sumR, double *__restrict__ rootR)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int side = 2 * win + 1, RC = 64 + 2 * win, RR = NCT + 2 * win;
    uint8_t *raw = smem;                                  // [RR][RC]
    int *hs = (int *)(smem + (((size_t)RR * RC + 15) & ~(size_t)15));   // [RR][64] row-window sums
    int *hq = hs + RR * 64;                               // [RR][64] row-window sums of squares
    const size_t po = (size_t)(blockIdx.z >> 1) * H * W;
    const uint8_t *img = ((blockIdx.z & 1) == 0 ? L : R) + po;
    int *osum = ((blockIdx.z & 1) == 0 ? sumL : sumR) + po;
    double *oroot = ((blockIdx.z & 1) == 0 ? rootL : rootR) + po;
    const int y0 = win + blockIdx.y * NCT, x0 = win + blockIdx.x * 64;   // first output of the tile
    for (int e = threadIdx.x; e < RR * RC; e += 256) {
        const int r = e / RC, c = e - r * RC;
        const int yy = min(y0 - win + r, H - 1), xx = min(x0 - win + c, W - 1);   // >= 0 by construction
        raw[e] = img[(size_t)yy * W + xx];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < RR * 64; e += 256) {
        const int r = e >> 6, x = e & 63;
        int s1 = 0, s2 = 0;
        for (int c = 0; c < side; c++) { const int v = raw[r * RC + x + c]; s1 += v; s2 += v * v; }
        hs[e] = s1; hq[e] = s2;
    }
    __syncthreads();
    const double n = (double)(side * side);
    for (int e = threadIdx.x; e < NCT * 64; e += 256) {
        const int y = e >> 6, x = e & 63;
        if (y0 + y >= H - win || x0 + x >= W - win) continue;
        int s1 = 0, s2 = 0;
        for (int r = 0; r < side; r++) { s1 += hs[(y + r) * 64 + x]; s2 += hq[(y + r) * 64 + x]; }
        const size_t p = (size_t)(y0 + y) * W + x0 + x;
        osum[p] = s1;
        oroot[p] = sqrt(n * (double)s2 - (double)s1 * (double)s1);   // both products < 2^53: exact, and so is the difference
    }
}

inline size_t ncc_stats_lds(int win)
{
    const int RR = NCT + 2 * win, RC = 64 + 2 * win;
    return (((size_t)RR * RC + 15) & ~(size_t)15) + (size_t)RR * 64 * 8;
}

// Up to 31 x 31 the tile fits the default 64 KiB of dynamic LDS and the launch is what it always was.  Larger windows
// (148 KiB at 181 x 181, of the 160 KiB a gfx950 workgroup may hold) need the kernel's dynamic-LDS attribute raised: done
// once per device (and per translation unit that includes this header: each holds its own copy of the kernel), to the
// size of the largest window, so that a warm call makes no runtime call besides its launches.  false: the attribute
// cannot be had and the caller takes the loop nest, as it does when the scratch cannot be had.
inline bool ncc_stats_ready(int win)
{
    if (ncc_stats_lds(win) <= 64 * 1024) return true;
    static std::mutex mu;
    static signed char state[64] = {};                     // per device: 0 not tried, 1 raised, -1 refused
    const int dev = smt_current_device();
    if (dev < 0 || dev >= 64) return false;
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] == 0) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_ncc_stats, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)ncc_stats_lds((NCC_INT_MAX_SIDE - 1) / 2));
        if (e != hipSuccess) (void)hipGetLastError();
        state[dev] = e == hipSuccess ? 1 : -1;
    }
    return state[dev] == 1;
}

// One launch for `pairs` pairs; the interior must not be empty, side <= 181 and ncc_stats_ready(win) true.
inline int ncc_stats_launch(hipStream_t st, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int win, int *sumL,
                            double *rootL, int *sumR, double *rootR)
{
    const int Hi = H - 2 * win, Wi = W - 2 * win;
    hipLaunchKernelGGL(k_ncc_stats, dim3((Wi + 63) / 64, (Hi + NCT - 1) / NCT, 2 * pairs), dim3(256), ncc_stats_lds(win), st,
                       L, R, H, W, win, sumL, rootL, sumR, rootR);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// cost = (n Sab - Sa Sb) / (sqrt(n Saa - Sa^2) sqrt(n Sbb - Sb^2)) from the exact integers (NCC.h:15-49 with the 1/n
// cancelled): both products stay below 2^53, so num is exact whether or not the compiler contracts it
__device__ __forceinline__ double ncc_int_cost(double n, unsigned sab, double sa, double ra, int sb, double rb)
{
    const double num = n * (double)sab - sa * (double)sb;
    return num / (ra * rb);
}

// ---- WinTakeAll (NCC.h:53-67) in parallel.  m before step d equals the maximum of (float)c[e] over e < d, NaN entries
// skipped (a NaN at d = 0 makes every test false); d wins iff (double)m < c[d]; the answer is the last winner.

// what a hypothesis contributes to the running maximum: NaN and idle entries never raise it
__device__ __forceinline__ float ncc_wta_term(double c, bool act) { return (act && c == c) ? (float)c : -INFINITY; }

// inclusive prefix maximum over the lanes of a wave (f32; NaN-free input)
__device__ __forceinline__ float wave_prefix_max_f32(float v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off, WAVE);
        if (lane >= off) v = fmaxf(v, o);
    }
    return v;
}

// key = 1 + the largest winning d of the lane (0: none); poison = the cost at d = 0 is NaN
__device__ __forceinline__ int ncc_wta_last(unsigned key, bool poison)
{
    const unsigned kmax = ~wave_min_u32(~key);            // the last winner
    return (poison || kmax == 0u) ? 0 : (int)(kmax - 1u);
}

}  // namespace
