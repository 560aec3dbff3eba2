// ComputeDispLeft / ComputeDispRight / ComputeDispV4 (CBLSM/CBLSM.h:451-489, :409-447, :494-532): the window cost
// volumes [H][W][D] that CBLSM.cpp:132 hands to the cross-based aggregation.  Rules: csrc/cblsm_window_rules.h.
//
// Two formulations of the gray forms:
//   1  k_win_tap   one thread per (pixel, d), the side x side tap loop (cwrule::entry); also the only form of V4;
//   2  k_win_box   the box recurrence of csrc/box_stage.h (box_steps, the engine k_ncc_box runs too) with the view as a
//                  template parameter: lanes along d (d = lane + 64 k), 8 or 4 columns per wave, the rows of both images
//                  staged in LDS, a running horizontal window sum per row and a running box sum per column in
//                  registers, so the work per hypothesis does not grow with side.  The `cost = last` chains are applied
//                  at the store: LEFT broadcasts lane x, RIGHT the lane W - 1 - w - x; the row-constant value of RIGHT's
//                  last w columns is a running box sum of its own, kept by the waves that own such columns.
// The kernel writes 4 bytes per hypothesis and reads two image rows per step, so its ceiling is the store rate; the
// volume is produced in one pass (chaining a SAD cost volume afterwards would read and write [H][W][D] once more).
#include "smt_common.h"
#include "box_stage.h"
#include "cblsm_window_rules.h"
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

namespace {

constexpr int BNT = 256;                 // four waves per workgroup
// Columns per wave: C[BS][KT] running box sums in VGPRs.  The kernel runs at the rate its occupancy allows (measured on an
// MI355X, DESIGN.md 5.13: 1920x1080 D=192 takes 1.67 ms with 16 columns per wave and one wave per SIMD, 0.55 ms with 4
// columns and four), so the column count follows the slot count: 8 columns at KT = 1, 4 beyond, and the register
// budget of two workgroups per CU at the least.
template <int KT> constexpr int win_bs() { return KT == 1 ? 8 : 4; }
template <int KT> constexpr int win_bsw() { return win_bs<KT>() * (BNT / 64); }   // columns per workgroup

// The kernel's quotient: a / n for a = (float)S, 0 <= S < 2^24, and fn = (float)n, 9 <= n <= 32761, rn = v_rcp_f32(fn).
// smt_common.h's wave_quotient argument without its range ballot: a is an integer below 2^24 and fn an integer below
// 2^16, so every value is 0 or in [1, 2^24) and the three-instruction sequence rounds as the division does; S = 0 gives
// q0 = 0, rem = 0, q = +0.  smt_cblsm_window_quotient sweeps this function over every S (tests/test_cblsm_window_gpu.py).
__device__ __forceinline__ float win_quot(float a, float fn, float rn)
{
    const float q0 = a * rn;
    const float rem = __builtin_fmaf(-q0, fn, a);
    return __builtin_fmaf(rem, rn, q0);
}

template <bool NT>
__device__ __forceinline__ void win_store(float *p, float v)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// grid (strips of BSW columns, bands of `band` rows, pairs).  The staged rows, the running sums and the step loop of a band
// are box_steps (csrc/box_stage.h) with the v_sad_u8 tap.  "own" is the image whose window stays at the pixel's column
// (LEFT: the left image, RIGHT: the right image), "oth" the one indexed by d (LEFT: the right image at x - d, RIGHT: the
// left image at x + d).  Own entries start at column x0 - 1; oth entries at x0 - 64 KT (LEFT) or x0 - 1 (RIGHT).  What is
// here is RIGHT's edge sum and the emit step: the chain, the quotient, the store.  VIEW 0: ComputeDispLeft, 1:
// ComputeDispRight.
template <int KT, int VIEW, bool NT>
__global__ void __launch_bounds__(BNT, 2) k_win_box(const uint8_t *__restrict__ Lp0, const uint8_t *__restrict__ Rp0, size_t img_stride,
                                                 int H, int W, int D, int w, int band, float *__restrict__ vol0, size_t vol_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_box[];
    constexpr int BS = win_bs<KT>(), BSW = win_bsw<KT>();
    const int side = 2 * w + 1, Wp = W + 2 * w;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * BSW, i0 = blockIdx.y * band;
    const int i1 = i0 + band < H ? i0 + band : H;
    const uint8_t *Lp = Lp0 + (size_t)blockIdx.z * img_stride, *Rp = Rp0 + (size_t)blockIdx.z * img_stride;
    const uint8_t *own = VIEW == 0 ? Lp : Rp, *oth = VIEW == 0 ? Rp : Lp;
    float *vol = vol0 + (size_t)blockIdx.z * vol_stride;
    const int nk = (D + 63) >> 6;                              // live hypothesis slots (uniform)
    const int xw = x0 + BS * wv;                               // this wave's first column

    // RIGHT's last w columns hold hypothesis 0 of column xe = W - 1 - w (cwrule::right_src): a wave that owns such a
    // column keeps that box sum E too, one horizontal window sum of the entering and of the leaving row per step, the
    // side taps spread over the lanes and read from global memory (two rows the workgroup has just staged: cache hits).
    const int xe = W - 1 - w;
    const bool edge = VIEW == 1 && xw < W && xw + BS - 1 > xe;
    unsigned E = 0;
    auto edge_row = [&](int r) __attribute__((always_inline)) {
        const int lane = threadIdx.x & 63;                     // not captured: see box_steps
        const uint8_t *a = Lp + (size_t)r * Wp + xe, *b = Rp + (size_t)r * Wp + xe;
        unsigned s = 0;
        for (int c = lane; c < side; c += 64) s += cwrule::absdiff_u8(a[c], b[c]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += (unsigned)__shfl_xor((int)s, off, WAVE);
        return s;
    };
    auto edge_step = [&](int t, bool leaving) __attribute__((always_inline)) {
        if (edge) {
            E += edge_row(i0 + t);
            if (leaving) E -= edge_row(i0 + t - side);
        }
    };

    const float fn = (float)(side * side), rn = __builtin_amdgcn_rcpf(fn);
    auto emit = [&](int, int io, int x, const unsigned (&Cj)[KT]) __attribute__((always_inline)) {
        const int lane = threadIdx.x & 63;                     // not captured: see box_steps
        unsigned cc[KT];
#pragma unroll
        for (int k = 0; k < KT; k++) cc[k] = Cj[k];
        // the chain: entries past `lim` repeat the entry at lim (LEFT: lim = x, RIGHT: lim = xe - x)
        const int lim = VIEW == 0 ? x : xe - x;
        if (lim < 0) {
#pragma unroll
            for (int k = 0; k < KT; k++) cc[k] = E;
        } else if (lim < D - 1) {
            unsigned bc = 0;
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k == (lim >> 6)) bc = (unsigned)__builtin_amdgcn_readlane((int)cc[k], lim & 63);
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (lane + 64 * k > lim) cc[k] = bc;
        }
        float *dst = vol + ((size_t)io * W + x) * D;
#pragma unroll
        for (int k = 0; k < KT; k++)
            if (k < nk && lane + 64 * k < D) win_store<NT>(dst + lane + 64 * k, win_quot((float)cc[k], fn, rn));
    };
    const int xAb = x0 - box_tap_sad::LEAD, xBb = VIEW == 0 ? x0 - 64 * KT : xAb;
    box_steps<KT, BS, BNT, box_tap_sad, VIEW == 0 ? -1 : 1>(s_box, own, oth, Wp, xAb, xBb, x0, i0, i1, W, side, nk, box_no_hook(),
                                                            edge_step, emit);
}

// The direct formulation: one thread per (pixel, d), the rules of cblsm_window_rules.h and nothing else
template <int FORM>
__global__ void __launch_bounds__(256) k_win_tap(const uint8_t *__restrict__ Lp, const uint8_t *__restrict__ Rp, size_t img_stride,
                                                 int H, int W, int D, int w, float *__restrict__ vol, size_t vol_stride)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)H * W * D) return;
    const int d = (int)(e % D);
    const size_t p = e / D;
    const int x = (int)(p % W), y = (int)(p / W);
    const size_t off = (size_t)blockIdx.z * img_stride;
    vol[(size_t)blockIdx.z * vol_stride + e] = cwrule::entry(FORM, Lp + off, Rp + off, W, w, y, x, d);
}

__global__ void __launch_bounds__(256) k_win_quot(const uint32_t *__restrict__ S, size_t count, int n, float *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float fn = (float)n;
    out[e] = win_quot((float)S[e], fn, __builtin_amdgcn_rcpf(fn));
}

int g_win_impl = 0;     // 0: the dispatch rule, 1: tap loop, 2: box kernel
int g_win_band = 0;     // test hook: rows per band of the box kernel, 0 = box_band's choice
int g_win_store = 0;    // 0: the default store (win_default_nt), 1: plain stores, 2: non-temporal stores
int g_win_last = 0;     // what the last call ran: 1 tap loop, 2 box kernel

// Which formulation serves (side, D) by default.  Measured on one MI355X (tools/cblsm_window_time.py,
// profiles/cblsm_window_time.json; box over tap loop, medians of 21 interleaved samples, left / right view): 0.31 / 0.35 at
// 450x375 D=60 5x5, 0.20 / 0.21 at 1242x375 D=128 5x5, 0.16 / 0.18 at 1920x1080 D=192 5x5, 0.038 / 0.046 at 11x11.  The
// box form wins at every (side, D) measured -- sides 5 and 11, D = 60, 128, 192 -- and its work does not grow with side
// while the tap loop's grows with side^2, so larger sides are a safe extrapolation; side 3 and D > 192 are extrapolated
// too (untimed).
bool win_use_box(int side, int D)
{
    (void)D;
    return side <= cwrule::MAX_SIDE;
}
// Plain against non-temporal stores, measured in the same runs: non-temporal is 1 % to 4 % faster at every size and view
// (0.5515 against 0.5735 ms at 1920x1080 D=192 5x5 left), never slower; the volume is written once and read by a later
// launch from HBM either way.
bool win_default_nt(void) { return true; }

template <int KT, int VIEW>
int launch_box(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t is, int H, int W, int D, int w, float *vol,
               size_t vs)
{
    constexpr int BSW = win_bsw<KT>();
    const int side = 2 * w + 1;
    int band = box_band_rule(g_win_band, H, W, side, BSW);
    if ((H + band - 1) / band > 65535) band = (H + 65534) / 65535;
    const size_t shm = (size_t)4 * (box_lwe(side, BSW) + box_rwe(side, KT, BSW)) * 4;   // <= 16 KiB
    const dim3 grid((W + BSW - 1) / BSW, (H + band - 1) / band, pairs);
    const bool nt = g_win_store == 0 ? win_default_nt() : g_win_store == 2;
    if (nt) hipLaunchKernelGGL((k_win_box<KT, VIEW, true>), grid, dim3(BNT), shm, st, Lp, Rp, is, H, W, D, w, band, vol, vs);
    else hipLaunchKernelGGL((k_win_box<KT, VIEW, false>), grid, dim3(BNT), shm, st, Lp, Rp, is, H, W, D, w, band, vol, vs);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

template <int VIEW>
int run_box(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t is, int H, int W, int D, int w, float *vol, size_t vs)
{
    return box_dispatch_kt(D, [&](auto kt) { return launch_box<decltype(kt)::value, VIEW>(st, Lp, Rp, pairs, is, H, W, D, w, vol, vs); });
}

// the argument rules shared by the device entry and the host twin; on SMT_OK the dense strides are filled in
int win_check(const void *Lp, const void *Rp, int pairs, size_t &is, int H, int W, int D, int winSize, int form, const void *vol,
              size_t &vs)
{
    if (pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!Lp || !Rp || !vol || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winSize < 0 ||
        2 * (winSize + 1) + 1 > cwrule::MAX_SIDE || pairs > 65535 || (long long)H * W > INT_MAX / 2)
        return SMT_ERR_ARG;
    if (form != SMT_CBLSM_COST_LEFT && form != SMT_CBLSM_COST_RIGHT && form != SMT_CBLSM_COST_V4) return SMT_ERR_ARG;
    const int w = winSize + 1;
    const size_t img = ((size_t)H + 2 * w) * ((size_t)W + 2 * w) * (form == SMT_CBLSM_COST_V4 ? 3 : 1), V = (size_t)H * W * D;
    if ((is && is < img) || (vs && vs < V)) return SMT_ERR_ARG;
    if (!is) is = img;
    if (!vs) vs = V;
    if (form == SMT_CBLSM_COST_RIGHT && !cwrule::right_defined(W, w)) return SMT_ERR_REF_UB;
    return SMT_OK;
}

}  // namespace

SMT_API int smt_cblsm_window_set_impl(int impl)
{
    if (impl < 0 || impl > 2) return SMT_ERR_ARG;
    g_win_impl = impl;
    return SMT_OK;
}

SMT_API int smt_cblsm_window_set_band(int band)
{
    if (band < 0) return SMT_ERR_ARG;
    g_win_band = band;
    return SMT_OK;
}

SMT_API int smt_cblsm_window_set_store(int mode)
{
    if (mode < 0 || mode > 2) return SMT_ERR_ARG;
    g_win_store = mode;
    return SMT_OK;
}

SMT_API int smt_cblsm_window_last_form(void) { return g_win_last; }

SMT_API int smt_cblsm_window_cost_batch(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D,
                                        int winSize, int form, float *vol, size_t vol_stride, void *stream)
{
    const int rc = win_check(Lp, Rp, pairs, img_stride, H, W, D, winSize, form, vol, vol_stride);
    if (rc != SMT_OK || pairs == 0) return rc;
    hipStream_t st = smt_stream(stream);
    const int w = winSize + 1, side = 2 * w + 1;
    const bool box = form != SMT_CBLSM_COST_V4 && (g_win_impl == 2 || (g_win_impl == 0 && win_use_box(side, D)));
    if (box) {
        const int r = form == SMT_CBLSM_COST_LEFT ? run_box<0>(st, Lp, Rp, pairs, img_stride, H, W, D, w, vol, vol_stride)
                                                  : run_box<1>(st, Lp, Rp, pairs, img_stride, H, W, D, w, vol, vol_stride);
        if (r != SMT_OK) return r;
        g_win_last = 2;
        return SMT_OK;
    }
    const dim3 grid((unsigned)(((size_t)H * W * D + 255) / 256), 1, pairs);
    if (form == SMT_CBLSM_COST_LEFT)
        hipLaunchKernelGGL(k_win_tap<1>, grid, dim3(256), 0, st, Lp, Rp, img_stride, H, W, D, w, vol, vol_stride);
    else if (form == SMT_CBLSM_COST_RIGHT)
        hipLaunchKernelGGL(k_win_tap<2>, grid, dim3(256), 0, st, Lp, Rp, img_stride, H, W, D, w, vol, vol_stride);
    else
        hipLaunchKernelGGL(k_win_tap<3>, grid, dim3(256), 0, st, Lp, Rp, img_stride, H, W, D, w, vol, vol_stride);
    SMT_LAUNCH_CHECK();
    g_win_last = 1;
    return SMT_OK;
}

SMT_API int smt_cblsm_window_quotient(const uint32_t *S_dev, size_t count, int n, float *out_dev, void *stream)
{
    if (!S_dev || !out_dev || n < 1 || n > cwrule::MAX_SIDE * cwrule::MAX_SIDE || count > ((size_t)1 << 31)) return SMT_ERR_ARG;
    if (count == 0) return SMT_OK;
    hipLaunchKernelGGL(k_win_quot, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, smt_stream(stream), S_dev, count, n, out_dev);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// ---- host only -----------------------------------------------------------------------------------------------------
SMT_API int smt_cblsm_window_cost_host(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D,
                                       int winSize, int form, float *vol, size_t vol_stride)
{
    const int rc = win_check(Lp, Rp, pairs, img_stride, H, W, D, winSize, form, vol, vol_stride);
    if (rc != SMT_OK || pairs == 0) return rc;
    const int w = winSize + 1;
    for (int b = 0; b < pairs; b++) {
        const uint8_t *L = Lp + (size_t)b * img_stride, *R = Rp + (size_t)b * img_stride;
        float *v = vol + (size_t)b * vol_stride;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                // one window sum per hypothesis the pixel really evaluates; the chained entries repeat it
                float *dst = v + ((size_t)y * W + x) * D;
                int pxs = -1, pds = -1;
                float last = 0.0f;
                for (int d = 0; d < D; d++) {
                    int xs = x, ds;
                    if (form == SMT_CBLSM_COST_RIGHT) cwrule::right_src(x, d, W, w, xs, ds);
                    else ds = cwrule::left_src(x, d);
                    if (xs != pxs || ds != pds) { last = cwrule::entry(form, L, R, W, w, y, x, d); pxs = xs; pds = ds; }
                    dst[d] = last;
                }
            }
    }
    return SMT_OK;
}

// Host only (no GPU).  On a pseudo-random padded pair and on an all-0 against an all-255 pair of the given shape:
//  1. the box arithmetic of k_win_box -- per hypothesis a horizontal window sum that slides along the row (add the
//     entering column's |a - b|, take out the leaving one's) and a box sum that moves down a row (add the entering row's
//     window sum, take out the leaving row's), all in uint32 -- equals the direct double loop over the window for every
//     (y, x, d) the view evaluates, and the largest sum stays below 2^24;
//  2. the chain rules (cwrule::left_src / right_src) equal a literal walk of the reference's loops over a flat buffer:
//     a guarded entry copies the element before it, whichever pixel that belongs to.
// V4 (three channels, the channel minimum per tap, the uchar wrap) is checked by 2 alone, against its own literal walk.
SMT_API int smt_cblsm_selftest_window(int H, int W, int D, int winSize, int form, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winSize < 0 || 2 * (winSize + 1) + 1 > cwrule::MAX_SIDE ||
        (form != SMT_CBLSM_COST_LEFT && form != SMT_CBLSM_COST_RIGHT && form != SMT_CBLSM_COST_V4) ||
        (long long)H * W * D > (1 << 22))
        return SMT_ERR_ARG;
    const int w = winSize + 1, side = 2 * w + 1, n = side * side, Hp = H + 2 * w, Wp = W + 2 * w;
    if (form == SMT_CBLSM_COST_RIGHT && !cwrule::right_defined(W, w)) return SMT_ERR_REF_UB;
    const int ch = form == SMT_CBLSM_COST_V4 ? 3 : 1;
    std::vector<uint8_t> L((size_t)Hp * Wp * ch), R((size_t)Hp * Wp * ch);
    std::vector<float> walk((size_t)H * W * D);
    std::vector<uint32_t> hs((size_t)Hp * W);
    host_rng rng(seed);
    for (int pat = 0; pat < 2; pat++) {
        for (size_t q = 0; q < L.size(); q++) {
            L[q] = pat ? 0 : (uint8_t)rng.next();
            R[q] = pat ? 255 : (uint8_t)rng.next();
        }
        // 2. the literal walk: rows, columns, d, a guarded entry copies flat element idx - 1
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int d = 0; d < D; d++) {
                    const size_t idx = ((size_t)y * W + x) * D + d;
                    const int j = x + w;                                           // the reference's padded column
                    const bool guard = form == SMT_CBLSM_COST_RIGHT ? (j + d + w + 1 > Wp - w) : (j - w - d < 0);
                    if (guard) { walk[idx] = walk[idx - 1]; continue; }            // idx >= 1: W > w for RIGHT, d >= 1 else
                    if (form == SMT_CBLSM_COST_V4) {
                        uint8_t sum = 0;
                        for (int r = 0; r < side; r++)
                            for (int c = 0; c < side; c++) {
                                const uint8_t *a = &L[((size_t)(y + r) * Wp + x + c) * 3], *b = &R[((size_t)(y + r) * Wp + x - d + c) * 3];
                                uint8_t m[3];
                                for (int q = 0; q < 3; q++) m[q] = (uint8_t)abs((int)a[q] - (int)b[q]);
                                sum = (uint8_t)(sum + (m[0] > m[1] ? (m[1] > m[2] ? m[2] : m[1]) : (m[0] > m[2] ? m[2] : m[0])));
                            }
                        walk[idx] = (float)(uint8_t)(sum / n);
                    } else {
                        const int xa = form == SMT_CBLSM_COST_RIGHT ? x + d : x, xb = form == SMT_CBLSM_COST_RIGHT ? x : x - d;
                        double s = 0.0;
                        for (int r = 0; r < side; r++)
                            for (int c = 0; c < side; c++)
                                s += (double)abs((int)L[(size_t)(y + r) * Wp + xa + c] - (int)R[(size_t)(y + r) * Wp + xb + c]);
                        walk[idx] = (float)(s * (1.0 / (double)n));                 // cv::mean: a double sum times a reciprocal
                    }
                }
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int d = 0; d < D; d++) {
                    const float got = cwrule::entry(form, L.data(), R.data(), W, w, y, x, d);
                    if (memcmp(&got, &walk[((size_t)y * W + x) * D + d], 4) != 0) return SMT_ERR_STATE;
                }
        if (form == SMT_CBLSM_COST_V4) continue;
        // 1. the recurrence, hypothesis by hypothesis
        for (int d = 0; d < D; d++) {
            // columns the view evaluates at d without a chain: LEFT x >= d, RIGHT x <= W - 1 - w - d (here up to the
            // last column whose window is still inside the padded row, x <= W - 1 - d: the kernel's sums exist there too)
            const int xlo = form == SMT_CBLSM_COST_LEFT ? d : 0, xhi = form == SMT_CBLSM_COST_LEFT ? W - 1 : W - 1 - d;
            if (xlo > xhi) continue;
            const int da = form == SMT_CBLSM_COST_RIGHT ? d : 0, db = form == SMT_CBLSM_COST_RIGHT ? 0 : -d;
            auto ad = [&](int r, int c) { return (uint32_t)abs((int)L[(size_t)r * Wp + c + da] - (int)R[(size_t)r * Wp + c + db]); };
            for (int r = 0; r < Hp; r++) {
                uint32_t run = 0;
                for (int c = 0; c < side; c++) run += ad(r, xlo + c);
                hs[(size_t)r * W + xlo] = run;
                for (int x = xlo + 1; x <= xhi; x++) {
                    run = run + ad(r, x - 1 + side) - ad(r, x - 1);
                    hs[(size_t)r * W + x] = run;
                }
            }
            for (int x = xlo; x <= xhi; x++) {
                uint32_t Cb = 0;
                for (int r = 0; r < side - 1; r++) Cb += hs[(size_t)r * W + x];
                for (int y = 0; y < H; y++) {
                    Cb += hs[(size_t)(y + side - 1) * W + x];
                    if (y > 0) Cb -= hs[(size_t)(y - 1) * W + x];
                    if (Cb >= (1u << 24)) return SMT_ERR_STATE;
                    if (Cb != cwrule::window_sum(L.data(), R.data(), Wp, y, x + da, x + db, side)) return SMT_ERR_STATE;
                    if (pat == 1 && Cb != 255u * (uint32_t)n) return SMT_ERR_STATE;
                }
            }
        }
    }
    return SMT_OK;
}
