// smt_sad_both: both SAD maps (SADmain.cpp:66-67) from ONE evaluation of the hypotheses, and smt_sad_flow_*:
// SADmain.cpp:47-48, :66-68 for a batch of gray pairs.
//
// 1. The right view's costs are the left view's.  With w = winsize + 1 and costL[i][x][d] = SAD of the left window at
//    column x against the right window at x - d, GetPointDepthRight's cost at (i, x', d) (Sad.h:173-174) is
//    costL[i][x' + d][d]: sadvalue is an exact integer sum of |a - b|.  The right view accepts d iff x' + d <= W - 1
//    (:167); at x = x' + d the left view accepts d iff x - d >= 0 (:125), always.  So the right map is the first minimum
//    over the diagonal, taken here through rank keys (cost << 9) | d: LDS atomic min per workgroup, one agent-scope atomic
//    min per touched right pixel into an [H][W] key map, and a finishing launch (the kernel boundary orders the atomics of
//    every XCD before it).
// 2. costL[i][x][d] is the side x side box sum of AD_d[y][c] = |Lp[y][c] - Rp[y][c - d]|.  k_sad_box keeps, per lane
//    (hypothesis d = lane + 64 k) and per column of its strip, the running box sum C in a register and moves it one image
//    row down by adding the horizontal window sums of the entering row and subtracting those of the leaving row; a
//    horizontal window sum slides along the row (add the entering column's |a - b|, subtract the leaving one's).  The work
//    per hypothesis does not depend on side (the tap loop of k_sad2 needs side^2 / 4 v_sad_u8); all of it is integer, and
//    every sum is below 2^24 for side <= 256, so the float handed to sad_optimal is the number the reference holds.
#include "smt_common.h"
#include "sad_select.h"
#include "box_stage.h"
#include <new>
#include <stdlib.h>
#include <type_traits>
#include <vector>

namespace {

constexpr int BNT = 256;                 // four waves per workgroup
constexpr int BS = 16;                   // columns per wave: C[BS][K] running box sums in VGPRs
constexpr int BSW = BS * (BNT / 64);     // columns per workgroup
constexpr unsigned NOKEY = 0xffffffffu;
constexpr int BOX_MAX_SIDE = 181;        // 255 * side^2 < 2^23: (cost << 9) | d fits 32 bits and never equals NOKEY

// grid (strips of BSW columns, bands of `band` rows).  Step t of a band that starts at row i0 brings in padded row
// i0 + t, takes out padded row i0 + t - side (once there is one) and, from t = side - 1 on, emits output row
// i0 + t - side + 1.  The two rows of step t + 1 are fetched into registers before step t computes and written to the
// other half of the LDS row buffer after it; one barrier per step.  rkeys == nullptr: no right view.
//
// This is the skeleton that box_steps (csrc/box_stage.h) holds for k_ncc_box and k_win_box, written out: row geometry,
// band rule, slot dispatch and host restatement are the shared ones, but staging, row_pass and the step loop stay here.
// Run through box_steps with its emit step and key-row flush as closures, the KT = 2 instantiation took 231 VGPRs for
// 171 and smt_sad_both was 1.7 % to 2.5 % slower at 1920x1080 D = 128, outside the parent's own spread
// (profiles/box_engine_ab.json).  With its own step loop on staging and row_pass factored out of
// box_steps as force-inlined functions taking references, the KT = 8 instantiation keeps C in scratch (560 private bytes
// for 0, one loop left rolled) and KT = 4 takes 394 VGPRs for 275; timed in the same section.  A fix to the skeleton goes
// into both places.
//
// SPX (smt_sad_both_subpixel): the left view's float map subL from the chained row of the emit
// step (sad_wave_subpixel), dispL the optional integer winner.  SPX = false is the integer kernel: subL and min_den are
// dead kernel arguments there.  (As a force-inlined body under two kernels of the old signatures, the KT = 2 integer
// instantiation took 230 VGPRs for 171: the sensitivity described above.)
template <int KT, bool SPX>
__global__ void __launch_bounds__(BNT) k_sad_box(const uint8_t *__restrict__ Lp, const uint8_t *__restrict__ Rp, int H, int W,
                                                 int D, int w, int band, int32_t *__restrict__ dispL,
                                                 float *__restrict__ costL, unsigned *__restrict__ rkeys,
                                                 float *__restrict__ subL, float min_den)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_box[];
    const int side = 2 * w + 1, Wp = W + 2 * w;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * BSW, i0 = blockIdx.y * band;
    const int i1 = i0 + band < H ? i0 + band : H;
    const int nk = (D + 63) >> 6;                              // live hypothesis slots (uniform)
    const int LWE = box_lwe(side, BSW), RWE = box_rwe(side, KT, BSW), ROWE = LWE + RWE;
    const int xLb = x0 - 1, xRb = x0 - 64 * KT;
    constexpr int NKEY = 64 * KT + BSW;
    unsigned *s_rows = s_box;                                  // [2 halves][entering, leaving][LWE left + RWE right entries]
    unsigned *s_keys = s_box + 4 * ROWE;                       // [2 halves][NKEY]
    for (int e = threadIdx.x; e < 2 * NKEY; e += BNT) s_keys[e] = NOKEY;

    // staging: one item = four consecutive entries (two unaligned dword loads, three v_alignbyte, one 16-byte store).
    // Items of a step: entering row left, entering row right, leaving row left, leaving row right; at most 2 per thread.
    const int nL4 = LWE >> 2, nR4 = RWE >> 2, nrow4 = nL4 + nR4;
    unsigned slo[2], shi[2];
    auto fetch = [&](int t) {
        const int rE = i0 + t, rL = rE - side;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * BNT;
            slo[q] = shi[q] = 0;
            if (e < 2 * nrow4) {
                const int which = e >= nrow4, f = e - which * nrow4;
                const int r = which ? rL : rE;
                if (!which || rL >= i0) {
                    const bool right = f >= nL4;
                    const int x = right ? xRb + 4 * (f - nL4) : xLb + 4 * f;
                    box_load8((right ? Rp : Lp) + (size_t)r * Wp, x, Wp, slo[q], shi[q]);
                }
            }
        }
    };
    auto commit = [&](int half) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * BNT;
            if (e < 2 * nrow4)
                *reinterpret_cast<u4v *>(s_rows + (size_t)half * 2 * ROWE + 4 * e) =
                    u4v{slo[q], __builtin_amdgcn_alignbyte(shi[q], slo[q], 1), __builtin_amdgcn_alignbyte(shi[q], slo[q], 2),
                        __builtin_amdgcn_alignbyte(shi[q], slo[q], 3)};
        }
    };
    fetch(0);
    commit(0);
    __syncthreads();

    const int xw = x0 + BS * wv;                               // this wave's first column
    const bool live = xw < W;
    const int nfull = side >> 2, rem = side & 3;
    const unsigned tmask = rem ? (0xffffffffu << (8 * (4 - rem))) : 0u;
    const int la = xw - xLb;                                   // left entry of column xw
    int ra[KT];                                                // right entry of column xw - d
    unsigned C[BS][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        ra[k] = xw - xRb - (lane + 64 * k);
#pragma unroll
        for (int j = 0; j < BS; j++) C[j][k] = 0;
    }
    // horizontal window sums of one staged row over the wave's BS columns, added to (SUB = false) or taken from C
    auto row_pass = [&](const unsigned *Lrow, const unsigned *Rrow, auto sub) {
        constexpr bool SUB = decltype(sub)::value;
        unsigned run[KT];
#pragma unroll
        for (int k = 0; k < KT; k++) run[k] = 0;
        for (int g = 0; g < nfull; g++) {
            const unsigned a4 = Lrow[la + 4 * g];
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = __builtin_amdgcn_sad_u8(a4, Rrow[ra[k] + 4 * g], run[k]);
        }
        if (rem) {
            // the last dword ends at the window's last byte; the bytes already counted are masked out of both operands
            const unsigned a4 = Lrow[la + side - 4] & tmask;
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = __builtin_amdgcn_sad_u8(a4, Rrow[ra[k] + side - 4] & tmask, run[k]);
        }
        const uint8_t *Lb = reinterpret_cast<const uint8_t *>(Lrow), *Rb = reinterpret_cast<const uint8_t *>(Rrow);
#pragma unroll
        for (int j = 0; j < BS; j++) {
            if (j > 0) {
                const unsigned aN = Lb[4 * (la + j - 1 + side)], aO = Lb[4 * (la + j - 1)];
#pragma unroll
                for (int k = 0; k < KT; k++)
                    if (k < nk) {
                        const unsigned bN = Rb[4 * (ra[k] + j - 1 + side)], bO = Rb[4 * (ra[k] + j - 1)];
                        run[k] = __builtin_amdgcn_sad_u8(aN, bN, run[k]) - __builtin_amdgcn_sad_u8(aO, bO, 0u);
                    }
            }
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) C[j][k] = SUB ? C[j][k] - run[k] : C[j][k] + run[k];
        }
    };

    const int nsteps = side - 1 + (i1 - i0);
    for (int t = 0; t < nsteps; t++) {
        const int half = t & 1;
        const int io = i0 + t - side + 1;                      // output row of this step (>= i0: there is one)
        const bool leaving = t >= side;
        if (t + 1 < nsteps) fetch(t + 1);
        unsigned *keys = s_keys + half * NKEY;
        if (live) {
            const unsigned *rows = s_rows + (size_t)half * 2 * ROWE;
            row_pass(rows, rows + LWE, std::false_type());
            if (leaving) row_pass(rows + ROWE, rows + ROWE + LWE, std::true_type());
            if (io >= i0) {
#pragma unroll
                for (int j = 0; j < BS; j++) {
                    const int x = xw + j;
                    if (x >= W) break;
                    unsigned cc[KT];
#pragma unroll
                    for (int k = 0; k < KT; k++) cc[k] = C[j][k];
                    if (x < D - 1) {                           // Sad.h:125-129: d > x repeats the cost at d = x
                        unsigned bc = 0;
#pragma unroll
                        for (int k = 0; k < KT; k++)
                            if (k == (x >> 6)) bc = (unsigned)__builtin_amdgcn_readlane((int)cc[k], x & 63);
#pragma unroll
                        for (int k = 0; k < KT; k++)
                            if (lane + 64 * k > x) cc[k] = bc;
                    }
                    float sad[KT];
#pragma unroll
                    for (int k = 0; k < KT; k++) sad[k] = (k < nk && lane + 64 * k < D) ? (float)cc[k] : 0.0f;   // sadvalue :15-20
                    const int out = sad_optimal<KT>(sad, D, lane);
                    const size_t pix = (size_t)io * W + x;
                    sad_store<SPX>(pix, lane, out, SPX ? sad_wave_subpixel<KT>(sad, out, D, min_den) : 0.0f, dispL, subL);
                    if (costL) {
#pragma unroll
                        for (int k = 0; k < KT; k++)
                            if (k < nk && lane + 64 * k < D) costL[pix * D + lane + 64 * k] = sad[k];
                    }
                    if (rkeys && io < H - 1) {                 // the right view never writes its last row (:157)
#pragma unroll
                        for (int k = 0; k < KT; k++) {
                            const int d = lane + 64 * k;
                            if (k < nk && d < D && d <= x) atomicMin(&keys[x - d - xRb], (cc[k] << 9) | (unsigned)d);
                        }
                    }
                }
            }
        }
        if (t + 1 < nsteps) commit(half ^ 1);
        __syncthreads();
        if (rkeys && io >= i0 && io < H - 1) {
            // this half is offered to again two steps on, after the next barrier
            for (int e = threadIdx.x; e < NKEY; e += BNT) {
                const unsigned v = keys[e];
                if (v != NOKEY) {
                    atomicMin(&rkeys[(size_t)io * W + xRb + e], v);
                    keys[e] = NOKEY;
                }
            }
        }
    }
}

// The right view's sub-pixel map from the finished key map.  The keys hold the winner w = key & 511 and its cost
// cm = key >> 9 only; the neighbours are other pixels' costs, costR(x', w +- 1) = costL(x' + w +- 1, w +- 1), which no
// lane of the box kernel holds when the key is final.  So they are recomputed: the two window sums of the right window at
// x' against the left windows at x' + w - 1 and x' + w + 1, with v_sad_u8 over full dwords plus the masked last dword of
// a row as sad_pixel (csrc/window.hip) takes them (bytes for the 3 x 3 window).  G lanes share a pixel (G a power of two
// from 4 to 64, chosen by the host from the window's dword count; 64 / G pixels per wave), each takes every G-th dword of
// the window, and the sums meet in an xor butterfly inside the group.  2 side^2 byte taps per pixel whatever D is.
// w + 1 > dmax = min(D - 1, W - 1 - x') is the copied tail (Sad.h:167-171): row[w + 1] == row[w] == cm.  A winner at
// either end of the range has no parabola; the last row and column are 0 (:157, :160).
__global__ void __launch_bounds__(256) k_sad_refine_right(const uint8_t *__restrict__ Lp, const uint8_t *__restrict__ Rp,
                                                          const unsigned *__restrict__ rkeys, int H, int W, int D, int w, int G,
                                                          float min_den, float *__restrict__ dispR)
{
    const int side = 2 * w + 1, Wp = W + 2 * w;
    const int ppb = 256 / G, sub = threadIdx.x & (G - 1);
    const size_t p = (size_t)blockIdx.x * ppb + threadIdx.x / G;
    const bool inside = p < (size_t)H * W;
    const int x = inside ? (int)(p % W) : 0, i = inside ? (int)(p / W) : 0;
    const bool real = inside && i < H - 1 && x < W - 1;
    const unsigned key = real ? rkeys[p] : 0u;
    const int wd = (int)(key & 511u);
    const int dmax = D - 1 < W - 1 - x ? D - 1 : W - 1 - x;
    const bool para = real && sad_spx_has_parabola(wd, D);
    const bool two = para && wd + 1 <= dmax;
    unsigned s1 = 0, s2 = 0;
    if (para) {
        const uint8_t *a = Rp + (size_t)i * Wp + x, *b1 = Lp + (size_t)i * Wp + x + wd - 1;
        const uint8_t *b2 = two ? b1 + 2 : b1;                             // never read past the row: w + 1 <= dmax
        if (side >= 4) {
            const int nfull = side >> 2, rem = side & 3, ndw = nfull + (rem ? 1 : 0);
            const unsigned tmask = rem ? (0xffffffffu << (8 * (4 - rem))) : 0u;
            for (int t = sub; t < side * ndw; t += G) {
                const int r = t / ndw, g = t - r * ndw;
                const int c0 = (g < nfull) ? 4 * g : side - 4;
                const unsigned m = (g < nfull) ? 0xffffffffu : tmask;
                const size_t o = (size_t)r * Wp + c0;
                unsigned a4, v1, v2;
                __builtin_memcpy(&a4, a + o, 4);
                __builtin_memcpy(&v1, b1 + o, 4);
                __builtin_memcpy(&v2, b2 + o, 4);
                a4 &= m;
                s1 = __builtin_amdgcn_sad_u8(a4, v1 & m, s1);
                s2 = __builtin_amdgcn_sad_u8(a4, v2 & m, s2);
            }
        } else {
            for (int t = sub; t < side * side; t += G) {
                const int r = t / side, c = t - r * side;
                const size_t o = (size_t)r * Wp + c;
                s1 += (unsigned)abs((int)a[o] - (int)b1[o]);
                s2 += (unsigned)abs((int)a[o] - (int)b2[o]);
            }
        }
    }
    for (int off = G >> 1; off >= 1; off >>= 1) {                          // every lane of the wave takes part
        s1 += (unsigned)__shfl_xor((int)s1, off, 64);
        s2 += (unsigned)__shfl_xor((int)s2, off, 64);
    }
    if (inside && sub == 0) {
        const float cm = (float)(key >> 9);
        dispR[p] = real ? sad_spx_value(wd, D, (float)s1, cm, two ? (float)s2 : cm, min_den) : 0.0f;
    }
}

// key map -> dispR; the last row and column are never written by GetPointDepthRight (Sad.h:157, :160)
__global__ void __launch_bounds__(256) k_sad_rkeys_finish(const unsigned *__restrict__ rkeys, int H, int W, int32_t *__restrict__ dispR)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)H * W) return;
    const int x = (int)(p % W), i = (int)(p / W);
    dispR[p] = (i >= H - 1 || x >= W - 1) ? 0 : (int32_t)(rkeys[p] & 511u);
}

// Volume form of the right view: one wave per right pixel, the first minimum of costL[i][x' + d][d] over
// d <= min(D - 1, W - 1 - x') through the same keys (the volume holds integers below 2^23)
__global__ void __launch_bounds__(256) k_sad_diag(const float *__restrict__ costL, int H, int W, int D, int32_t *__restrict__ dispR)
{
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= (size_t)H * W) return;
    const int x = (int)(p % W), i = (int)(p / W);
    if (i >= H - 1 || x >= W - 1) {
        if (lane == 0) dispR[p] = 0;
        return;
    }
    const int dmax = D - 1 < W - 1 - x ? D - 1 : W - 1 - x;
    unsigned key = NOKEY;
    for (int d = lane; d <= dmax; d += 64) {
        const unsigned k = ((unsigned)costL[(p + d) * D + d] << 9) | (unsigned)d;
        key = k < key ? k : key;
    }
    key = wave_min_u32(key);
    if (lane == 0) dispR[p] = (int32_t)(key & 511u);
}

// k_sad_diag with the parabola: the neighbours of the winner are two more elements of the diagonal, read from the volume
// (the formulation independent of k_sad_refine_right's recomputation).  winR optional.
__global__ void __launch_bounds__(256) k_sad_diag_sub(const float *__restrict__ costL, int H, int W, int D, float min_den,
                                                      float *__restrict__ dispR, int32_t *__restrict__ winR)
{
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= (size_t)H * W) return;
    const int x = (int)(p % W), i = (int)(p / W);
    if (i >= H - 1 || x >= W - 1) {
        sad_store<true>(p, lane, 0, 0.0f, winR, dispR);
        return;
    }
    const int dmax = D - 1 < W - 1 - x ? D - 1 : W - 1 - x;
    unsigned key = NOKEY;
    for (int d = lane; d <= dmax; d += 64) {
        const unsigned k = ((unsigned)costL[(p + d) * D + d] << 9) | (unsigned)d;
        key = k < key ? k : key;
    }
    key = wave_min_u32(key);
    const int wd = (int)(key & 511u);
    const float cm = (float)(key >> 9);
    float f = (float)wd;
    if (sad_spx_has_parabola(wd, D)) {                                     // wave-uniform
        const float c1 = costL[(p + wd - 1) * D + wd - 1];
        const float c2 = wd + 1 <= dmax ? costL[(p + wd + 1) * D + wd + 1] : cm;   // the copied tail (Sad.h:167-171)
        f = spx_refine(wd, D, c1, cm, c2, min_den);
    }
    sad_store<true>(p, lane, wd, f, winR, dispR);
}

// The left view's sad vector, tap by tap, for windows beyond the box kernel: one thread per (pixel, d)
__global__ void __launch_bounds__(256) k_sad_volume(const uint8_t *__restrict__ Lp, const uint8_t *__restrict__ Rp, int H, int W,
                                                    int D, int w, float *__restrict__ costL)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)H * W * D) return;
    const int d = (int)(e % D);
    const size_t p = e / D;
    const int x = (int)(p % W), i = (int)(p / W);
    const int side = 2 * w + 1, Wp = W + 2 * w, dd = d < x ? d : x;
    const uint8_t *a = Lp + (size_t)i * Wp + x, *b = Rp + (size_t)i * Wp + x - dd;
    unsigned acc = 0;
    for (int r = 0; r < side; r++)
        for (int c = 0; c < side; c++) acc += (unsigned)abs((int)a[(size_t)r * Wp + c] - (int)b[(size_t)r * Wp + c]);
    costL[e] = (float)acc;
}

// Rows per band: box_band_rule (csrc/box_stage.h).
int g_sad_both_band = 0;       // test hook: rows per band, 0 = box_band's choice

template <int KT>
int launch_box(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int w, int32_t *dispL, float *costL,
               unsigned *rkeys)
{
    const int side = 2 * w + 1, band = box_band_rule(g_sad_both_band, H, W, side, BSW);
    const size_t shm = ((size_t)4 * (box_lwe(side, BSW) + box_rwe(side, KT, BSW)) + 2 * (64 * KT + BSW)) * 4;   // <= 24 KiB
    const dim3 grid((W + BSW - 1) / BSW, (H + band - 1) / band);
    hipLaunchKernelGGL((k_sad_box<KT, false>), grid, dim3(BNT), shm, st, Lp, Rp, H, W, D, w, band, dispL, costL, rkeys, (float *)nullptr, 0.0f);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

int run_box(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int w, int32_t *dispL, float *costL,
            unsigned *rkeys)
{
    return box_dispatch_kt(D, [&](auto kt) { return launch_box<decltype(kt)::value>(st, Lp, Rp, H, W, D, w, dispL, costL, rkeys); });
}

template <int KT>
int launch_box_sub(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int w, int32_t *winL, float *costL,
                   unsigned *rkeys, float *subL, float min_den)
{
    const int side = 2 * w + 1, band = box_band_rule(g_sad_both_band, H, W, side, BSW);
    const size_t shm = ((size_t)4 * (box_lwe(side, BSW) + box_rwe(side, KT, BSW)) + 2 * (64 * KT + BSW)) * 4;   // as launch_box
    const dim3 grid((W + BSW - 1) / BSW, (H + band - 1) / band);
    hipLaunchKernelGGL((k_sad_box<KT, true>), grid, dim3(BNT), shm, st, Lp, Rp, H, W, D, w, band, winL, costL, rkeys, subL, min_den);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

int run_box_sub(hipStream_t st, const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int w, int32_t *winL, float *costL,
                unsigned *rkeys, float *subL, float min_den)
{
    return box_dispatch_kt(D, [&](auto kt) {
        return launch_box_sub<decltype(kt)::value>(st, Lp, Rp, H, W, D, w, winL, costL, rkeys, subL, min_den);
    });
}

// lanes that share a right pixel in k_sad_refine_right: the power of two from 4 to 64 nearest above the window's dword
// count (9 x 9: 27 dwords, 32 lanes, two pixels per wave; 45 x 45 and beyond: the whole wave)
int refine_group(int side)
{
    const int items = side >= 4 ? side * ((side + 3) >> 2) : side * side;
    int g = 4;
    while (g < 64 && g < items) g <<= 1;
    return g;
}

// Which box form serves smt_sad_both_subpixel by default (dispatch 0, impl 2): true = the left volume in the scratch arena
// and k_sad_diag_sub, false = rank keys and k_sad_refine_right.  The refinement kernel's work grows with side^2, the
// volume's with D.  Measured on one MI355X (tools/sad_subpixel_time.py, profiles/sad_subpixel_time.json, medians; keys +
// refine over volume + diagonal): 0.88 at 450x375 D=60 9x9, 0.67 at 1920x1080 D=128 9x9, 1.38 at 45x45, 3.11 at 450x375
// D=60 181x181.  Per pixel that is about 0.23 + 0.00041 side^2 ns for the refinement against 0.15 + 0.0036 D ns for the
// volume's store and gather; the rule below is where the two lines cross, exact at the four measured points and
// extrapolated everywhere else (D > 128 is not timed).  Volumes beyond 2 GiB stay with the keys.
bool sad_sub_use_volume(int side, int D, size_t N)
{
    return (long long)side * side > 9LL * D - 200 && N * (size_t)D * 4 <= ((size_t)2 << 30);
}

// Which path serves (side, D) by default.  Measured on one MI355X (tools/sad_both_time.py, profiles/sad_both_time.json;
// smt_sad_both with the box kernel over the same-run sum of the two smt_sad calls, medians): 0.53 at 450x375 D=64 5x5
// (the smallest window any driver uses), 0.39 at 450x375 D=60 9x9, 0.037 at 45x45, 0.42 at 1920x1080 D=128 9x9, 0.0075 at
// 45x45.  The box kernel wins at every size measured, so it serves every window it covers.  D > 128 is not timed.
bool sad_both_use_box(int side, int D)
{
    (void)D;
    return side <= BOX_MAX_SIDE;
}

int g_sad_both_impl = 2;       // 2: rank keys (default); 1: left volume + k_sad_diag
int g_sad_both_dispatch = 0;   // 0: sad_both_use_box; 1: the box kernel wherever it covers the window; 2: composed smt_sad calls
int g_sad_both_last = 0;       // what the last call ran: SMT_SAD_FORM_*

}  // namespace

SMT_API int smt_sad_both_set_impl(int impl)
{
    if (impl != 1 && impl != 2) return SMT_ERR_ARG;
    g_sad_both_impl = impl;
    return SMT_OK;
}

SMT_API int smt_sad_both_set_dispatch(int mode)
{
    if (mode < 0 || mode > 2) return SMT_ERR_ARG;
    g_sad_both_dispatch = mode;
    return SMT_OK;
}

SMT_API int smt_sad_both_set_band(int band)
{
    if (band < 0) return SMT_ERR_ARG;
    g_sad_both_band = band;
    return SMT_OK;
}

SMT_API int smt_sad_both_last_form(void) { return g_sad_both_last; }

SMT_API int smt_sad_both(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize, int32_t *dispL, int32_t *dispR,
                         float *costL, void *stream)
{
    if (!Lp || !Rp || !dispL || !dispR || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winsize < 0)
        return SMT_ERR_ARG;
    hipStream_t st = smt_stream(stream);
    const size_t N = (size_t)H * W;
    const int w = winsize + 1;
    const long long side = 2LL * w + 1;
    const bool covered = side <= BOX_MAX_SIDE;
    const bool box = covered && (g_sad_both_dispatch == 1 || (g_sad_both_dispatch == 0 && sad_both_use_box((int)side, D)));
    if (!box) {
        int rc = smt_sad(Lp, Rp, H, W, D, winsize, SMT_VIEW_LEFT, dispL, stream);
        if (rc == SMT_OK) rc = smt_sad(Lp, Rp, H, W, D, winsize, SMT_VIEW_RIGHT, dispR, stream);
        if (rc != SMT_OK) return rc;
        if (costL) {
            hipLaunchKernelGGL(k_sad_volume, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, st, Lp, Rp, H, W, D, w, costL);
            SMT_LAUNCH_CHECK();
        }
        g_sad_both_last = SMT_SAD_FORM_COMPOSED;
        return SMT_OK;
    }
    if (g_sad_both_impl == 2) {
        unsigned *rkeys = nullptr;
        if (smt_scratch_alloc((void **)&rkeys, N * 4, st) != hipSuccess) return SMT_ERR_ALLOC;
        int rc = hipMemsetAsync(rkeys, 0xFF, N * 4, st) == hipSuccess ? SMT_OK : SMT_ERR_HIP;
        if (rc == SMT_OK) rc = run_box(st, Lp, Rp, H, W, D, w, dispL, costL, rkeys);
        if (rc == SMT_OK) hipLaunchKernelGGL(k_sad_rkeys_finish, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rkeys, H, W, dispR);
        smt_scratch_free(rkeys, st);
        if (rc != SMT_OK) return rc;
        SMT_LAUNCH_CHECK();
        g_sad_both_last = SMT_SAD_FORM_BOX_KEYS;
        return SMT_OK;
    }
    float *vol = costL;
    if (!vol && smt_scratch_alloc((void **)&vol, N * D * 4, st) != hipSuccess) return SMT_ERR_ALLOC;
    int rc = run_box(st, Lp, Rp, H, W, D, w, dispL, vol, nullptr);
    if (rc == SMT_OK) hipLaunchKernelGGL(k_sad_diag, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const float *)vol, H, W, D, dispR);
    if (!costL) smt_scratch_free(vol, st);
    if (rc != SMT_OK) return rc;
    SMT_LAUNCH_CHECK();
    g_sad_both_last = SMT_SAD_FORM_BOX_VOLUME;
    return SMT_OK;
}

// smt_sad_both with the parabola kept (include/smt_sad_subpixel.h): the same three forms behind
// the same hooks.  Box + keys: the left view inside k_sad_box_sub, the right view by k_sad_refine_right behind the
// finished keys.  Box + volume: k_sad_diag_sub reads the neighbours from the volume.  Composed: smt_sad_subpixel per view.
SMT_API int smt_sad_both_subpixel(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize,
                                  const smt_subpixel_params *params, float *dispL, float *dispR, int32_t *winL, int32_t *winR,
                                  float *costL, void *stream)
{
    if (!Lp || !Rp || !dispL || !dispR || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winsize < 0)
        return SMT_ERR_ARG;
    const float md = params ? params->min_den : 1.0f;
    if (!spx_min_den_ok(md)) return SMT_ERR_ARG;
    hipStream_t st = smt_stream(stream);
    const size_t N = (size_t)H * W;
    const int w = winsize + 1;
    const long long side = 2LL * w + 1;
    const bool covered = side <= BOX_MAX_SIDE;
    const bool box = covered && (g_sad_both_dispatch == 1 || (g_sad_both_dispatch == 0 && sad_both_use_box((int)side, D)));
    if (!box) {
        int rc = smt_sad_subpixel(Lp, Rp, H, W, D, winsize, SMT_VIEW_LEFT, params, dispL, winL, stream);
        if (rc == SMT_OK) rc = smt_sad_subpixel(Lp, Rp, H, W, D, winsize, SMT_VIEW_RIGHT, params, dispR, winR, stream);
        if (rc != SMT_OK) return rc;
        if (costL) {
            hipLaunchKernelGGL(k_sad_volume, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, st, Lp, Rp, H, W, D, w, costL);
            SMT_LAUNCH_CHECK();
        }
        g_sad_both_last = SMT_SAD_FORM_COMPOSED;
        return SMT_OK;
    }
    // the hooks are obeyed to the letter when the box form is forced (dispatch 1); by default the measured rule chooses
    const bool keys = g_sad_both_impl == 2 && (g_sad_both_dispatch == 1 || !sad_sub_use_volume((int)side, D, N));
    if (keys) {
        unsigned *rkeys = nullptr;
        if (smt_scratch_alloc((void **)&rkeys, N * 4, st) != hipSuccess) return SMT_ERR_ALLOC;
        int rc = hipMemsetAsync(rkeys, 0xFF, N * 4, st) == hipSuccess ? SMT_OK : SMT_ERR_HIP;
        if (rc == SMT_OK) rc = run_box_sub(st, Lp, Rp, H, W, D, w, winL, costL, rkeys, dispL, md);
        if (rc == SMT_OK) {
            if (winR) hipLaunchKernelGGL(k_sad_rkeys_finish, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, rkeys, H, W, winR);
            const int G = refine_group((int)side), ppb = 256 / G;
            hipLaunchKernelGGL(k_sad_refine_right, dim3((unsigned)((N + ppb - 1) / ppb)), dim3(256), 0, st, Lp, Rp, rkeys, H, W, D, w,
                               G, md, dispR);
        }
        smt_scratch_free(rkeys, st);
        if (rc != SMT_OK) return rc;
        SMT_LAUNCH_CHECK();
        g_sad_both_last = SMT_SAD_FORM_BOX_KEYS;
        return SMT_OK;
    }
    float *vol = costL;
    if (!vol && smt_scratch_alloc((void **)&vol, N * D * 4, st) != hipSuccess) return SMT_ERR_ALLOC;
    int rc = run_box_sub(st, Lp, Rp, H, W, D, w, winL, vol, nullptr, dispL, md);
    if (rc == SMT_OK)
        hipLaunchKernelGGL(k_sad_diag_sub, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const float *)vol, H, W, D, md, dispR, winR);
    if (!costL) smt_scratch_free(vol, st);
    if (rc != SMT_OK) return rc;
    SMT_LAUNCH_CHECK();
    g_sad_both_last = SMT_SAD_FORM_BOX_VOLUME;
    return SMT_OK;
}

// ---- host-only checks ----------------------------------------------------------------------------------------------
// host_rng and box_host<Tap>, the restatement of the kernel's recurrence: csrc/box_stage.h

// Host only (no GPU).  On four padded pairs of the given shape -- pseudo-random, constant 0 against constant 255,
// opposed checkerboards, a shifted copy -- the restated recurrence of k_sad_box (box_host<box_tap_sad> and the chain of the
// kernel's emit step, under the band the launch would choose and under a band of 1 and of 3 rows) equals the direct double
// loop over the window for every (i, x, d).
SMT_API int smt_sad_selftest_box(int H, int W, int D, int winsize, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winsize < 0 || 2 * (winsize + 1) + 1 > BOX_MAX_SIDE ||
        (long long)H * W * D > (1 << 24))
        return SMT_ERR_ARG;
    const int w = winsize + 1, side = 2 * w + 1, Hp = H + 2 * w, Wp = W + 2 * w;
    std::vector<uint8_t> L((size_t)Hp * Wp), R((size_t)Hp * Wp);
    std::vector<unsigned> want((size_t)H * W * D), got((size_t)H * W * D);
    host_rng rng(seed);
    for (int pat = 0; pat < 4; pat++) {
        for (int y = 0; y < Hp; y++)
            for (int x = 0; x < Wp; x++) {
                const size_t q = (size_t)y * Wp + x;
                switch (pat) {
                case 0: L[q] = (uint8_t)rng.next(); R[q] = (uint8_t)rng.next(); break;
                case 1: L[q] = 0; R[q] = 255; break;
                case 2: L[q] = ((x ^ y) & 1) ? 255 : 0; R[q] = ((x ^ y) & 1) ? 0 : 255; break;
                default: L[q] = (uint8_t)((x * 37 + y * 11) ^ (x >> 2)); R[q] = (uint8_t)(((x + 3) * 37 + y * 11) ^ ((x + 3) >> 2)); break;
                }
            }
        for (int i = 0; i < H; i++)
            for (int x = 0; x < W; x++)
                for (int d = 0; d < D; d++) {
                    const int dd = d < x ? d : x;                      // Sad.h:125-129
                    unsigned acc = 0;
                    for (int r = 0; r < side; r++)
                        for (int c = 0; c < side; c++)
                            acc += (unsigned)abs((int)L[(size_t)(i + r) * Wp + x + c] - (int)R[(size_t)(i + r) * Wp + x + c - dd]);
                    want[((size_t)i * W + x) * D + d] = acc;
                }
        const int bands[3] = {box_band(H, W, side, BSW), 1, 3};
        for (int b = 0; b < 3; b++) {
            std::fill(got.begin(), got.end(), 0xdeadbeefu);
            box_host<box_tap_sad>(L.data(), R.data(), Wp, H, W, D, side, bands[b], got.data());
            for (size_t p = 0; p < (size_t)H * W; p++)                 // the chain: d > x repeats the sum at d = x
                for (int d = (int)(p % W) + 1; d < D; d++) got[p * D + d] = got[p * D + p % W];
            if (got != want) return SMT_ERR_STATE;
        }
    }
    return SMT_OK;
}

// Host only (no GPU).  Left costs [W][D] with exact ties, all-equal rows and values at the 2^23 bound: the minimum of
// (cost << 9) | d over a right pixel's diagonal is GetMinSadIndex (Sad.h:22-38) of its chained row (:167-171).
SMT_API int smt_sad_selftest_right_keys(int W, int D, int winsize, unsigned seed)
{
    if (W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winsize < 0 || W > (1 << 16)) return SMT_ERR_ARG;
    host_rng rng(seed);
    const long long side = 2LL * (winsize + 1) + 1;
    const unsigned top = (unsigned)(255 * side * side < (1 << 23) - 1 ? 255 * side * side : (1 << 23) - 1);   // largest cost of the window
    std::vector<unsigned> cl((size_t)W * D);
    std::vector<float> row(D);
    const unsigned pal[] = {0u, 0u, 7u, 7u, top, top, top - 1, 1u, 300u, 300u};
    const int mode = (int)(seed % 3);                          // 0: palette (ties), 1: every cost equal, 2: near the bound
    for (auto &c : cl) {
        const uint32_t r = rng.next();
        c = mode == 1 ? top : mode == 2 ? top - (r % 3) : ((r % 5 == 0) ? (r >> 8) % (top + 1) : pal[(r >> 3) % 10]);
    }
    for (int x = 0; x < W; x++) {
        for (int d = 0; d < D; d++) row[d] = (x + d <= W - 1) ? (float)cl[(size_t)(x + d) * D + d] : row[d - 1];
        float mn = row[0];
        int want = 0;
        for (int d = 1; d < D; d++) if (row[d] < mn) { mn = row[d]; want = d; }
        unsigned best = NOKEY;
        for (int d = 0; d < D && x + d <= W - 1; d++) {
            const unsigned key = (cl[(size_t)(x + d) * D + d] << 9) | (unsigned)d;
            if (key == NOKEY) return SMT_ERR_STATE;
            if (key < best) best = key;
        }
        if ((int)(best & 511u) != want) return SMT_ERR_STATE;
    }
    return SMT_OK;
}

// ---- smt_sad_flow_*: the lines of SAD/SADmain.cpp with :67-68 enabled, for a batch of gray pairs -------------------
//   :47-48  copyMakeBorder(img, winsize + 1, BORDER_REPLICATE) of both images      smt_pad_replicate
//   :66-67  GetPointDepthLeft, GetPointDepthRight                                  smt_sad_both (one pass over the hypotheses)
//   :68     CrossCheckDiaparity                                                    smt_sad_crosscheck
// The flow stops there: RemoveSpeckles at :69 reads an int Mat through at<float>, and :71-78 are OpenCV calls and the
// scan-order fillers.  The handle owns the padded images and one set of maps, so a warm call allocates nothing beyond
// the scratch arena of smt_sad_both.
struct smt_sad_flow {
    int device;
    int H, W, D;
    smt_sad_params P;
    hipStream_t stream;
    uint8_t *padL, *padR;       // [H + 2 w][W + 2 w]
    int32_t *mapL, *mapR, *last;   // maps of the current pair where the caller passes no buffer
    uint8_t *cls;
    float *subL, *subR;            // float maps of smt_sad_flow_run_batch_subpixel, allocated by its first call
};

SMT_API void smt_sad_default_params(smt_sad_params *p)
{
    if (!p) return;
    p->winsize = 3;                                           // SADmain.cpp:34
}

SMT_API int smt_sad_flow_destroy(smt_sad_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->padL); (void)hipFree(h->padR);
    (void)hipFree(h->mapL); (void)hipFree(h->mapR); (void)hipFree(h->last); (void)hipFree(h->cls);
    (void)hipFree(h->subL); (void)hipFree(h->subR);
    delete h;
    return SMT_OK;
}

SMT_API int smt_sad_flow_create_on(int device, int H, int W, int D, const smt_sad_params *p, smt_sad_flow **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    smt_sad_params P;
    if (p) P = *p; else smt_sad_default_params(&P);
    if (P.winsize < 0) return SMT_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    smt_sad_flow *h = new (std::nothrow) smt_sad_flow();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->P = P;
    const int w = P.winsize + 1;
    const size_t np = ((size_t)H + 2 * (size_t)w) * ((size_t)W + 2 * (size_t)w), N = (size_t)H * W;
    int rc = smt_malloc((void **)&h->padL, np);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->padR, np);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->mapL, N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->mapR, N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->last, N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->cls, N);
    if (rc != SMT_OK) { smt_sad_flow_destroy(h); return rc; }
    *out = h;
    return SMT_OK;
}

SMT_API int smt_sad_flow_set_stream(smt_sad_flow *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_sad_flow_run_batch(smt_sad_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *dispL,
                                   int32_t *dispR, int32_t *lastdisp, uint8_t *cls)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, w = h->P.winsize + 1;
    const size_t N = (size_t)H * W;
    void *st = (void *)h->stream;
    for (int b = 0; b < pairs; b++) {
        int32_t *dl = dispL ? dispL + b * N : h->mapL, *dr = dispR ? dispR + b * N : h->mapR;
        int rc = smt_pad_replicate(grayL + b * N, H, W, w, h->padL, st);                              // SADmain.cpp:47
        if (rc == SMT_OK) rc = smt_pad_replicate(grayR + b * N, H, W, w, h->padR, st);                // :48
        if (rc == SMT_OK) rc = smt_sad_both(h->padL, h->padR, H, W, h->D, h->P.winsize, dl, dr, nullptr, st);   // :66-67
        if (rc == SMT_OK && (lastdisp || cls))
            rc = smt_sad_crosscheck(dl, dr, H, W, lastdisp ? lastdisp + b * N : h->last, cls ? cls + b * N : h->cls, st);   // :68
        if (rc != SMT_OK) return rc;
    }
    return SMT_OK;
}

// lastdisp of the sub-pixel flow: CrossCheckDiaparity's decision (cls, made on the integer winners) applied to the float
// map -- dispL where accepted, Invalid_Float (Sad.h:13) where rejected
namespace {
__global__ void __launch_bounds__(256) k_sad_last_sub(const uint8_t *__restrict__ cls, const float *__restrict__ subL, int n,
                                                      float *__restrict__ last)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) last[p] = cls[p] ? INFINITY : subL[p];
}
}  // namespace

SMT_API int smt_sad_flow_run_batch_subpixel(smt_sad_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                            const smt_subpixel_params *params, float *dispL, float *dispR, float *lastdisp,
                                            uint8_t *cls)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (params && !spx_min_den_ok(params->min_den)) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, w = h->P.winsize + 1;
    const size_t N = (size_t)H * W;
    if (!h->subL) {                                            // the first sub-pixel call of the handle
        int rc = smt_malloc((void **)&h->subL, N * 4);
        if (rc == SMT_OK) rc = smt_malloc((void **)&h->subR, N * 4);
        if (rc != SMT_OK) {
            (void)hipFree(h->subL); (void)hipFree(h->subR);
            h->subL = h->subR = nullptr;
            return rc;
        }
    }
    void *st = (void *)h->stream;
    const bool check = lastdisp || cls;
    for (int b = 0; b < pairs; b++) {
        float *dl = dispL ? dispL + b * N : h->subL, *dr = dispR ? dispR + b * N : h->subR;
        uint8_t *c = cls ? cls + b * N : h->cls;
        int rc = smt_pad_replicate(grayL + b * N, H, W, w, h->padL, st);                              // SADmain.cpp:47
        if (rc == SMT_OK) rc = smt_pad_replicate(grayR + b * N, H, W, w, h->padR, st);                // :48
        if (rc == SMT_OK)
            rc = smt_sad_both_subpixel(h->padL, h->padR, H, W, h->D, h->P.winsize, params, dl, dr, check ? h->mapL : nullptr,
                                       check ? h->mapR : nullptr, nullptr, st);                       // :66-67
        if (rc == SMT_OK && check) rc = smt_sad_crosscheck(h->mapL, h->mapR, H, W, h->last, c, st);   // :68, on the winners
        if (rc != SMT_OK) return rc;
        if (lastdisp) {
            hipLaunchKernelGGL(k_sad_last_sub, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (const uint8_t *)c,
                               (const float *)dl, (int)N, lastdisp + b * N);
            SMT_LAUNCH_CHECK();
        }
    }
    return SMT_OK;
}
