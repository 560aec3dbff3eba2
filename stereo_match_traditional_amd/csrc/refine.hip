// AD-Census iterative region voting and outlier interpolation (include/smt_refine.h, csrc/refine_rule.h, DESIGN.md
// section 5.20).  Parity unpinned: no reference code.
//
// A call is one opening launch (k_refine_open: state, the entry count, the arm-range flag and, when the number of passes
// is odd, the copy into the scratch map that makes the last pass land in the caller's map), one launch per voting
// iteration and one for the interpolation.  Every pass reads one map and writes every pixel of the other (Jacobi), so no
// pass needs a copy and nothing waits on the host.  Counts reach `status` by one integer atomic per wave that has
// something to add: integer sums do not depend on their order.
//
// Voting, two formulations with identical bits:
//   direct  one thread per pixel in a grid-stride loop; a thread's D counters lie in arena scratch, bin-major and
//           thread-minor so that a wave's increments of one bin touch one line; the scan that finds the winner clears
//           them for the next outlier.  Obviously the rule; written first.
//   wave    a workgroup of four waves owns 64 pixels of a row; every wave ballots the segment's outliers and takes
//           every fourth of them.  Lanes run along a region row's columns (a row of the default arms, 69 columns, is
//           two steps), the histogram is the wave's own D counters in LDS (LDS atomic add), the winner comes from one
//           wave reduction over count << 9 | (511 - bin): the largest count, then the smallest bin.
// Interpolation: a wave owns 64 pixels of a row, copies the reliable ones and gives 16 lanes, one per ray, to each
// outlier, four outliers at a time; the winner is a 16-lane minimum over refinerule::cand_key and the lowest lane
// among the equal ones.
#include "smt_common.h"
#include "../../include/smt_refine.h"
#include "refine_rule.h"
#include <stdlib.h>
#include <string.h>

namespace rr = refinerule;

namespace {

int g_refine_impl = 0;
int g_refine_last_form = 0;

constexpr int RV_WAVES = 4;                // waves of a k_vote_wave workgroup
constexpr int RV_DIRECT_THREADS = 32768;   // most threads of a k_vote_direct launch: bounds its counters

struct maps_view {                         // one side of a pass: the caller's maps or the scratch maps
    float *p;
    size_t stride;
};

// state, entry count, arm flag, optional copy.  One thread per pixel, pairs on grid.y.
__global__ __launch_bounds__(256) void k_refine_open(const float *maps, size_t mstride, float *copy, int pairs, int N, int D,
                                                     const int *aL, const int *aR, const int *aT, const int *aB,
                                                     size_t astride, uint8_t *state, size_t sstride, int *status)
{
    const int idx = (int)(blockIdx.x * 256u + threadIdx.x);
    for (int p = (int)blockIdx.y; p < pairs; p += (int)gridDim.y) {
        bool out = false, clamp = false;
        if (idx < N) {
            const float v = maps[p * mstride + idx];
            out = !rr::reliable(v, D);
            if (copy) copy[(size_t)p * N + idx] = v;
            if (state) state[p * sstride + idx] = out ? SMT_REFINE_STATE_OUTLIER : 0;
            if (aL) {
                const size_t a = p * astride + idx;
                clamp = rr::arm_out_of_range(aL[a]) || rr::arm_out_of_range(aR[a]) || rr::arm_out_of_range(aT[a]) ||
                        rr::arm_out_of_range(aB[a]);
            }
        }
        if (status) {
            const unsigned long long bo = __ballot(out), bc = __ballot(clamp);
            if ((threadIdx.x & 63) == 0) {
                if (bo) atomicAdd(&status[4 * p], __popcll(bo));
                if (bc) atomicOr(&status[4 * p + 3], SMT_REFINE_ARM_CLAMPED);
            }
        }
    }
}

// One voting iteration, direct form.  hist: gridDim.y * T * D counters, T = gridDim.x * 256 threads per grid row.
__global__ __launch_bounds__(256) void k_vote_direct(maps_view src, maps_view dst, int pairs, int H, int W, int D,
                                                     const int *aL, const int *aR, const int *aT, const int *aB,
                                                     size_t astride, int irv_ts, float irv_th, int iter, uint8_t *state,
                                                     size_t sstride, int *status, unsigned *hist)
{
    const int T = (int)gridDim.x * 256, t = (int)(blockIdx.x * 256u + threadIdx.x), N = H * W;
    unsigned *mine = hist + (size_t)blockIdx.y * T * D + t;              // counter of bin b: mine[b * T]
    for (int b = 0; b < D; b++) mine[(size_t)b * T] = 0;
    for (int p = (int)blockIdx.y; p < pairs; p += (int)gridDim.y) {
        const float *M = src.p + p * src.stride;
        float *Mn = dst.p + p * dst.stride;
        const int *pL = aL + p * astride, *pR = aR + p * astride, *pT = aT + p * astride, *pB = aB + p * astride;
        int fills = 0;
        for (int idx = t; idx < N; idx += T) {
            const float v = M[idx];
            if (rr::reliable(v, D)) { Mn[idx] = v; continue; }
            const int i = idx / W, j = idx - i * W;
            const int r0 = rr::span_lo(i, pT[idx]), r1 = rr::span_hi(i, pB[idx], H);
            int S = 0;
            for (int r = r0; r <= r1; r++) {
                const int q = r * W + j;
                const int c0 = rr::span_lo(j, pL[q]), c1 = rr::span_hi(j, pR[q], W);
                for (int c = c0; c <= c1; c++) {
                    const float x = M[r * W + c];
                    if (rr::reliable(x, D)) { mine[(size_t)rr::bin_of(x, D) * T]++; S++; }
                }
            }
            int h = 0, d = 0;
            for (int b = 0; b < D; b++) {                                 // the smallest bin with the largest count
                const int cnt = (int)mine[(size_t)b * T];
                mine[(size_t)b * T] = 0;
                if (cnt > h) { h = cnt; d = b; }
            }
            const bool fill = rr::vote_fills(S, h, irv_ts, irv_th);
            Mn[idx] = fill ? (float)d : v;
            if (fill) {
                fills++;
                if (state) state[p * sstride + idx] = (uint8_t)iter;
            }
        }
        if (status && fills) atomicAdd(&status[4 * p + 1], fills);
    }
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, off, WAVE));
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// One voting iteration, wave-per-outlier form.  grid.x = segments per row * H, grid.y = pairs (looped).
__global__ __launch_bounds__(RV_WAVES * 64) void k_vote_wave(maps_view src, maps_view dst, int pairs, int H, int W, int D,
                                                             int nseg, const int *aL, const int *aR, const int *aT,
                                                             const int *aB, size_t astride, int irv_ts, float irv_th,
                                                             int iter, uint8_t *state, size_t sstride, int *status)
{
    __shared__ unsigned s_hist[RV_WAVES][SMT_MAX_DISPARITY];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    const int i = (int)(blockIdx.x / (unsigned)nseg), j0 = (int)(blockIdx.x % (unsigned)nseg) * 64;
    const int j = j0 + lane;
    unsigned *hist = s_hist[w];
    for (int p = (int)blockIdx.y; p < pairs; p += (int)gridDim.y) {
        const float *M = src.p + p * src.stride;
        float *Mn = dst.p + p * dst.stride;
        const int *pL = aL + p * astride, *pR = aR + p * astride, *pT = aT + p * astride, *pB = aB + p * astride;
        const bool in = j < W;
        const float v = in ? M[i * W + j] : 0.0f;
        const bool out = in && !rr::reliable(v, D);
        if (w == 0 && in && !out) Mn[i * W + j] = v;                       // outliers are written by the wave that owns them
        int fills = 0, turn = 0;
        for (unsigned long long m = __ballot(out); m; m &= m - 1, turn++) {
            if ((turn & (RV_WAVES - 1)) != w) continue;                    // wave-uniform
            const int l = __builtin_ctzll(m), pj = j0 + l, pidx = i * W + pj;
            const int orig = __builtin_amdgcn_readlane(__float_as_int(v), l);
            for (int b = lane; b < D; b += 64) hist[b] = 0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int r0 = __builtin_amdgcn_readfirstlane(rr::span_lo(i, pT[pidx]));
            const int r1 = __builtin_amdgcn_readfirstlane(rr::span_hi(i, pB[pidx], H));
            int S = 0;
            for (int r = r0; r <= r1; r++) {
                const int q = r * W + pj;
                const int c0 = __builtin_amdgcn_readfirstlane(rr::span_lo(pj, pL[q]));
                const int c1 = __builtin_amdgcn_readfirstlane(rr::span_hi(pj, pR[q], W));
                for (int c = c0 + lane; c <= c1; c += 64) {
                    const float x = M[r * W + c];
                    if (rr::reliable(x, D)) { atomicAdd(&hist[rr::bin_of(x, D)], 1u); S++; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            unsigned key = 0;
            for (int b = lane; b < D; b += 64) key = max(key, hist[b] << 9 | (unsigned)(511 - b));
            key = wave_max_u32(key);
            S = wave_sum_i32(S);
            const int h = (int)(key >> 9), d = 511 - (int)(key & 511u);
            const bool fill = rr::vote_fills(S, h, irv_ts, irv_th);
            if (lane == 0) {
                Mn[pidx] = fill ? (float)d : __int_as_float(orig);
                if (fill && state) state[p * sstride + pidx] = (uint8_t)iter;
            }
            fills += fill;
            __builtin_amdgcn_wave_barrier();                               // the next outlier clears the counters
        }
        if (status && fills && lane == 0) atomicAdd(&status[4 * p + 1], fills);
    }
}

// The interpolation.  grid.x = segments per row * H / 4 waves, grid.y = pairs (looped); a wave per 64-pixel row segment.
__global__ __launch_bounds__(256) void k_interpolate(maps_view src, maps_view dst, int pairs, int H, int W, int D, int nseg,
                                                     const uint8_t *cls, size_t cstride, const uint8_t *gray, size_t gstride,
                                                     int search, uint8_t *state, size_t sstride, int *status)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= (long long)nseg * H) return;                                // whole waves leave: nothing below is a block barrier
    const int i = (int)(seg / nseg), j0 = (int)(seg % nseg) * 64, j = j0 + lane;
    const int grp = lane >> 4, ray = lane & 15;
    for (int p = (int)blockIdx.y; p < pairs; p += (int)gridDim.y) {
        const float *M = src.p + p * src.stride;
        float *Mn = dst.p + p * dst.stride;
        const uint8_t *pc = cls + p * cstride, *pg = gray + p * gstride;
        const bool in = j < W;
        const float v = in ? M[i * W + j] : 0.0f;
        const bool out = in && !rr::reliable(v, D);
        if (in && !out) Mn[i * W + j] = v;
        int fills = 0;
        unsigned long long m = __ballot(out);
        while (m) {
            int l = -1;                                                    // group g takes the g-th of the next four outliers
#pragma unroll
            for (int g = 0; g < 4; g++)
                if (m) {
                    if (g == grp) l = __builtin_ctzll(m);
                    m &= m - 1;
                }
            unsigned key = 0xFFFFFFFFu;
            int bits = 0;
            const int pj = j0 + (l < 0 ? 0 : l), pidx = i * W + pj;
            if (l >= 0) {
                const long long q = rr::ray_candidate(M, H, W, D, i, pj, ray, search);
                if (q >= 0) {
                    bits = __float_as_int(M[q]);
                    key = rr::cand_key(pc[pidx] == 1, (unsigned)bits, pg[pidx], pg[q]);
                }
            }
            const bool has = key != 0xFFFFFFFFu;                           // no candidate's key: a NaN's bits, or above 255
            unsigned best = key;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, off, WAVE));
            const unsigned long long eq = __ballot(has && key == best);
            const unsigned mine = (unsigned)(eq >> (16 * grp)) & 0xFFFFu;  // the group's rays that hold the smallest key
            const int win = mine ? 16 * grp + __builtin_ctz(mine) : lane;
            const int wbits = __shfl(bits, win, WAVE);
            if (l >= 0 && ray == 0) {
                Mn[pidx] = mine ? __int_as_float(wbits) : M[pidx];
                if (mine) {
                    fills++;
                    if (state) state[p * sstride + pidx] = SMT_REFINE_STATE_INTERPOLATED;
                }
            }
        }
        if (status) {
            fills = wave_sum_i32(fills);
            if (fills && lane == 0) atomicAdd(&status[4 * p + 2], fills);
        }
    }
}

struct refine_args {
    float *maps; int pairs; size_t map_stride;
    const int *aL, *aR, *aT, *aB; size_t arm_stride;
    const uint8_t *cls; size_t cls_stride;
    const uint8_t *gray; size_t gray_stride;
    int H, W, D;
    smt_refine_params P;
    uint8_t *state; size_t state_stride;
    int *status;
    bool vote, interp;
};

// arguments -> SMT_ERR_ARG or SMT_OK, strides resolved (0 -> H*W)
int refine_check(refine_args &a, const smt_refine_params *params)
{
    if (params) a.P = *params; else smt_refine_default_params(&a.P);
    if (!a.maps || a.pairs < 0 || a.H <= 0 || a.W <= 0 || a.D < 1 || a.D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    if ((long long)a.H * a.W >= (1ll << 31)) return SMT_ERR_ARG;
    if (a.P.irv_iters < 0 || a.P.irv_iters > 16 || a.P.search < 0) return SMT_ERR_ARG;
    if (a.vote && (!a.aL || !a.aR || !a.aT || !a.aB)) return SMT_ERR_ARG;
    if (a.interp && (!a.cls || !a.gray)) return SMT_ERR_ARG;
    const size_t N = (size_t)a.H * a.W;
    for (size_t *s : {&a.map_stride, &a.arm_stride, &a.cls_stride, &a.gray_stride, &a.state_stride}) {
        if (*s == 0) *s = N;
        if (*s < N) return SMT_ERR_ARG;
    }
    return SMT_OK;
}

int refine_enqueue(const refine_args &a, hipStream_t st)
{
    if (a.pairs == 0) return SMT_OK;
    const int H = a.H, W = a.W, D = a.D, N = H * W, pairs = a.pairs;
    const int iters = a.vote ? a.P.irv_iters : 0, passes = iters + (a.interp ? 1 : 0);
    const int nseg = (W + 63) / 64;
    if ((long long)nseg * H >= (1ll << 31)) return SMT_ERR_ARG;
    const int form = g_refine_impl ? g_refine_impl : SMT_REFINE_FORM_WAVE;  // the default: DESIGN.md section 5.20
    scratch_set ss(st);
    float *scr = nullptr;
    if (passes > 0 && !(scr = (float *)ss.get((size_t)pairs * N * 4))) return SMT_ERR_ALLOC;
    const unsigned gy = (unsigned)(pairs < 128 ? pairs : 128);
    unsigned dgx = (unsigned)((N + 255) / 256);                             // the direct form's grid
    if (dgx > RV_DIRECT_THREADS / 256 / gy) dgx = RV_DIRECT_THREADS / 256 / gy;
    unsigned *hist = nullptr;
    if (iters > 0 && form == SMT_REFINE_FORM_DIRECT &&
        !(hist = (unsigned *)ss.get((size_t)gy * dgx * 256 * D * 4)))
        return SMT_ERR_ALLOC;
    if (a.status) SMT_HIP(hipMemsetAsync(a.status, 0, (size_t)pairs * 16, st));
    const maps_view user{a.maps, a.map_stride}, mine{scr, (size_t)N};
    // an odd number of passes starts from the scratch copy, so that the last pass writes the caller's maps
    maps_view src = (passes & 1) ? mine : user, dst = (passes & 1) ? user : mine;
    hipLaunchKernelGGL(k_refine_open, dim3((unsigned)((N + 255) / 256), gy), dim3(256), 0, st, a.maps, a.map_stride,
                       (passes & 1) ? scr : (float *)nullptr, pairs, N, D, a.vote ? a.aL : nullptr, a.aR, a.aT, a.aB,
                       a.arm_stride, a.state, a.state_stride, a.status);
    SMT_LAUNCH_CHECK();
    for (int k = 1; k <= iters; k++) {
        if (form == SMT_REFINE_FORM_DIRECT)
            hipLaunchKernelGGL(k_vote_direct, dim3(dgx, gy), dim3(256), 0, st, src, dst, pairs, H, W, D, a.aL, a.aR, a.aT,
                               a.aB, a.arm_stride, a.P.irv_ts, a.P.irv_th, k, a.state, a.state_stride, a.status, hist);
        else
            hipLaunchKernelGGL(k_vote_wave, dim3((unsigned)(nseg * H), gy), dim3(RV_WAVES * 64), 0, st, src, dst, pairs, H,
                               W, D, nseg, a.aL, a.aR, a.aT, a.aB, a.arm_stride, a.P.irv_ts, a.P.irv_th, k, a.state,
                               a.state_stride, a.status);
        SMT_LAUNCH_CHECK();
        g_refine_last_form = form;
        const maps_view t = src; src = dst; dst = t;
    }
    if (a.interp) {
        const unsigned gx = (unsigned)(((long long)nseg * H + 3) / 4);
        hipLaunchKernelGGL(k_interpolate, dim3(gx, gy), dim3(256), 0, st, src, dst, pairs, H, W, D, nseg, a.cls,
                           a.cls_stride, a.gray, a.gray_stride, a.P.search, a.state, a.state_stride, a.status);
        SMT_LAUNCH_CHECK();
    }
    return SMT_OK;
}

// ---- host twins: plain loops through refine_rule.h -------------------------------------------------------------------
int refine_host(const refine_args &a)
{
    const int H = a.H, W = a.W, D = a.D;
    const size_t N = (size_t)H * W;
    float *tmp = (float *)malloc(N * sizeof(float));
    int *hist = (int *)malloc((size_t)D * sizeof(int));
    if (!tmp || !hist) { free(tmp); free(hist); return SMT_ERR_ALLOC; }
    for (int p = 0; p < a.pairs; p++) {
        float *M = a.maps + p * a.map_stride;
        uint8_t *state = a.state ? a.state + p * a.state_stride : nullptr;
        int st[4] = {0, 0, 0, 0};
        for (size_t x = 0; x < N; x++) {
            const bool out = !rr::reliable(M[x], D);
            st[0] += out;
            if (state) state[x] = out ? SMT_REFINE_STATE_OUTLIER : 0;
        }
        if (a.vote) {
            const int *pL = a.aL + p * a.arm_stride, *pR = a.aR + p * a.arm_stride, *pT = a.aT + p * a.arm_stride,
                      *pB = a.aB + p * a.arm_stride;
            for (size_t x = 0; x < N; x++)
                if (rr::arm_out_of_range(pL[x]) || rr::arm_out_of_range(pR[x]) || rr::arm_out_of_range(pT[x]) ||
                    rr::arm_out_of_range(pB[x]))
                    st[3] |= SMT_REFINE_ARM_CLAMPED;
            for (int k = 1; k <= a.P.irv_iters; k++) {
                memcpy(tmp, M, N * sizeof(float));                          // M' is written from the whole of M
                for (int i = 0; i < H; i++)
                    for (int j = 0; j < W; j++) {
                        const size_t idx = (size_t)i * W + j;
                        if (rr::reliable(tmp[idx], D)) continue;
                        memset(hist, 0, (size_t)D * sizeof(int));
                        int S = 0;
                        const int r0 = rr::span_lo(i, pT[idx]), r1 = rr::span_hi(i, pB[idx], H);
                        for (int r = r0; r <= r1; r++) {
                            const size_t q = (size_t)r * W + j;
                            const int c0 = rr::span_lo(j, pL[q]), c1 = rr::span_hi(j, pR[q], W);
                            for (int c = c0; c <= c1; c++) {
                                const float x = tmp[(size_t)r * W + c];
                                if (rr::reliable(x, D)) { hist[rr::bin_of(x, D)]++; S++; }
                            }
                        }
                        int h = 0, d = 0;
                        for (int b = 0; b < D; b++)
                            if (hist[b] > h) { h = hist[b]; d = b; }
                        if (rr::vote_fills(S, h, a.P.irv_ts, a.P.irv_th)) {
                            M[idx] = (float)d;
                            st[1]++;
                            if (state) state[idx] = (uint8_t)k;
                        }
                    }
            }
        }
        if (a.interp) {
            const uint8_t *pc = a.cls + p * a.cls_stride, *pg = a.gray + p * a.gray_stride;
            memcpy(tmp, M, N * sizeof(float));
            for (int i = 0; i < H; i++)
                for (int j = 0; j < W; j++) {
                    const size_t idx = (size_t)i * W + j;
                    if (rr::reliable(tmp[idx], D)) continue;
                    unsigned best = 0;
                    long long win = -1;
                    for (int n = 0; n < rr::RAYS; n++) {
                        const long long q = rr::ray_candidate(tmp, H, W, D, i, j, n, a.P.search);
                        if (q < 0) continue;
                        unsigned bits;
                        memcpy(&bits, &tmp[q], 4);
                        const unsigned key = rr::cand_key(pc[idx] == 1, bits, pg[idx], pg[q]);
                        if (win < 0 || key < best) { best = key; win = q; }
                    }
                    if (win >= 0) {
                        M[idx] = tmp[win];
                        st[2]++;
                        if (state) state[idx] = SMT_REFINE_STATE_INTERPOLATED;
                    }
                }
        }
        if (a.status) memcpy(a.status + 4 * p, st, sizeof(st));
    }
    free(tmp); free(hist);
    return SMT_OK;
}

}  // namespace

SMT_API void smt_refine_default_params(smt_refine_params *p)
{
    if (!p) return;
    p->irv_ts = 20; p->irv_th = 0.4f;                    // adcensus_types.h:58-59, 72
    p->irv_iters = 5; p->search = 0;
}

SMT_API int smt_refine_set_impl(int impl)
{
    if (impl != 0 && impl != SMT_REFINE_FORM_DIRECT && impl != SMT_REFINE_FORM_WAVE) return SMT_ERR_ARG;
    g_refine_impl = impl;
    return SMT_OK;
}

SMT_API int smt_refine_last_form(void) { return g_refine_last_form; }

#define REFINE_VOTE_ARGS(a) \
    refine_args a{maps, pairs, map_stride, armL, armR, armT, armB, arm_stride, nullptr, 0, nullptr, 0, H, W, D, {}, state, state_stride, status, true, false}
#define REFINE_INTERP_ARGS(a) \
    refine_args a{maps, pairs, map_stride, nullptr, nullptr, nullptr, nullptr, 0, cls, cls_stride, gray, gray_stride, H, W, D, {}, state, state_stride, status, false, true}
#define REFINE_BOTH_ARGS(a) \
    refine_args a{maps, pairs, map_stride, armL, armR, armT, armB, arm_stride, cls, cls_stride, gray, gray_stride, H, W, D, {}, state, state_stride, status, true, true}

SMT_API int smt_region_vote_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR,
                                  const int *armT, const int *armB, size_t arm_stride, int H, int W, int D,
                                  const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status,
                                  void *stream)
{
    REFINE_VOTE_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_enqueue(a, smt_stream(stream));
}

SMT_API int smt_interpolate_outliers_batch(float *maps, int pairs, size_t map_stride, const uint8_t *cls, size_t cls_stride,
                                           const uint8_t *gray, size_t gray_stride, int H, int W, int D,
                                           const smt_refine_params *params, uint8_t *state, size_t state_stride,
                                           int *status, void *stream)
{
    REFINE_INTERP_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_enqueue(a, smt_stream(stream));
}

SMT_API int smt_refine_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT,
                             const int *armB, size_t arm_stride, const uint8_t *cls, size_t cls_stride,
                             const uint8_t *gray, size_t gray_stride, int H, int W, int D, const smt_refine_params *params,
                             uint8_t *state, size_t state_stride, int *status, void *stream)
{
    REFINE_BOTH_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_enqueue(a, smt_stream(stream));
}

SMT_API int smt_region_vote_batch_host(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR,
                                       const int *armT, const int *armB, size_t arm_stride, int H, int W, int D,
                                       const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status)
{
    REFINE_VOTE_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_host(a);
}

SMT_API int smt_interpolate_outliers_batch_host(float *maps, int pairs, size_t map_stride, const uint8_t *cls,
                                                size_t cls_stride, const uint8_t *gray, size_t gray_stride, int H, int W,
                                                int D, const smt_refine_params *params, uint8_t *state,
                                                size_t state_stride, int *status)
{
    REFINE_INTERP_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_host(a);
}

SMT_API int smt_refine_batch_host(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR,
                                  const int *armT, const int *armB, size_t arm_stride, const uint8_t *cls,
                                  size_t cls_stride, const uint8_t *gray, size_t gray_stride, int H, int W, int D,
                                  const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status)
{
    REFINE_BOTH_ARGS(a);
    const int rc = refine_check(a, params);
    return rc != SMT_OK ? rc : refine_host(a);
}
