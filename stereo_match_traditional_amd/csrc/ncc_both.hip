// smt_lrncc: both views of NCC (NCC.h:69-95 and its mirror) from one pass over the costs.
//
// The reference has no NCC right view; the definition (include/smt.h) mirrors NCC_algorithem as GetPointDepthRight
// mirrors GetPointDepthLeft: costR[i][x'][d] = ComputeCost(R window at (i, x'), L window at (i, x' + d)) while
// x' + winSize + d <= W - 1, the sentinel 255.0 beyond, and dispR = WinTakeAll of that row.  On the integer forms
// (k_ncc2, k_ncc_box) ncc_int_cost is symmetric in its two windows -- n Sab - Sa Sb is an exact integer and ra rb
// commutes -- so costR[i][x'][d] is costL[i][x' + d][d] bit for bit, and every real right-view hypothesis is one the left
// view evaluates (x = x' + d is interior and x - winSize - d >= 0).
//
// KEYS      the left cost kernel publishes each real, non-NaN cost to right pixel x - d as a rank key (csrc/ncc_keys.h),
//           combined per workgroup in LDS, one agent-scope maximum per touched pixel into an [H][W] uint64 map in arena
//           scratch; k_lrncc_finish reads the map and resolves what a key cannot carry.
// COMPOSED  both images flipped left-right on the device, the single-view path on (flip R, flip L), map and costs flipped
//           back: the independent formulation, and the form of the loop nest, whose float64 sums are not symmetric.
// costR under KEYS is a diagonal gather of costL (in scratch when the caller takes none).
#include "smt_common.h"
#include "ncc_keys.h"
#include "box_stage.h"
#include <math.h>
#include <vector>

namespace {

int g_lrncc_impl = 0;          // 0: lrncc_rule; 1: COMPOSED; 2: KEYS wherever it exists
int g_lrncc_last = 0;          // what the last call ran: SMT_LRNCC_FORM_*

// Which form serves (left form, side, D) by default.  Measured on one MI355X at 450x375 (tools/ncc_both_time.py,
// profiles/ncc_both_time.json; KEYS over two smt_ncc calls, medians of 21 interleaved samples, every KEYS median below
// the baseline's minimum):
//   dot4, D = 64:  0.61 at 9x9, 0.59 at 21x21, 0.54 at 31x31;   D = 200: 0.55 at 21x21;
//   box,  D = 64:  0.73 at 9x9, 0.73 at 21x21, 0.72 at 31x31, 0.71 at 45x45;   D = 200: 0.55 at 21x21;
//   8-pair flow at 21x21, D = 200: 0.54 (dot4, the default rule there) and 0.54 (box).
// KEYS therefore serves wherever it exists.  Only those sizes are timed; every other side and D (D > 256 with its
// eight-slot kernels included) inherits the nearest of them and is extrapolation.
bool lrncc_rule(int form, long long side, int D)
{
    (void)side; (void)D;
    return form != SMT_NCC_FORM_LOOP;
}

// dst[r][x][0 .. E) = src[r][W - 1 - x][0 .. E)
template <typename T>
__global__ void __launch_bounds__(256) k_lrncc_flip(const T *__restrict__ src, T *__restrict__ dst, size_t rows, int W, int E)
{
    const size_t n = rows * W * E;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const size_t px = t / E;
        const int e = (int)(t - px * E);
        const size_t r = px / W;
        const int x = (int)(px - r * W);
        dst[t] = src[(r * W + (W - 1 - x)) * E + e];
    }
}

// The right map from the key map, every pixel of [pairs][H][W].  Interior pixel (i, x'): 0 when the cost at d = 0 is NaN
// (ra rb == 0: a flat window on either side; WinTakeAll's running maximum starts as NaN and nothing beats it); else, when
// a hypothesis below D is a sentinel, the first of them, d = W - winSize - x' >= 1 (255.0 beats every real cost and
// later sentinels do not beat it); else the hypothesis the largest key names.
__global__ void __launch_bounds__(256) k_lrncc_finish(const unsigned long long *__restrict__ keys, const double *__restrict__ rootL,
                                                      const double *__restrict__ rootR, size_t total, int H, int W, int D,
                                                      int win, int32_t *__restrict__ dispR)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const size_t row = p / W;
    const int x = (int)(p - row * W), i = (int)(row % H);
    int out = 0;
    if (i >= win && i < H - win && x >= win && x < W - win && rootL[p] * rootR[p] != 0.0) {
        const int ds = W - win - x;
        if (ds < D) out = ds;
        else {
            const unsigned long long k = keys[p];
            out = k ? ncc_rank_key_d(k) : 0;
        }
    }
    dispR[p] = out;
}

// costR[p][d] = costL[p + d][d] while x + d <= W - winSize - 1, 255.0 beyond; 0.0 on the border
__global__ void __launch_bounds__(256) k_lrncc_diag(const double *__restrict__ costL, size_t total, int H, int W, int D, int win,
                                                    double *__restrict__ costR)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / D;
    const int d = (int)(t - p * D);
    const size_t row = p / W;
    const int x = (int)(p - row * W), i = (int)(row % H);
    double c = 0.0;
    if (i >= win && i < H - win && x >= win && x < W - win) c = x + d <= W - win - 1 ? costL[(p + d) * D + d] : 255.0;
    costR[t] = c;
}

template <typename T>
int flip(hipStream_t st, const T *src, T *dst, size_t rows, int W, int E)
{
    const size_t n = rows * W * E;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 65535 * 16 ? (n + 255) / 256 : 65535 * 16);
    hipLaunchKernelGGL(k_lrncc_flip<T>, dim3(blocks), dim3(256), 0, st, src, dst, rows, W, E);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// the single view of `pairs` pairs as smt_ncc and smt_ncc_flow_run_batch write it: borders, then the form's launches
int left_view(int form, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int win, int *sumL, double *rootL,
              int *sumR, double *rootR, int32_t *disp, double *cost, unsigned long long *rkeys, hipStream_t st)
{
    const size_t N = (size_t)H * W;
    const long long Hi = (long long)H - 2LL * win, Wi = (long long)W - 2LL * win;
    if (cost && win > 0) SMT_HIP(hipMemsetAsync(cost, 0, (size_t)pairs * N * D * 8, st));
    if (form != SMT_NCC_FORM_LOOP || Hi <= 0 || Wi <= 0) SMT_HIP(hipMemsetAsync(disp, 0, (size_t)pairs * N * 4, st));
    if (Hi <= 0 || Wi <= 0) return SMT_OK;
    if (form == SMT_NCC_FORM_LOOP) return smt_ncc_loop_enqueue(L, R, pairs, H, W, D, win, disp, cost, st);
    const int rc = smt_ncc_stats_enqueue(L, R, pairs, H, W, win, sumL, rootL, sumR, rootR, st);
    if (rc != SMT_OK) return rc;
    return form == SMT_NCC_FORM_DOT4 ? smt_ncc_dot4_enqueue(L, R, pairs, H, W, D, win, sumL, rootL, sumR, rootR, disp, cost, st, rkeys)
                                     : smt_ncc_box_enqueue(L, R, pairs, H, W, D, win, sumL, rootL, sumR, rootR, disp, cost, st, rkeys);
}

}  // namespace

int smt_lrncc_enqueue(int form, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int win, int *sumL,
                      double *rootL, int *sumR, double *rootR, int32_t *dispL, int32_t *dispR, double *costL, double *costR,
                      hipStream_t st)
{
    const size_t N = (size_t)H * W, PN = (size_t)pairs * N;
    const long long Hi = (long long)H - 2LL * win, Wi = (long long)W - 2LL * win, side = 2LL * win + 1;
    if (Hi <= 0 || Wi <= 0) {                                  // all border: zero maps, zero costs
        const int rc = left_view(form, L, R, pairs, H, W, D, win, sumL, rootL, sumR, rootR, dispL, costL, nullptr, st);
        if (rc != SMT_OK) return rc;
        SMT_HIP(hipMemsetAsync(dispR, 0, PN * 4, st));
        if (costR) SMT_HIP(hipMemsetAsync(costR, 0, PN * D * 8, st));
        return SMT_OK;
    }
    scratch_set S(st);
    const bool keys_exist = form != SMT_NCC_FORM_LOOP;
    bool use_keys = keys_exist && g_lrncc_impl != 1 && (g_lrncc_impl == 2 || lrncc_rule(form, side, D));
    unsigned long long *keys = nullptr;
    double *cl = costL;
    if (use_keys) {
        keys = (unsigned long long *)S.get(PN * 8);
        if (keys && costR && !cl) cl = (double *)S.get(PN * D * 8);
        if (!keys || (costR && !cl)) use_keys = false;         // scratch that cannot be had: the composed form
    }
    if (use_keys) {
        SMT_HIP(hipMemsetAsync(keys, 0, PN * 8, st));
        int rc = left_view(form, L, R, pairs, H, W, D, win, sumL, rootL, sumR, rootR, dispL, cl, keys, st);
        if (rc != SMT_OK) return rc;
        hipLaunchKernelGGL(k_lrncc_finish, dim3((unsigned)((PN + 255) / 256)), dim3(256), 0, st, keys, rootL, rootR, PN, H, W, D, win,
                           dispR);
        if (costR)
            hipLaunchKernelGGL(k_lrncc_diag, dim3((unsigned)((PN * D + 255) / 256)), dim3(256), 0, st, cl, PN * D, H, W, D, win, costR);
        SMT_LAUNCH_CHECK();
        g_lrncc_last = SMT_LRNCC_FORM_KEYS;
        return SMT_OK;
    }
    // COMPOSED: dispR = fliplr(NCC_algorithem(fliplr(R), fliplr(L))), the costs likewise
    int rc = left_view(form, L, R, pairs, H, W, D, win, sumL, rootL, sumR, rootR, dispL, costL, nullptr, st);
    if (rc != SMT_OK) return rc;
    uint8_t *fimg = (uint8_t *)S.get(2 * PN);                  // flip R, then flip L
    int32_t *fmap = (int32_t *)S.get(PN * 4);
    double *fcost = costR ? (double *)S.get(PN * D * 8) : nullptr;
    if (!fimg || !fmap || (costR && !fcost)) return SMT_ERR_ALLOC;
    rc = flip(st, R, fimg, (size_t)pairs * H, W, 1);
    if (rc == SMT_OK) rc = flip(st, L, fimg + PN, (size_t)pairs * H, W, 1);
    if (rc == SMT_OK) rc = left_view(form, fimg, fimg + PN, pairs, H, W, D, win, sumL, rootL, sumR, rootR, fmap, fcost, nullptr, st);
    if (rc == SMT_OK) rc = flip(st, fmap, dispR, (size_t)pairs * H, W, 1);
    if (rc == SMT_OK && costR) rc = flip(st, fcost, costR, (size_t)pairs * H, W, D);
    if (rc != SMT_OK) return rc;
    g_lrncc_last = SMT_LRNCC_FORM_COMPOSED;
    return SMT_OK;
}

SMT_API int smt_lrncc_set_impl(int impl)
{
    if (impl < 0 || impl > 2) return SMT_ERR_ARG;
    g_lrncc_impl = impl;
    return SMT_OK;
}

SMT_API int smt_lrncc_last_form(void) { return g_lrncc_last; }

SMT_API int smt_lrncc(const uint8_t *L, const uint8_t *R, int H, int W, int D, int winSize, int32_t *dispL, int32_t *dispR,
                      double *costL, double *costR, void *stream)
{
    if (!L || !R || !dispL || !dispR || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winSize < 0 ||
        (size_t)H * W >= ((size_t)1 << 31))
        return SMT_ERR_ARG;
    hipStream_t st = smt_stream(stream);
    const size_t N = (size_t)H * W;
    const long long side = 2LL * winSize + 1;
    const int Hi = H - 2 * winSize, Wi = W - 2 * winSize;
    const int impl = smt_ncc_current_impl();
    int form = SMT_NCC_FORM_LOOP;                              // as smt_ncc chooses
    if (impl == 2 && side <= 31) form = SMT_NCC_FORM_DOT4;
    else if (impl == 3 && side <= 181 && smt_ncc_stats_ready(winSize)) form = SMT_NCC_FORM_BOX;
    scratch_set S(st);
    int *sums = nullptr;
    double *roots = nullptr;
    if (form != SMT_NCC_FORM_LOOP && Hi > 0 && Wi > 0) {
        roots = (double *)S.get(N * 8 * 2);
        if (roots) {
            sums = (int *)S.get(N * 4 * 2);
            if (!sums) return SMT_ERR_ALLOC;
        } else form = SMT_NCC_FORM_LOOP;                       // no scratch memory: the first formulation, as smt_ncc
    }
    return smt_lrncc_enqueue(form, L, R, 1, H, W, D, winSize, sums, roots, sums ? sums + N : nullptr, roots ? roots + N : nullptr,
                             dispL, dispR, costL, costR, st);
}

// Host only (no GPU).  Left costs [Wi][D] over the Wi = W - 2 winSize interior columns of one row, drawn from a hostile
// palette by seed % 4 -- exact ties; pairs of doubles that round down and up to one float; NaN at d = 0 and at d > 0;
// all of them mixed -- : for every right pixel x', the hypothesis named by the largest published key, with the NaN-at-0
// and first-sentinel rules of k_lrncc_finish, equals WinTakeAll (NCC.h:53-67) run sequentially over the row
// c[d] = costL[x' + d][d] while x' + d <= Wi - 1, 255.0 beyond.  W < D and W <= 2 winSize (nothing to compare) are fine.
SMT_API int smt_lrncc_selftest_keys(int W, int D, int winSize, unsigned seed)
{
    if (W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winSize < 0 || W > (1 << 16)) return SMT_ERR_ARG;
    const long long Wi = (long long)W - 2LL * winSize;
    if (Wi <= 0) return SMT_OK;
    host_rng rng(seed);
    const int mode = (int)(seed % 4);
    // floats F and doubles just above / below them that narrow to F (spacing of float near 0.5 is 2^-24 .. 2^-25)
    const double F1 = 0.5, F2 = (double)0.7310586f, F3 = -0.25, e = ldexp(1.0, -40);
    const double ties[] = {F1, F1, F2, F2, F3, 0.0, -0.0, 1.0, 1.0, -1.0};
    const double near[] = {F1, F1 + e, F1 - e / 2, F1 + 3 * e, F2, F2 + e, F2 - e, F2 + 2 * e, 1.0, 1.0 - e / 4, F3 + e, F3 - e};
    const double qnan = nan("");
    std::vector<double> cl((size_t)Wi * D), row(D);
    for (auto &c : cl) {
        const uint32_t r = rng.next();
        switch (mode) {
        case 0: c = ties[(r >> 4) % 10]; break;
        case 1: c = near[(r >> 4) % 12]; break;
        case 2: c = (r % 3 == 0) ? qnan : ties[(r >> 4) % 10]; break;
        default: c = (r % 7 == 0) ? qnan : (r % 7 < 3 ? near[(r >> 4) % 12] : (r % 7 < 5 ? ties[(r >> 4) % 10]
                                                                                      : (double)(int)((r >> 8) % 2001 - 1000) / 1000.0)); break;
        }
    }
    for (long long x = 0; x < Wi; x++) {
        for (int d = 0; d < D; d++) row[d] = x + d <= Wi - 1 ? cl[(size_t)(x + d) * D + d] : 255.0;
        int want = 0;
        float m = (float)row[0];
        for (int d = 1; d < D; d++)
            if ((double)m < row[d]) { want = d; m = (float)row[d]; }
        unsigned long long best = 0;
        for (int d = 0; d < D && x + d <= Wi - 1; d++) {
            const double c = row[d];
            if (c != c) continue;                              // NaN costs publish nothing
            const unsigned long long k = ncc_rank_key(c, d);
            if (k == 0 || ncc_rank_key_d(k) != d) return SMT_ERR_STATE;
            if (k > best) best = k;
        }
        int got = 0;
        if (row[0] == row[0]) {                                // the kernel's test is ra rb != 0, the same statement
            const long long ds = Wi - x;                       // = W - winSize - (x + winSize)
            got = ds < D ? (int)ds : (best ? ncc_rank_key_d(best) : 0);
        }
        if (got != want) return SMT_ERR_STATE;
    }
    return SMT_OK;
}
