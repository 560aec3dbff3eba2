// k_ncc_box: the cross term of NCC (NCC.h:15-49) as a running box sum, for windows up to 181 x 181, and smt_ncc_flow_*:
// NCC_main.cpp:33 for a batch of gray pairs.
//
// With Sab[i][x][d] = the side x side box sum of P_d[y][c] = L[y][c] * R[y][c - d] over rows i .. i + side - 1 and columns
// x .. x + side - 1 (window corners, image coordinates), the cost of output pixel (i + win, x + win) at hypothesis d is the
// expression of k_ncc2 (csrc/ncc_common.h) on the same integers; only the route to Sab differs.  A lane owns the
// hypotheses d = lane + 64 k and keeps, per column of its strip, the running box sum in a register; it moves the sum one
// image row down by adding the entering row's horizontal window sums and subtracting the leaving row's, and a horizontal
// window sum slides along the row (add the entering column's product, subtract the leaving one's).  The work per
// hypothesis does not depend on side (k_ncc2 needs side^2 / 4 v_dot4).  All of it is uint32 arithmetic, exact modulo
// 2^32; the true sums are below 255^2 side^2 < 2^31 for side <= 181, so every valid Sab is the integer k_ncc2 holds.
#include "smt_common.h"
#include "ncc_common.h"
#include "box_stage.h"
#include <new>
#include <stdlib.h>
#include <type_traits>
#include <vector>

namespace {

constexpr int BNT = 256;                 // four waves per workgroup
constexpr int BS = 16;                   // columns per wave: C[BS][KT] running box sums in VGPRs
constexpr int BSW = BS * (BNT / 64);     // columns per workgroup (the strip width)

// grid (strips of BSW window columns, bands of `band` window rows, pairs).  The staged rows, the running sums and the step
// loop of a band are box_steps (csrc/box_stage.h) with the v_dot4 tap, over window rows and columns: step t brings in
// image row i0 + t and, from t = side - 1 on, emits window row io = i0 + t - side + 1, i.e. image row io + win.  Left
// entries start at column x0, right entries at x0 - 64 KT; a hypothesis that reads clamped columns (x - d < 0) keeps
// consistent running sums and costs 255.0 whatever they hold.  What is here is the emit step: the cost, the ordered
// WinTakeAll and PUB's keys.
//
// PUB (the both-view call, csrc/ncc_both.hip): every real, non-NaN cost of (x, d) is also offered to right pixel x - d as
// a rank key (csrc/ncc_keys.h).  The workgroup's 64 columns times 64 KT hypotheses reach 64 KT + 64 right pixels of a
// row; the offers of one step are combined by 64-bit LDS maxima in one of two key rows, and the step after it sends one
// agent-scope maximum per touched pixel to rkeys ([pairs][H][W], zero before the launch) and clears the row -- behind
// the step's own barrier, so no barrier is added.
template <int KT, bool PUB>
__global__ void __launch_bounds__(BNT) k_ncc_box(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int H, int W,
                                                 int D, int win, int band, const int *__restrict__ sumL,
                                                 const double *__restrict__ rootL, const int *__restrict__ sumR,
                                                 const double *__restrict__ rootR, int32_t *__restrict__ disp,
                                                 double *__restrict__ cost_out, unsigned long long *__restrict__ rkeys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_nbox[];
    const int side = 2 * win + 1, Hi = H - 2 * win, Wi = W - 2 * win;
    {                                                          // blockIdx.z: the pair of a batch ([pairs][H][W] everything)
        const size_t po = (size_t)blockIdx.z * H * W;
        L += po; R += po; sumL += po; rootL += po; sumR += po; rootR += po; disp += po;
        if (cost_out) cost_out += po * D;
        if constexpr (PUB) rkeys += po;
    }
    const int x0 = blockIdx.x * BSW, i0 = blockIdx.y * band;
    const int i1 = i0 + band < Hi ? i0 + band : Hi;
    const int nk = (D + 63) >> 6;                              // live hypothesis slots (uniform)
    const int ROWE = box_lwe(side, BSW) + box_rwe(side, KT, BSW);
    // PUB: [2][NKE] keys behind the staged rows; entry e of a row is right window column x0 - 64 KT + e
    constexpr int NKE = 64 * KT + BSW;
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(s_nbox + 4 * ROWE);
    auto flush = [&](int half, int io) __attribute__((always_inline)) {   // the keys of window row io go out, the row is cleared
        for (int e = threadIdx.x; e < NKE; e += BNT) {
            const unsigned long long v = s_keys[half * NKE + e];
            if (v) {
                atomicMax(rkeys + (size_t)(io + win) * W + win + (x0 - 64 * KT + e), v);
                s_keys[half * NKE + e] = 0ull;
            }
        }
    };
    if constexpr (PUB)
        for (int e = threadIdx.x; e < 2 * NKE; e += BNT) s_keys[e] = 0ull;

    const double n = (double)(side * side);
    auto pre = [&](int half, int io) __attribute__((always_inline)) {
        if constexpr (PUB)
            if (io > i0) flush(half ^ 1, io - 1);              // what the step before emitted
    };
    auto emit = [&](int half, int io, int x, const unsigned (&Cj)[KT]) __attribute__((always_inline)) {
        const int lane = threadIdx.x & 63;                     // not captured: see box_steps
        const size_t p = (size_t)(io + win) * W + x + win;
        const double sa = (double)sumL[p], rta = rootL[p];
        double c[KT];
        float v[KT];
        bool poison = false;
#pragma unroll
        for (int k = 0; k < KT; k++) {
            const int d = lane + 64 * k;
            const bool act = k < nk && d < D;
            if (act && x - d >= 0) {
                const size_t q = p - d;
                c[k] = ncc_int_cost(n, Cj[k], sa, rta, sumR[q], rootR[q]);
            } else c[k] = 255.0;                               // `invalid` 0xff, NCC.h:88
            if (cost_out && act) cost_out[p * D + d] = c[k];
            if constexpr (PUB)
                if (act && x - d >= 0 && c[k] == c[k])
                    atomicMax(s_keys + half * NKE + (x - d - (x0 - 64 * KT)), ncc_rank_key(c[k], d));
            if (k == 0) poison = __ballot(c[0] != c[0] && lane == 0) != 0;   // d = 0 is slot 0 of lane 0
            v[k] = ncc_wta_term(c[k], act);
        }
        // WinTakeAll in d order = (slot, lane): before (k, lane) = max(every lane of the slots < k, the lanes below `lane`
        // of slot k)
        float below = -INFINITY;
        unsigned key = 0;                                      // 1 + the largest winning d of the lane (0: none)
#pragma unroll
        for (int k = 0; k < KT; k++)
            if (k < nk) {
                const int d = lane + 64 * k;
                const float inc = wave_prefix_max_f32(v[k], lane);
                const float up = __shfl_up(inc, 1, WAVE);
                const float m = fmaxf(below, lane >= 1 ? up : -INFINITY);
                if (d < D && (double)m < c[k]) key = (unsigned)d + 1u;   // d grows with k
                below = fmaxf(below, __shfl(inc, 63, WAVE));
            }
        const int out = ncc_wta_last(key, poison);
        if (lane == 0) disp[p] = out;
    };
    box_steps<KT, BS, BNT, box_tap_dot, -1>(s_nbox, L, R, W, x0 - box_tap_dot::LEAD, x0 - 64 * KT, x0, i0, i1, Wi, side, nk, pre,
                                            box_no_hook(), emit);
    // the last step's row (i1 > i0: it emitted), in the last step's half
    if constexpr (PUB) flush((side - 2 + (i1 - i0)) & 1, i1 - 1);
}

int g_ncc_box_band = 0;        // test hook: window rows per band, 0 = box_band's choice

template <int KT>
int launch_nbox(hipStream_t st, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int win, const int *sumL,
                const double *rootL, const int *sumR, const double *rootR, int32_t *disp, double *cost,
                unsigned long long *rkeys)
{
    const int side = 2 * win + 1, Hi = H - 2 * win, Wi = W - 2 * win, band = box_band_rule(g_ncc_box_band, Hi, Wi, side, BSW);
    const size_t shm = (size_t)4 * (box_lwe(side, BSW) + box_rwe(side, KT, BSW)) * 4;   // <= 16 KiB; two staging items per thread suffice
    static_assert(2 * (((BSW + NCC_INT_MAX_SIDE + 3) & ~3) + ((64 * KT + BSW + NCC_INT_MAX_SIDE + 3) & ~3)) / 4 <= 2 * BNT, "staging items");
    const dim3 grid((Wi + BSW - 1) / BSW, (Hi + band - 1) / band, pairs);
    if (rkeys)                                                 // + the two key rows, at most 9 KiB
        hipLaunchKernelGGL((k_ncc_box<KT, true>), grid, dim3(BNT), shm + (size_t)2 * (64 * KT + BSW) * 8, st, L, R, H, W, D, win, band,
                           sumL, rootL, sumR, rootR, disp, cost, rkeys);
    else
        hipLaunchKernelGGL((k_ncc_box<KT, false>), grid, dim3(BNT), shm, st, L, R, H, W, D, win, band, sumL, rootL, sumR, rootR, disp,
                           cost, rkeys);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// Which cost launch serves (side, D) in smt_ncc_flow_run_batch by default.  Measured on one MI355X at 450x375
// (tools/ncc_box_time.py, profiles/ncc_box_time.json; box over dot4, medians of 21 interleaved samples):
//   D = 64:  0.84 at 9x9, 0.59 at 21x21, 0.47 at 31x31 -- the box form wins, more with every side;
//   D = 200: 3.40 at 9x9, 2.61 at 21x21, 2.22 at 31x31 -- the KT = 4 instantiation loses at every side k_ncc2 covers;
//   45x45, D = 64: 0.205 ms against the loop nest's 8.146 ms (0.025).
// Up to 31x31 the box form therefore serves 33 <= D <= 64 at sides 9 .. 31 and k_ncc2 everything else.  Of that branch
// only D = 64 at sides 9, 21 and 31 on a 450x375 image is timed; the rest of it is extrapolation: the sides in between
// (the ratio falls from side to side), and D = 33 .. 63, where both kernels run the same one-slot instantiation with
// more than half of their lanes at work.  D <= 32, sides below 9, D = 65 .. 199 and D > 200 are not timed and stay
// with k_ncc2, which served them before.  The box form takes 33 .. 181 at every D, where the only alternative is the
// loop nest whose work grows with side^2 (timed at 45x45, D = 64 only; D > 64 there, D > 256 included, is not timed).
int ncc_flow_rule(long long side, int D)
{
    if (side <= 31) return (side >= 9 && D >= 33 && D <= 64) ? SMT_NCC_FORM_BOX : SMT_NCC_FORM_DOT4;
    if (side <= NCC_INT_MAX_SIDE) return SMT_NCC_FORM_BOX;
    return SMT_NCC_FORM_LOOP;
}

}  // namespace

// side <= 181, interior not empty, tables from ncc_stats_launch (declared in csrc/smt_common.h); rkeys: NULL, or the
// zeroed [pairs][H][W] key map of the both-view call
int smt_ncc_box_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int winSize, const int *sumL,
                        const double *rootL, const int *sumR, const double *rootR, int32_t *disp, double *cost, hipStream_t st,
                        unsigned long long *rkeys)
{
    const int rc = box_dispatch_kt(D, [&](auto kt) {
        return launch_nbox<decltype(kt)::value>(st, L, R, pairs, H, W, D, winSize, sumL, rootL, sumR, rootR, disp, cost, rkeys);
    });
    if (rc == SMT_OK) g_smt_ncc_last_form = SMT_NCC_FORM_BOX;
    return rc;
}

// the statistics pass and the flow's dispatch rule for csrc/ncc_both.hip (this translation unit's copy of k_ncc_stats)
bool smt_ncc_stats_ready(int winSize) { return ncc_stats_ready(winSize); }
int smt_ncc_stats_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int winSize, int *sumL, double *rootL,
                          int *sumR, double *rootR, hipStream_t st)
{
    return ncc_stats_launch(st, L, R, pairs, H, W, winSize, sumL, rootL, sumR, rootR);
}

SMT_API int smt_ncc_box_set_band(int band)
{
    if (band < 0) return SMT_ERR_ARG;
    g_ncc_box_band = band;
    return SMT_OK;
}

// ---- host-only check -----------------------------------------------------------------------------------------------
// box_host<Tap>, the restatement of the kernel's recurrence: csrc/box_stage.h

// Host only (no GPU).  On four unpadded pairs of the given shape -- pseudo-random, 255 against 255 (the largest sums),
// opposed checkerboards, a shifted copy -- the restated recurrence of k_ncc_box (box_host<box_tap_dot>, under the band the launch
// would choose and under a band of 1 and of 3 rows) equals the direct double loop sum a b over the window for every
// (i, x, d); columns left of the image are read clamped by both.  An empty interior has nothing to compare: SMT_OK.
SMT_API int smt_ncc_selftest_box(int H, int W, int D, int winSize, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || winSize < 0 || 2LL * winSize + 1 > NCC_INT_MAX_SIDE ||
        (long long)H * W * D > (1 << 24))
        return SMT_ERR_ARG;
    const int win = winSize, side = 2 * win + 1, Hi = H - 2 * win, Wi = W - 2 * win;
    if (Hi <= 0 || Wi <= 0) return SMT_OK;
    std::vector<uint8_t> L((size_t)H * W), R((size_t)H * W);
    std::vector<unsigned> want((size_t)Hi * Wi * D), got((size_t)Hi * Wi * D);
    host_rng rng(seed);
    for (int pat = 0; pat < 4; pat++) {
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t q = (size_t)y * W + x;
                switch (pat) {
                case 0: L[q] = (uint8_t)rng.next(); R[q] = (uint8_t)rng.next(); break;
                case 1: L[q] = 255; R[q] = 255; break;
                case 2: L[q] = ((x ^ y) & 1) ? 255 : 0; R[q] = ((x ^ y) & 1) ? 0 : 255; break;
                default: L[q] = (uint8_t)((x * 37 + y * 11) ^ (x >> 2)); R[q] = (uint8_t)(((x + 3) * 37 + y * 11) ^ ((x + 3) >> 2)); break;
                }
            }
        for (int i = 0; i < Hi; i++)
            for (int x = 0; x < Wi; x++)
                for (int d = 0; d < D; d++) {
                    unsigned acc = 0;
                    for (int r = 0; r < side; r++)
                        for (int c = 0; c < side; c++) {
                            const int xr = x + c - d < 0 ? 0 : x + c - d;
                            acc += (unsigned)L[(size_t)(i + r) * W + x + c] * (unsigned)R[(size_t)(i + r) * W + xr];
                        }
                    want[((size_t)i * Wi + x) * D + d] = acc;
                }
        const int bands[3] = {box_band(Hi, Wi, side, BSW), 1, 3};
        for (int b = 0; b < 3; b++) {
            std::fill(got.begin(), got.end(), 0xdeadbeefu);
            box_host<box_tap_dot>(L.data(), R.data(), W, Hi, Wi, D, side, bands[b] < Hi ? bands[b] : Hi, got.data());
            if (got != want) return SMT_ERR_STATE;
        }
    }
    return SMT_OK;
}

// ---- smt_ncc_flow_*: NCC_main.cpp:33 for a batch of gray pairs -----------------------------------------------------
// One statistics launch and one cost launch serve the whole batch (the pair on a grid axis).  The handle owns the
// statistics tables, grown to the largest batch it has seen: a warm call allocates nothing and does not synchronise.
struct smt_ncc_flow {
    int device;
    int H, W, D;
    smt_ncc_params P;
    hipStream_t stream;
    int form;                   // 0: ncc_flow_rule; else SMT_NCC_FORM_*
    int cap;                    // pairs the tables hold
    int *sums;                  // [2][cap][H][W]: left, right
    double *roots;              // [2][cap][H][W]
};

// cold: the tables grow to `pairs` (the old ones may still be read, so the stream is waited for)
static int ncc_flow_grow(smt_ncc_flow *h, int pairs)
{
    if (pairs <= h->cap) return SMT_OK;
    const size_t N = (size_t)h->H * h->W;
    SMT_HIP(hipStreamSynchronize(h->stream));
    (void)hipFree(h->sums); (void)hipFree(h->roots);
    h->sums = nullptr; h->roots = nullptr; h->cap = 0;
    int rc = smt_malloc((void **)&h->sums, (size_t)2 * pairs * N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->roots, (size_t)2 * pairs * N * 8);
    if (rc != SMT_OK) { (void)hipFree(h->sums); h->sums = nullptr; return rc; }
    h->cap = pairs;
    return SMT_OK;
}

SMT_API void smt_ncc_default_params(smt_ncc_params *p)
{
    if (!p) return;
    p->winSize = 10;                                          // NCC_main.cpp:17
}

SMT_API int smt_ncc_flow_destroy(smt_ncc_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->sums); (void)hipFree(h->roots);
    delete h;
    return SMT_OK;
}

SMT_API int smt_ncc_flow_create_on(int device, int H, int W, int D, const smt_ncc_params *p, smt_ncc_flow **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    smt_ncc_params P;
    if (p) P = *p; else smt_ncc_default_params(&P);
    if (P.winSize < 0) return SMT_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    smt_ncc_flow *h = new (std::nothrow) smt_ncc_flow();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->P = P;
    *out = h;
    return SMT_OK;
}

SMT_API int smt_ncc_flow_set_stream(smt_ncc_flow *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_ncc_flow_set_form(smt_ncc_flow *h, int form)
{
    if (!h || form < 0 || form > SMT_NCC_FORM_BOX) return SMT_ERR_ARG;
    const long long side = 2LL * h->P.winSize + 1;
    if ((form == SMT_NCC_FORM_DOT4 && side > 31) || (form == SMT_NCC_FORM_BOX && side > NCC_INT_MAX_SIDE)) return SMT_ERR_ARG;
    h->form = form;
    return SMT_OK;
}

SMT_API int smt_ncc_flow_run_batch(smt_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *disp,
                                   double *cost)
{
    if (!h || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR || !disp) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, D = h->D, win = h->P.winSize;
    const size_t N = (size_t)H * W;
    hipStream_t st = h->stream;
    const long long Hi = (long long)H - 2LL * win, Wi = (long long)W - 2LL * win;
    int form = h->form ? h->form : ncc_flow_rule(2LL * win + 1, D);
    if (form != SMT_NCC_FORM_LOOP && Hi > 0 && Wi > 0 && !ncc_stats_ready(win)) form = SMT_NCC_FORM_LOOP;   // as smt_ncc falls back
    // borders: map 0, cost 0.0 (as smt_ncc); an empty interior is all border
    if (cost && win > 0) SMT_HIP(hipMemsetAsync(cost, 0, (size_t)pairs * N * D * 8, st));
    if (form != SMT_NCC_FORM_LOOP || Hi <= 0 || Wi <= 0) SMT_HIP(hipMemsetAsync(disp, 0, (size_t)pairs * N * 4, st));
    if (Hi <= 0 || Wi <= 0) return SMT_OK;
    if (form == SMT_NCC_FORM_LOOP) return smt_ncc_loop_enqueue(grayL, grayR, pairs, H, W, D, win, disp, cost, st);
    int rc = ncc_flow_grow(h, pairs);
    if (rc != SMT_OK) return rc;
    int *sumL = h->sums, *sumR = h->sums + (size_t)h->cap * N;
    double *rootL = h->roots, *rootR = h->roots + (size_t)h->cap * N;
    rc = ncc_stats_launch(st, grayL, grayR, pairs, H, W, win, sumL, rootL, sumR, rootR);
    if (rc != SMT_OK) return rc;
    return form == SMT_NCC_FORM_DOT4 ? smt_ncc_dot4_enqueue(grayL, grayR, pairs, H, W, D, win, sumL, rootL, sumR, rootR, disp, cost, st)
                                     : smt_ncc_box_enqueue(grayL, grayR, pairs, H, W, D, win, sumL, rootL, sumR, rootR, disp, cost, st);
}

// Both views and the int-map cross-check for a batch, on the handle of smt_ncc_flow_run_batch: the form is chosen as
// there, the tables grow as there, and smt_lrncc_enqueue (csrc/ncc_both.hip) does the rest for the whole batch.  Maps
// the caller does not take live in arena scratch for the call.
SMT_API int smt_lrncc_flow_run_batch(smt_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *dispL,
                                     int32_t *dispR, int32_t *lastdisp, uint8_t *cls)
{
    if (!h || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR) return SMT_ERR_ARG;
    if (!dispL && !dispR && !lastdisp && !cls) return SMT_OK;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, D = h->D, win = h->P.winSize;
    const size_t N = (size_t)H * W;
    hipStream_t st = h->stream;
    const long long Hi = (long long)H - 2LL * win, Wi = (long long)W - 2LL * win;
    int form = h->form ? h->form : ncc_flow_rule(2LL * win + 1, D);
    if (form != SMT_NCC_FORM_LOOP && Hi > 0 && Wi > 0 && !ncc_stats_ready(win)) form = SMT_NCC_FORM_LOOP;
    int *sumL = nullptr, *sumR = nullptr;
    double *rootL = nullptr, *rootR = nullptr;
    if (form != SMT_NCC_FORM_LOOP && Hi > 0 && Wi > 0) {
        const int rc = ncc_flow_grow(h, pairs);
        if (rc != SMT_OK) return rc;
        sumL = h->sums; sumR = h->sums + (size_t)h->cap * N;
        rootL = h->roots; rootR = h->roots + (size_t)h->cap * N;
    }
    int32_t *dl = dispL, *dr = dispR, *last1 = nullptr;
    uint8_t *cls1 = nullptr;
    int rc = SMT_OK;
    if (!dl && smt_scratch_alloc((void **)&dl, (size_t)pairs * N * 4, st) != hipSuccess) { dl = nullptr; rc = SMT_ERR_ALLOC; }
    if (rc == SMT_OK && !dr && smt_scratch_alloc((void **)&dr, (size_t)pairs * N * 4, st) != hipSuccess) { dr = nullptr; rc = SMT_ERR_ALLOC; }
    if (rc == SMT_OK && cls && !lastdisp && smt_scratch_alloc((void **)&last1, N * 4, st) != hipSuccess) { last1 = nullptr; rc = SMT_ERR_ALLOC; }
    if (rc == SMT_OK && lastdisp && !cls && smt_scratch_alloc((void **)&cls1, N, st) != hipSuccess) { cls1 = nullptr; rc = SMT_ERR_ALLOC; }
    if (rc == SMT_OK)
        rc = smt_lrncc_enqueue(form, grayL, grayR, pairs, H, W, D, win, sumL, rootL, sumR, rootR, dl, dr, nullptr, nullptr, st);
    if (rc == SMT_OK && (lastdisp || cls))
        for (int b = 0; b < pairs && rc == SMT_OK; b++)                       // Sad.h:184-222 on the call's own maps
            rc = smt_sad_crosscheck(dl + b * N, dr + b * N, H, W, lastdisp ? lastdisp + b * N : last1, cls ? cls + b * N : cls1,
                                    (void *)st);
    if (cls1) smt_scratch_free(cls1, st);
    if (last1) smt_scratch_free(last1, st);
    if (!dispR && dr) smt_scratch_free(dr, st);
    if (!dispL && dl) smt_scratch_free(dl, st);
    return rc;
}
