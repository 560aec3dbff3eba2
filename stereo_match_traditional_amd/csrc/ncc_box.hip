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

constexpr int NBT = 256;                 // four waves per workgroup
constexpr int NBS = 16;                  // columns per wave: C[NBS][KT] running box sums in VGPRs
constexpr int NBSW = NBS * (NBT / 64);   // columns per workgroup (the strip width)

// Staged row geometry, shared by the kernel and its host restatement.  A row of either image sits in LDS expanded to one
// dword per BYTE offset (entry A = bytes A .. A + 3, as k_sad_box stages its rows): the initial window sum of a row
// reads aligned dwords for v_dot4 whatever the hypothesis, the sliding sum reads the low byte of an entry, and lanes with
// consecutive d read consecutive dwords (one bank each; the left entry is one address for the wave, a broadcast).  Left
// entries start at column x0, right entries at x0 - 64 KT.  Columns outside the image are clamped into the row by
// box_load8, for the entering and the leaving row alike: a hypothesis that reads them (x - d < 0) keeps consistent
// running sums and costs 255.0 whatever they hold.
__host__ __device__ inline int nbox_lwe(int side) { return (NBSW + side + 3) & ~3; }
__host__ __device__ inline int nbox_rwe(int side, int KT) { return (64 * KT + NBSW + side + 3) & ~3; }

// grid (strips of NBSW window columns, bands of `band` window rows, pairs).  Step t of a band that starts at window row
// i0 brings in image row i0 + t, takes out image row i0 + t - side (once there is one) and, from t = side - 1 on, emits
// window row i0 + t - side + 1, i.e. image row i0 + t - side + 1 + win.  The two rows of step t + 1 are fetched into
// registers before step t computes and written to the other half of the LDS row buffer after it; one barrier per step.
//
// PUB (the both-view call, csrc/ncc_both.hip): every real, non-NaN cost of (x, d) is also offered to right pixel x - d as
// a rank key (csrc/ncc_keys.h).  The workgroup's 64 columns times 64 KT hypotheses reach 64 KT + 64 right pixels of a
// row; the offers of one step are combined by 64-bit LDS maxima in one of two key rows, and the step after it sends one
// agent-scope maximum per touched pixel to rkeys ([pairs][H][W], zero before the launch) and clears the row -- behind
// the step's own barrier, so no barrier is added.
template <int KT, bool PUB>
__global__ void __launch_bounds__(NBT) k_ncc_box(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int H, int W,
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
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * NBSW, i0 = blockIdx.y * band;
    const int i1 = i0 + band < Hi ? i0 + band : Hi;
    const int nk = (D + 63) >> 6;                              // live hypothesis slots (uniform)
    const int LWE = nbox_lwe(side), RWE = nbox_rwe(side, KT), ROWE = LWE + RWE;
    const int xLb = x0, xRb = x0 - 64 * KT;
    unsigned *s_rows = s_nbox;                                 // [2 halves][entering, leaving][LWE left + RWE right entries]

    // staging: one item = four consecutive entries (two unaligned dword loads, three v_alignbyte, one 16-byte store).
    // Items of a step: entering row left, entering row right, leaving row left, leaving row right; at most 2 per thread.
    const int nL4 = LWE >> 2, nR4 = RWE >> 2, nrow4 = nL4 + nR4;
    unsigned slo[2], shi[2];
    auto fetch = [&](int t) {
        const int rE = i0 + t, rL = rE - side;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * NBT;
            slo[q] = shi[q] = 0;
            if (e < 2 * nrow4) {
                const int which = e >= nrow4, f = e - which * nrow4;
                const int r = which ? rL : rE;
                if (!which || rL >= i0) {
                    const bool right = f >= nL4;
                    const int x = right ? xRb + 4 * (f - nL4) : xLb + 4 * f;
                    box_load8((right ? R : L) + (size_t)r * W, x, W, slo[q], shi[q]);
                }
            }
        }
    };
    auto commit = [&](int half) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * NBT;
            if (e < 2 * nrow4)
                *reinterpret_cast<u4v *>(s_rows + (size_t)half * 2 * ROWE + 4 * e) =
                    u4v{slo[q], __builtin_amdgcn_alignbyte(shi[q], slo[q], 1), __builtin_amdgcn_alignbyte(shi[q], slo[q], 2),
                        __builtin_amdgcn_alignbyte(shi[q], slo[q], 3)};
        }
    };
    // PUB: [2][NKE] keys behind the staged rows; entry e of a row is right window column x0 - 64 KT + e
    constexpr int NKE = 64 * KT + NBSW;
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(s_nbox + 4 * ROWE);
    auto flush = [&](int half, int io) {                       // the keys of window row io go out, the row is cleared
        for (int e = threadIdx.x; e < NKE; e += NBT) {
            const unsigned long long v = s_keys[half * NKE + e];
            if (v) {
                atomicMax(rkeys + (size_t)(io + win) * W + win + (x0 - 64 * KT + e), v);
                s_keys[half * NKE + e] = 0ull;
            }
        }
    };
    if constexpr (PUB)
        for (int e = threadIdx.x; e < 2 * NKE; e += NBT) s_keys[e] = 0ull;
    fetch(0);
    commit(0);
    __syncthreads();

    const int xw = x0 + NBS * wv;                              // this wave's first window column
    const bool live = xw < Wi;
    const int nfull = side >> 2, rem = side & 3;
    const unsigned hmask = (1u << (8 * rem)) - 1u;             // the window's last rem columns: the low bytes of one more dword
    const int la = xw - xLb;                                   // left entry of column xw
    int ra[KT];                                                // right entry of column xw - d
    unsigned C[NBS][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        ra[k] = xw - xRb - (lane + 64 * k);
#pragma unroll
        for (int j = 0; j < NBS; j++) C[j][k] = 0;
    }
    // horizontal window sums of one staged row over the wave's NBS columns, added to (SUB = false) or taken from C
    auto row_pass = [&](const unsigned *Lrow, const unsigned *Rrow, auto sub) {
        constexpr bool SUB = decltype(sub)::value;
        unsigned run[KT];
#pragma unroll
        for (int k = 0; k < KT; k++) run[k] = 0;
        for (int g = 0; g < nfull; g++) {
            const unsigned a4 = Lrow[la + 4 * g];
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = __builtin_amdgcn_udot4(a4, Rrow[ra[k] + 4 * g], run[k], false);
        }
        if (rem) {
            const unsigned a4 = Lrow[la + 4 * nfull] & hmask;  // a zero byte on the left takes the right one out of the sum
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = __builtin_amdgcn_udot4(a4, Rrow[ra[k] + 4 * nfull], run[k], false);
        }
        const uint8_t *Lb = reinterpret_cast<const uint8_t *>(Lrow), *Rb = reinterpret_cast<const uint8_t *>(Rrow);
#pragma unroll
        for (int j = 0; j < NBS; j++) {
            if (j > 0) {
                const unsigned aN = Lb[4 * (la + j - 1 + side)], aO = Lb[4 * (la + j - 1)];
#pragma unroll
                for (int k = 0; k < KT; k++)
                    if (k < nk) {
                        const unsigned bN = Rb[4 * (ra[k] + j - 1 + side)], bO = Rb[4 * (ra[k] + j - 1)];
                        // one byte per operand: two single products, through the intrinsic on purpose.  Written as plain
                        // multiplies, the compiler (ROCm 7.2) folds the products of neighbouring columns into v_dot4 of
                        // v_perm-packed bytes, and in the KT = 1 instantiation the packed operands take in a leaving pair
                        // (aO, bO), whose product is then added instead of subtracted (tools/dot4_fold_probe.hip)
                        run[k] = __builtin_amdgcn_udot4(aN, bN, run[k], false) - __builtin_amdgcn_udot4(aO, bO, 0u, false);
                    }
            }
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) C[j][k] = SUB ? C[j][k] - run[k] : C[j][k] + run[k];
        }
    };

    const double n = (double)(side * side);
    const int nsteps = side - 1 + (i1 - i0);
    for (int t = 0; t < nsteps; t++) {
        const int half = t & 1;
        const int io = i0 + t - side + 1;                      // window row of this step (>= i0: there is one)
        const bool leaving = t >= side;
        if (t + 1 < nsteps) fetch(t + 1);
        if constexpr (PUB)
            if (io > i0) flush(half ^ 1, io - 1);              // what step t - 1 emitted
        if (live) {
            const unsigned *rows = s_rows + (size_t)half * 2 * ROWE;
            row_pass(rows, rows + LWE, std::false_type());
            if (leaving) row_pass(rows + ROWE, rows + ROWE + LWE, std::true_type());
            if (io >= i0) {
#pragma unroll
                for (int j = 0; j < NBS; j++) {
                    const int x = xw + j;
                    if (x >= Wi) break;
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
                            c[k] = ncc_int_cost(n, C[j][k], sa, rta, sumR[q], rootR[q]);
                        } else c[k] = 255.0;                   // `invalid` 0xff, NCC.h:88
                        if (cost_out && act) cost_out[p * D + d] = c[k];
                        if constexpr (PUB)
                            if (act && x - d >= 0 && c[k] == c[k])
                                atomicMax(s_keys + half * NKE + (x - d - (x0 - 64 * KT)), ncc_rank_key(c[k], d));
                        if (k == 0) poison = __ballot(c[0] != c[0] && lane == 0) != 0;   // d = 0 is slot 0 of lane 0
                        v[k] = ncc_wta_term(c[k], act);
                    }
                    // WinTakeAll in d order = (slot, lane): before (k, lane) = max(every lane of the slots < k, the
                    // lanes below `lane` of slot k)
                    float below = -INFINITY;
                    unsigned key = 0;                          // 1 + the largest winning d of the lane (0: none)
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
                }
            }
        }
        if (t + 1 < nsteps) commit(half ^ 1);
        __syncthreads();
    }
    if constexpr (PUB) flush((nsteps - 1) & 1, i1 - 1);        // the last step's row (i1 > i0: it emitted)
}

int g_ncc_box_band = 0;        // test hook: window rows per band, 0 = box_band's choice

int nbox_band(int Hi, int Wi, int side)
{
    return g_ncc_box_band > 0 ? (g_ncc_box_band < Hi ? g_ncc_box_band : Hi) : box_band(Hi, Wi, side, NBSW);
}

template <int KT>
int launch_nbox(hipStream_t st, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int win, const int *sumL,
                const double *rootL, const int *sumR, const double *rootR, int32_t *disp, double *cost,
                unsigned long long *rkeys)
{
    const int side = 2 * win + 1, Hi = H - 2 * win, Wi = W - 2 * win, band = nbox_band(Hi, Wi, side);
    const size_t shm = (size_t)4 * (nbox_lwe(side) + nbox_rwe(side, KT)) * 4;   // <= 16 KiB; two staging items per thread suffice
    static_assert(2 * (((NBSW + NCC_INT_MAX_SIDE + 3) & ~3) + ((64 * KT + NBSW + NCC_INT_MAX_SIDE + 3) & ~3)) / 4 <= 2 * NBT, "staging items");
    const dim3 grid((Wi + NBSW - 1) / NBSW, (Hi + band - 1) / band, pairs);
    if (rkeys)                                                 // + the two key rows, at most 9 KiB
        hipLaunchKernelGGL((k_ncc_box<KT, true>), grid, dim3(NBT), shm + (size_t)2 * (64 * KT + NBSW) * 8, st, L, R, H, W, D, win, band,
                           sumL, rootL, sumR, rootR, disp, cost, rkeys);
    else
        hipLaunchKernelGGL((k_ncc_box<KT, false>), grid, dim3(NBT), shm, st, L, R, H, W, D, win, band, sumL, rootL, sumR, rootR, disp,
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
    const int K = (D + 63) / 64;
    int rc;
    if (K <= 1) rc = launch_nbox<1>(st, L, R, pairs, H, W, D, winSize, sumL, rootL, sumR, rootR, disp, cost, rkeys);
    else if (K <= 2) rc = launch_nbox<2>(st, L, R, pairs, H, W, D, winSize, sumL, rootL, sumR, rootR, disp, cost, rkeys);
    else if (K <= 4) rc = launch_nbox<4>(st, L, R, pairs, H, W, D, winSize, sumL, rootL, sumR, rootR, disp, cost, rkeys);
    else rc = launch_nbox<8>(st, L, R, pairs, H, W, D, winSize, sumL, rootL, sumR, rootR, disp, cost, rkeys);
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
namespace {

unsigned host_dot4(unsigned a, unsigned b, unsigned acc)
{
    for (int q = 0; q < 4; q++) acc += ((a >> (8 * q)) & 255u) * ((b >> (8 * q)) & 255u);
    return acc;
}

// k_ncc_box on the host, hypothesis by hypothesis: the same strips, bands, steps, staged entries (clamped columns
// included), dword groups, sliding sums and entering and leaving rows, in uint32.  sab: [Hi][Wi][D].
void nbox_host(const uint8_t *L, const uint8_t *R, int H, int W, int D, int win, int band, unsigned *sab)
{
    const int side = 2 * win + 1, Hi = H - 2 * win, Wi = W - 2 * win;
    const int KT = D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : 8;
    const int LWE = nbox_lwe(side), RWE = nbox_rwe(side, KT);
    const int nfull = side >> 2, rem = side & 3;
    const unsigned hmask = (1u << (8 * rem)) - 1u;
    std::vector<unsigned> eL(LWE), eR(RWE), lL(LWE), lR(RWE), C((size_t)NBS * 64 * KT);
    auto stage = [&](std::vector<unsigned> &dst, const uint8_t *row, int xb) {
        for (size_t e = 0; e < dst.size(); e++) {
            unsigned v = 0;
            for (int b = 0; b < 4; b++) {
                int x = xb + (int)e + b;
                x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
                v |= (unsigned)row[x] << (8 * b);
            }
            dst[e] = v;
        }
    };
    for (int i0 = 0; i0 < Hi; i0 += band) {
        const int i1 = i0 + band < Hi ? i0 + band : Hi;
        for (int x0 = 0; x0 < Wi; x0 += NBSW) {
            const int xLb = x0, xRb = x0 - 64 * KT;
            for (int xw = x0; xw < x0 + NBSW && xw < Wi; xw += NBS) {
                std::fill(C.begin(), C.end(), 0u);
                const int la = xw - xLb;
                const int nsteps = side - 1 + (i1 - i0);
                for (int t = 0; t < nsteps; t++) {
                    const int rE = i0 + t, rL = rE - side, io = rE - side + 1;
                    stage(eL, L + (size_t)rE * W, xLb);
                    stage(eR, R + (size_t)rE * W, xRb);
                    if (rL >= i0) { stage(lL, L + (size_t)rL * W, xLb); stage(lR, R + (size_t)rL * W, xRb); }
                    for (int d = 0; d < D; d++) {
                        const int ra = xw - xRb - d;
                        for (int pass = 0; pass < (rL >= i0 ? 2 : 1); pass++) {
                            const unsigned *Lrow = pass ? lL.data() : eL.data(), *Rrow = pass ? lR.data() : eR.data();
                            unsigned run = 0;
                            for (int g = 0; g < nfull; g++) run = host_dot4(Lrow[la + 4 * g], Rrow[ra + 4 * g], run);
                            if (rem) run = host_dot4(Lrow[la + 4 * nfull] & hmask, Rrow[ra + 4 * nfull], run);
                            for (int j = 0; j < NBS; j++) {
                                if (j > 0)
                                    run = run + (Lrow[la + j - 1 + side] & 255u) * (Rrow[ra + j - 1 + side] & 255u) -
                                          (Lrow[la + j - 1] & 255u) * (Rrow[ra + j - 1] & 255u);
                                unsigned &c = C[(size_t)j * 64 * KT + d];
                                c = pass ? c - run : c + run;
                            }
                        }
                    }
                    if (io < i0) continue;
                    for (int j = 0; j < NBS && xw + j < Wi; j++)
                        for (int d = 0; d < D; d++)
                            sab[((size_t)io * Wi + xw + j) * D + d] = C[(size_t)j * 64 * KT + d];
                }
            }
        }
    }
}

}  // namespace

// Host only (no GPU).  On four unpadded pairs of the given shape -- pseudo-random, 255 against 255 (the largest sums),
// opposed checkerboards, a shifted copy -- the restated recurrence of k_ncc_box (nbox_host, under the band the launch
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
        const int bands[3] = {box_band(Hi, Wi, side, NBSW), 1, 3};
        for (int b = 0; b < 3; b++) {
            std::fill(got.begin(), got.end(), 0xdeadbeefu);
            nbox_host(L.data(), R.data(), H, W, D, win, bands[b] < Hi ? bands[b] : Hi, got.data());
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
