// costAggregationV4 (CBLSM/CBLSM.h:1128-1176), the consumer of the per-hypothesis arm volumes of
// chooseArmLength{Left,Right,Up,Down} (:65-236), in two forms.
//
// Literal (smt_cblsm_cost_aggregation_v4): any float volume, any four [H][W][D] int arm volumes.  One thread per
// (pixel, d) walks rows [-up, down) outer and columns [-L, R) inner with sequential float adds and divides by the int
// tap count; an empty rectangle is 0.0f / 0 = NaN.  Adjacent lanes hold adjacent d, so every tap row is one coalesced
// read while the lanes' rectangles agree.  ComputeDispOringin (:383-407) is smt_wta on the result.
//
// Fused (smt_cblsm_v4_box_enqueue, the core of smt_cblsm_flow_run_batch_v4): the volume is ComputeAD's, every entry an
// integer 0..255, and the arm volumes are functions of the eight [H][W] arm maps (cblsm_v4_rules.h), so neither is
// materialised.  With arm bound m a rectangle has at most (2m)^2 taps, every partial sum of the reference's float loop
// is an integer <= 255 (2m)^2 <= 16 451 580 < 2^24 for m <= 127: each add is exact and the result is exactly
// (float)S / (float)n with S the integer rectangle sum, read from the flow's uint32 summed-area table in four corners
// (mod 2^32, as in cblsm.hip).  One wave per pixel; lane l owns the C = ceil(D / 64) hypotheses l*C .. l*C+C-1, so its
// corner reads are C consecutive words and the wave's are contiguous.  Left and right arms are closed forms in d; the
// up and down walks read the right image's horizontal arms of column j row by row -- wave-uniform loads shared by all
// hypotheses -- and each lane counts its own hits.  The WTA is wave_wta on the quotients the wave already holds.
#include "smt_common.h"
#include "cblsm_v4_rules.h"
#include <limits.h>
#include <new>
#include <string.h>

namespace {

constexpr int NT = 256;   // four waves per workgroup

__global__ void __launch_bounds__(NT) k_v4_literal(const float *__restrict__ vin, const int *__restrict__ aL,
                                                   const int *__restrict__ aR, const int *__restrict__ aUp,
                                                   const int *__restrict__ aDown, int H, int W, int D,
                                                   float *__restrict__ vout, int *ub_flag)
{
    const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
    if (k >= (size_t)H * W * D) return;
    const int d = (int)(k % D);
    const size_t p = k / D;
    const int j = (int)(p % W), i = (int)(p / W);
    // top in [t0, t1), left in [l0, l1); 64-bit so that no arm value overflows the bounds
    long long t0 = -(long long)aUp[k], t1 = aDown[k], l0 = -(long long)aL[k], l1 = aR[k];
    if (t1 > t0 && l1 > l0) {
        // a tap outside the plane is an out-of-bounds (or wrapped) read in the reference: flagged, and the walk is
        // clipped to the plane
        const bool ub = i + t0 < 0 || i + t1 > H || j + l0 < 0 || j + l1 > W;
        if (ub) {
            if (ub_flag) atomicOr(ub_flag, 1);
            t0 = t0 < -i ? -i : t0; t1 = t1 > H - i ? H - i : t1;
            l0 = l0 < -j ? -j : l0; l1 = l1 > W - j ? W - j : l1;
        }
    }
    float value = 0.0f;
    int number = 0;
    if (t1 > t0 && l1 > l0) {
        for (int top = (int)t0; top < (int)t1; top++) {
            const float *row = vin + ((size_t)(i + top) * W + j) * D + d;
            for (int left = (int)l0; left < (int)l1; left++) value = value + row[(ptrdiff_t)left * D];
        }
        number = (int)((t1 - t0) * (l1 - l0));
    }
    vout[k] = value / (float)number;
}

template <int C>
__global__ void __launch_bounds__(NT) k_v4_box(const uint32_t *__restrict__ S, const int *__restrict__ LL,
                                               const int *__restrict__ LR, const int *__restrict__ LUp,
                                               const int *__restrict__ LDown, const int *__restrict__ RL,
                                               const int *__restrict__ RR, const int *__restrict__ RUp,
                                               const int *__restrict__ RDown, int H, int W, int D,
                                               float *__restrict__ vol, float *__restrict__ disp, int *err)
{
    const int p = blockIdx.x * (NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= H * W) return;
    const int lane = threadIdx.x & 63, dl = lane * C;
    const int i = p / W, j = p - i * W;
    const int ll = LL[p], lr = LR[p], rl = RL[p], rr = RR[p];
    bool clip = false;
    // the walks stay inside the plane for arms the arm kernels compute; anything else is cut there and reported
    int nu = v4rule::up_rows(LUp[p], RUp[p]), nd = v4rule::down_rows(LDown[p], RDown[p]);
    if (nu > i) { nu = i; clip = true; }
    if (nd > H - 1 - i) { nd = H - 1 - i; clip = true; }
    int up[C], dn[C];
#pragma unroll
    for (int k = 0; k < C; k++) up[k] = dn[k] = 0;
    for (int t = 1; t <= nu; t++) {
        const int a = RL[p - t * W], b = RR[p - t * W];
#pragma unroll
        for (int k = 0; k < C; k++) up[k] += v4rule::up_hit(dl + k, a, b);
    }
    for (int t = 1; t <= nd; t++) {
        const int a = RL[p + t * W], b = RR[p + t * W];
#pragma unroll
        for (int k = 0; k < C; k++) dn[k] += v4rule::down_hit(dl + k, a, b);
    }
    float q[C];
#pragma unroll
    for (int k = 0; k < C; k++) {
        const int d = dl + k;
        q[k] = 0.0f;
        if (d < D) {
            const bool before = j - d < 0;                      // CBLSM.h:171, :215
            int c[4], n;
            if (v4rule::box(i, j, v4rule::arm_left(ll, rl, rr, d), v4rule::arm_right(lr, rl, rr, d), before ? 0 : up[k],
                            before ? 0 : dn[k], H, W, c, n))
                clip = true;
            const uint32_t s = n ? v4rule::box_sum(S, (size_t)D, c, d) : 0u;
            q[k] = (float)s / (float)n;                         // n == 0: 0.0f / 0 = NaN, as the reference
            if (vol) vol[(size_t)p * D + d] = q[k];
        }
    }
    const int wd = wave_wta<C, false>(q, dl, D);
    if (lane == 0) disp[p] = (float)wd;
    if (__ballot(clip) != 0 && lane == 0) atomicOr(err, 1);
}

}  // namespace

int smt_cblsm_v4_box_enqueue(const uint32_t *S, int *const armL[4], int *const armR[4], int H, int W, int D, float *vol,
                             float *disp, int *err_dev, hipStream_t st)
{
    const dim3 grid((unsigned)(((long long)H * W + 3) / 4));
#define SMT_V4(CC)                                                                                                    \
    hipLaunchKernelGGL((k_v4_box<CC>), grid, dim3(NT), 0, st, S, armL[0], armL[1], armL[2], armL[3], armR[0], armR[1], \
                       armR[2], armR[3], H, W, D, vol, disp, err_dev)
    switch ((D + 63) / 64) {
    case 1: SMT_V4(1); break;
    case 2: SMT_V4(2); break;
    case 3: SMT_V4(3); break;
    case 4: SMT_V4(4); break;
    case 5: SMT_V4(5); break;
    case 6: SMT_V4(6); break;
    case 7: SMT_V4(7); break;
    default: SMT_V4(8); break;
    }
#undef SMT_V4
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_cblsm_cost_aggregation_v4(const float *vol_in, const int *armvolL, const int *armvolR,
                                          const int *armvolUp, const int *armvolDown, int H, int W, int D,
                                          float *vol_out, float *disp, int *ub_flag, void *stream)
{
    if (!vol_in || !armvolL || !armvolR || !armvolUp || !armvolDown || !vol_out || vol_in == vol_out || H <= 0 ||
        W <= 0 || D <= 0 || (disp && D > SMT_MAX_DISPARITY))
        return SMT_ERR_ARG;
    const size_t V = (size_t)H * W * D;
    if ((size_t)H * W > (size_t)INT_MAX || (V + NT - 1) / NT > (size_t)INT_MAX) return SMT_ERR_ARG;   // int tap counts, grid size
    hipLaunchKernelGGL(k_v4_literal, dim3((unsigned)((V + NT - 1) / NT)), dim3(NT), 0, smt_stream(stream), vol_in, armvolL,
                       armvolR, armvolUp, armvolDown, H, W, D, vol_out, ub_flag);
    SMT_LAUNCH_CHECK();
    return disp ? smt_wta(vol_out, H, W, D, disp, stream) : SMT_OK;          // ComputeDispOringin, CBLSM.h:383-407
}

// Host only (no GPU).  Eight random arm maps (zeros, arms at their bound max_arm or the border, anything between;
// the left image's stay inside the plane as the arm kernels guarantee):
//  * the rules of cblsm_v4_rules.h against the loops of CBLSM.h:65-236 as written, for every (pixel, d);
//  * the half-open box against costAggregationV4's walk on an AD-like uint8 volume and a uint32 summed-area table built
//    as the kernels build it: tap count, four-corner sum against the direct integer sum, (float)S / (float)n against
//    the sequential float sum over the int count bit for bit, NaN for NaN where the rectangle is empty; and a
//    rectangle pushed past column 0 must be reported and clipped.
SMT_API int smt_cblsm_selftest_v4(int H, int W, int D, int max_arm, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || max_arm < 0 || max_arm > 255 || (long long)H * W * D > (1ll << 22)) return SMT_ERR_ARG;
    const size_t N = (size_t)H * W;
    int *arm = new (std::nothrow) int[N * 8];          // LL LR LUp LDown RL RR RUp RDown, one plane each
    uint8_t *ad = new (std::nothrow) uint8_t[N * D];
    uint32_t *S = new (std::nothrow) uint32_t[N * D];
    if (!arm || !ad || !S) { delete[] arm; delete[] ad; delete[] S; return SMT_ERR_ALLOC; }
    uint32_t st = seed;
    auto rnd = [&st]() { st = st * 1664525u + 1013904223u; return st >> 8; };
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const int lim[4] = {j, W - 1 - j, i, H - 1 - i};
            for (int q = 0; q < 8; q++) {
                const int m = lim[q & 3] < max_arm ? lim[q & 3] : max_arm;
                const uint32_t kind = rnd() % 5;
                arm[q * N + (size_t)i * W + j] = kind == 0 ? 0 : kind == 1 ? m : (int)(rnd() % (uint32_t)(m + 1));
            }
        }
    const int *LL = arm, *LR = arm + N, *LUp = arm + 2 * N, *LDown = arm + 3 * N;
    const int *RL = arm + 4 * N, *RR = arm + 5 * N, *RUp = arm + 6 * N, *RDown = arm + 7 * N;
    for (size_t k = 0; k < N * D; k++) ad[k] = (uint8_t)(rnd() & 255);
    // the kernels' order: column prefix, then row prefix, mod 2^32
    for (size_t k = 0; k < N * D; k++) S[k] = ad[k];
    for (int i = 1; i < H; i++)
        for (size_t k = 0; k < (size_t)W * D; k++) S[(size_t)i * W * D + k] += S[(size_t)(i - 1) * W * D + k];
    for (int i = 0; i < H; i++)
        for (int j = 1; j < W; j++)
            for (int d = 0; d < D; d++) S[((size_t)i * W + j) * D + d] += S[((size_t)i * W + j - 1) * D + d];

    // the reference's four loops for one (i, j, d), conditions in the reference's order
    auto ref_arms = [&](int i, int j, int d, int (&out)[4]) {
        const size_t p = (size_t)i * W + j;
        int save = 0;
        if (!((j - d < j - RL[p]) || (j + d > j + RR[p])))                                   // :77
            for (int a = 1; a <= LL[p]; a++) {
                if (((j - a - d) >= (j - RL[p])) && ((j - a - d) <= (j + RR[p]))) save++;    // :88
                else break;
            }
        out[0] = save; save = 0;
        if (!((j - d < j - RL[p]) || (j - d > j + RR[p])))                                   // :123
            for (int a = 1; a <= LR[p]; a++) {
                if ((j + a - d >= j - RL[p]) && (j + a - d < j + RR[p])) save++;             // :134
                else break;
            }
        out[1] = save; save = 0;
        for (int up = 1; up <= LUp[p]; up++) {                                               // :164-185
            const int pr = i - up;
            const int pl = RL[(size_t)pr * W + j], prr = RR[(size_t)pr * W + j];
            if (pr >= i - RUp[p]) {
                if (j - d < 0) break;
                if (((j - d) < (j + prr)) && ((j - d) > (j - pl))) save++;
            } else { save = 0; break; }
        }
        out[2] = save; save = 0;
        for (int dn = 1; dn <= LDown[p]; dn++) {                                             // :208-229
            const int pr = i + dn;
            const int pl = RL[(size_t)pr * W + j], prr = RR[(size_t)pr * W + j];
            if (pr <= i + RDown[p]) {
                if (j - d < 0) { save = 0; break; }
                if ((j - d <= j + prr) && (j - d >= j - pl)) save++;
            } else break;
        }
        out[3] = save;
    };

    const double area = (double)(2 * max_arm) * (2 * max_arm);
    const size_t step = 1 + (size_t)((double)N * D * (area < (double)N ? area : (double)N) / (double)(1 << 25));
    int rc = SMT_OK;
    for (size_t p = 0; p < N && rc == SMT_OK; p++) {
        const int i = (int)(p / W), j = (int)(p % W);
        for (int d = 0; d < D && rc == SMT_OK; d++) {
            int ref[4];
            ref_arms(i, j, d, ref);
            const int got[4] = {v4rule::arm_left(LL[p], RL[p], RR[p], d), v4rule::arm_right(LR[p], RL[p], RR[p], d),
                                v4rule::arm_up(LUp[p], RUp[p], RL + p, RR + p, W, j, d),
                                v4rule::arm_down(LDown[p], RDown[p], RL + p, RR + p, W, j, d)};
            if (memcmp(ref, got, sizeof ref) != 0) { rc = SMT_ERR_STATE; break; }
            if ((p * D + d) % step != 0) continue;
            // costAggregationV4's walk (:1160-1170)
            const int L = ref[0], R = ref[1], up = ref[2], down = ref[3];
            float value = 0;
            int number = 0;
            uint64_t direct = 0;
            for (int top = -up; top < down; top++)
                for (int left = -L; left < R; left++) {
                    const uint8_t v = ad[((size_t)(i + top) * W + j + left) * D + d];
                    value = value + (float)v;
                    direct += v;
                    number++;
                }
            value = value / number;
            int c[4], n;
            if (v4rule::box(i, j, L, R, up, down, H, W, c, n) || n != number) { rc = SMT_ERR_STATE; break; }
            const uint32_t s = n ? v4rule::box_sum(S, (size_t)D, c, d) : 0u;
            if ((uint64_t)s != direct) { rc = SMT_ERR_STATE; break; }
            const float q = (float)s / (float)n;
            if (n == 0 ? !(q != q && value != value) : (direct < (1u << 24) && memcmp(&q, &value, 4) != 0)) { rc = SMT_ERR_STATE; break; }
            if (n) {                                   // the same rectangle pushed one column past the left border
                const int cols = j + R;                // columns [0, j + R) remain
                uint64_t dc = 0;
                for (int top = -up; top < down; top++)
                    for (int x = 0; x < cols; x++) dc += ad[((size_t)(i + top) * W + x) * D + d];
                if (!v4rule::box(i, j, j + 1, R, up, down, H, W, c, n) || n != (up + down) * cols ||
                    (uint64_t)(n ? v4rule::box_sum(S, (size_t)D, c, d) : 0u) != dc)
                    rc = SMT_ERR_STATE;
            }
        }
    }
    delete[] arm; delete[] ad; delete[] S;
    return rc;
}
