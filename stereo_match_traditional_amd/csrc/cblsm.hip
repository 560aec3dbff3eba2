// CBLSM/CBLSM.cpp's active flow (:64-67, 101-104, 133-134, 146-153) as one batched entry point: arms of both images,
// the first costAggregationV5 pass of each view, the second pass of each view on the LEFT arms (:150) with the WTA
// (ComputeDispOringin, :152-153) fused.  Like csrc/pipeline.hip it sequences the library's own entry points and owns
// the buffers between them, so a batch of pairs reuses three [H][W][D] buffers whatever its size: the two first-pass
// volumes and one scratch that holds the summed-area table of each first pass and then each second-pass output.
//
// First pass without the AD volume.  The first pass of each view aggregates ComputeAD / ComputeADRight
// (CBLSM.h:327-381): every entry is an integer 0..255.  An arm is at most m = max(sec_length, max_length) long (the
// walk stops at an offset past both), so a rectangle has at most (2m+1)^2 taps and every partial sum of the
// reference's float loop (CBLSM.h:1210-1216) is an integer <= 255 (2m+1)^2, which for m <= 127 is <= 16 581 375 < 2^24:
// every float add of that loop is exact, and its result is exactly (float)S / (float)n with S the integer rectangle
// sum and n = (up+down+1)(L+R+1).  crossarm.hip's sequential walk is O(area) per hypothesis (up to 69 x 69 taps at
// max_length 34); here S comes from a uint32 summed-area table in O(1), bit-identical:
//   k_sat_cols  one wave per (column, 64 hypotheses): walks the rows, AD from the two images, writes the column prefix;
//   k_sat_rows  one wave per (row, 64 hypotheses): walks the columns, turns it into the summed-area table in place;
//   k_sat_box   one wave per pixel: the four corners of its rectangle, the quotient -> the float first-pass volume.
// Unsigned wrap-around in the table is harmless: the four-corner difference is the rectangle's sum modulo 2^32, and
// that sum is below 2^24.  For m > 127 the argument fails and the handle materialises AD (smt_cblsm_ad) into the
// scratch and runs smt_crossarm_aggregate(order 1) instead; the choice follows from the parameters alone.  The second
// pass aggregates float quotients, whose sums round, so it stays crossarm.hip's in-order walk.
#include "smt_common.h"
#include <limits.h>
#include <math.h>
#include <new>
#include <stdlib.h>
#include <string.h>

// The rectangle [i-u, i+dn] x [j-l, j+r] of pixel (i, j) as corners of a summed-area table S (S[p] = sum over rows
// <= p's row and columns <= p's column): sum = S[c0] - S[c1] - S[c2] + S[c3], c = pixel index, or -1 for a row or
// column before the image (contributes 0); n = its tap count.  Arms that would leave the plane (or are negative) are
// clipped to it and the function returns true -- never the case for arms the crossarm kernels compute, which stop at
// the border.  Shared by k_sat_box and the host self-test.
__host__ __device__ inline bool cblsm_box(int i, int j, int l, int r, int u, int dn, int H, int W, int (&c)[4], int &n)
{
    bool clip = l < 0 || r < 0 || u < 0 || dn < 0;
    l = l < 0 ? 0 : l; r = r < 0 ? 0 : r; u = u < 0 ? 0 : u; dn = dn < 0 ? 0 : dn;
    clip = clip || i - u < 0 || i + dn > H - 1 || j - l < 0 || j + r > W - 1;
    const int r1 = i + dn > H - 1 ? H - 1 : i + dn, r0 = (i - u < 0 ? 0 : i - u) - 1;
    const int c1 = j + r > W - 1 ? W - 1 : j + r, c0 = (j - l < 0 ? 0 : j - l) - 1;
    c[0] = r1 * W + c1;
    c[1] = r0 >= 0 ? r0 * W + c1 : -1;
    c[2] = c0 >= 0 ? r1 * W + c0 : -1;
    c[3] = (r0 >= 0 && c0 >= 0) ? r0 * W + c0 : -1;
    n = (r1 - r0) * (c1 - c0);
    return clip;
}

// hypothesis d of the rectangle whose corners cblsm_box gave, in uint32 (mod 2^32) arithmetic
__host__ __device__ inline uint32_t cblsm_box_sum(const uint32_t *S, size_t D, const int (&c)[4], int d)
{
    uint32_t s = S[(size_t)c[0] * D + d];
    if (c[1] >= 0) s -= S[(size_t)c[1] * D + d];
    if (c[2] >= 0) s -= S[(size_t)c[2] * D + d];
    if (c[3] >= 0) s += S[(size_t)c[3] * D + d];
    return s;
}

// the largest arm length the handle's arms can reach, and whether the summed-area first pass is exact for it
static inline int cblsm_arm_bound(const smt_cblsm_params &p) { return p.sec_length > p.max_length ? p.sec_length : p.max_length; }
static inline bool cblsm_sat_exact(const smt_cblsm_params &p) { return cblsm_arm_bound(p) <= 127; }

namespace {

constexpr int NT = 256;   // four waves per workgroup
constexpr int CBLSM_WINDOW_MAX_W = 90;   // winSize + 1 of the widest window smt_cblsm_window_cost_batch takes (side 181)
constexpr int SU = 8;     // rows / columns whose loads are issued before their adds

// Column prefix of the AD volume of one view, AD evaluated from the two images: view 0 |L[i][j] - R[i][max(j-d, 0)]|
// (ComputeAD, CBLSM.h:340-349: the copy from d-1 at j < d is the clamp), view 1 |R[i][j] - L[i][min(j+d, W-1)]|
// (ComputeADRight, :368-377).  S[i][j][d] = sum of rows 0..i.
template <int VIEW>
__global__ void __launch_bounds__(NT) k_sat_cols(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int H, int W,
                                                 int D, int nck, uint32_t *__restrict__ S)
{
    const int w = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (w >= W * nck) return;
    const int j = w / nck, d = (w - j * nck) * 64 + (threadIdx.x & 63);
    if (d >= D) return;
    const int x = VIEW == 0 ? (j - d < 0 ? 0 : j - d) : (j + d > W - 1 ? W - 1 : j + d);
    const uint8_t *own = VIEW == 0 ? L : R, *oth = VIEW == 0 ? R : L;
    const size_t rs = (size_t)W * D;
    uint32_t *dst = S + (size_t)j * D + d;
    uint32_t acc = 0;
    int i = 0;
    for (; i + SU <= H; i += SU) {
        int a[SU], b[SU];
#pragma unroll
        for (int u = 0; u < SU; u++) {
            a[u] = own[(size_t)(i + u) * W + j];
            b[u] = oth[(size_t)(i + u) * W + x];
        }
#pragma unroll
        for (int u = 0; u < SU; u++) {
            acc += (uint32_t)abs(a[u] - b[u]);
            dst[(size_t)(i + u) * rs] = acc;
        }
    }
    for (; i < H; i++) {
        acc += (uint32_t)abs((int)own[(size_t)i * W + j] - (int)oth[(size_t)i * W + x]);
        dst[(size_t)i * rs] = acc;
    }
}

// Row prefix in place: the column prefixes become the summed-area table.
__global__ void __launch_bounds__(NT) k_sat_rows(int H, int W, int D, int nck, uint32_t *__restrict__ S)
{
    const int w = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (w >= H * nck) return;
    const int i = w / nck, d = (w - i * nck) * 64 + (threadIdx.x & 63);
    if (d >= D) return;
    uint32_t *row = S + (size_t)i * W * D + d;
    uint32_t acc = 0;
    int j = 0;
    for (; j + SU <= W; j += SU) {
        uint32_t v[SU];
#pragma unroll
        for (int u = 0; u < SU; u++) v[u] = row[(size_t)(j + u) * D];
#pragma unroll
        for (int u = 0; u < SU; u++) {
            acc += v[u];
            row[(size_t)(j + u) * D] = acc;
        }
    }
    for (; j < W; j++) {
        acc += row[(size_t)j * D];
        row[(size_t)j * D] = acc;
    }
}

// First-pass volume: rectangle sum over its tap count, correctly rounded (the reference's exact float sum over the same
// count, crossarm.hip's `acc / cnt`).
__global__ void __launch_bounds__(NT) k_sat_box(const uint32_t *__restrict__ S, const int *__restrict__ armL,
                                                const int *__restrict__ armR, const int *__restrict__ armT,
                                                const int *__restrict__ armB, int H, int W, int D,
                                                float *__restrict__ out, int *err)
{
    const int p = blockIdx.x * (NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= H * W) return;
    const int lane = threadIdx.x & 63;
    const int i = p / W, j = p - i * W;
    int c[4], n;
    const bool clip = cblsm_box(i, j, armL[p], armR[p], armT[p], armB[p], H, W, c, n);
    if (clip && lane == 0) atomicOr(err, 1);
    const float fn = (float)n;
    float *dst = out + (size_t)p * D;
    for (int d = lane; d < D; d += 64) dst[d] = (float)cblsm_box_sum(S, (size_t)D, c, d) / fn;
}

}  // namespace

struct smt_cblsm_flow {
    int device;
    int H, W, D;
    smt_cblsm_params P;
    bool sat;                 // summed-area first pass (cblsm_sat_exact), else AD materialised + order-1 walk
    hipStream_t stream;
    smt_crossarm *caL, *caR;  // arms of the left / the right image
    float *pass1[2];          // first-pass volumes of the left / right view (the last pair's after a call)
    void *scratch;            // [H][W][D] x 4 B: summed-area table (or AD volume), then each second-pass output
    int *err;                 // nonzero when k_sat_box (or the costAggregationV4 kernels) clipped a rectangle to the plane
    int *post_err;            // nonzero when a speckle kernel of run_batch_post hit its loop cap
    int *v4_arms;             // run_batch_v4 past the summed-area bound only: three [H][W][D] arm volumes, allocated on first use
    uint8_t *padL, *padR;     // run_batch_window: the images of CBLSM.cpp:124-125, room for the widest border (90)
};

SMT_API void smt_cblsm_default_params(smt_cblsm_params *p)
{
    if (!p) return;
    p->tau = 25; p->max_length = 34; p->sec_length = 17;     // CBLSM.cpp:30-32
}

SMT_API int smt_cblsm_flow_destroy(smt_cblsm_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipDeviceSynchronize();
    if (h->caL) smt_crossarm_destroy(h->caL);
    if (h->caR) smt_crossarm_destroy(h->caR);
    (void)hipFree(h->pass1[0]); (void)hipFree(h->pass1[1]);
    (void)hipFree(h->scratch); (void)hipFree(h->err); (void)hipFree(h->post_err); (void)hipFree(h->v4_arms);
    (void)hipFree(h->padL); (void)hipFree(h->padR);
    delete h;
    return SMT_OK;
}

static int cblsm_create(int H, int W, int D, const smt_cblsm_params *p, smt_cblsm_flow **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    // pixel indices are int, and so are the (line, 64-hypothesis chunk) wave counts of the table kernels
    if ((long long)H * W * (SMT_MAX_DISPARITY / 64) > INT_MAX) return SMT_ERR_ARG;
    smt_cblsm_params P;
    if (p) P = *p; else smt_cblsm_default_params(&P);
    // tau is CBLSM.cpp:30's uchar; the arm limits are those smt_crossarm_create accepts
    if (P.tau < 0 || P.tau > 255 || P.sec_length < 0 || P.max_length < 0 || P.max_length > 4096) return SMT_ERR_ARG;
    smt_cblsm_flow *h = new (std::nothrow) smt_cblsm_flow();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->P = P;
    h->sat = cblsm_sat_exact(P);
    smt_crossarm_params cp;
    smt_crossarm_cblsm_params(&cp);                  // tau_low 6 (CBLSM.h:719), by-value threshold, no stride bug
    cp.tau = P.tau; cp.sec_length = P.sec_length; cp.max_length = P.max_length;
    const size_t V = (size_t)H * W * D * 4;
    int rc = smt_crossarm_create(H, W, D, &cp, &h->caL);
    if (rc == SMT_OK) rc = smt_crossarm_create(H, W, D, &cp, &h->caR);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->pass1[0], V);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->pass1[1], V);
    if (rc == SMT_OK) rc = smt_malloc(&h->scratch, V);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->err, 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->post_err, 4);
    // a few hundred KiB beside the volumes, so that run_batch_window never allocates whatever winSize it is given
    const size_t padded = ((size_t)H + 2 * CBLSM_WINDOW_MAX_W) * ((size_t)W + 2 * CBLSM_WINDOW_MAX_W);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->padL, padded);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->padR, padded);
    if (rc == SMT_OK && (hipMemset(h->err, 0, 4) != hipSuccess || hipMemset(h->post_err, 0, 4) != hipSuccess)) rc = SMT_ERR_HIP;
    if (rc != SMT_OK) { smt_cblsm_flow_destroy(h); return rc; }
    *out = h;
    return SMT_OK;
}

SMT_API int smt_cblsm_flow_create_on(int device, int H, int W, int D, const smt_cblsm_params *p, smt_cblsm_flow **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return cblsm_create(H, W, D, p, out);
}

SMT_API int smt_cblsm_flow_set_stream(smt_cblsm_flow *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->stream = smt_stream(s);
    int rc = smt_crossarm_set_stream(h->caL, s);
    if (rc == SMT_OK) rc = smt_crossarm_set_stream(h->caR, s);
    return rc;
}

// summed-area table of one view's AD volume (0 left, 1 right) -> h->scratch
static void cblsm_sat_table(smt_cblsm_flow *h, const uint8_t *L8, const uint8_t *R8, int view)
{
    const int H = h->H, W = h->W, D = h->D;
    const int nck = (D + 63) / 64;
    uint32_t *S = (uint32_t *)h->scratch;
    const dim3 blk(NT);
    const unsigned gc = (unsigned)(((long long)W * nck + 3) / 4), gr = (unsigned)(((long long)H * nck + 3) / 4);
    if (view == 0) hipLaunchKernelGGL(k_sat_cols<0>, dim3(gc), blk, 0, h->stream, L8, R8, H, W, D, nck, S);
    else hipLaunchKernelGGL(k_sat_cols<1>, dim3(gc), blk, 0, h->stream, L8, R8, H, W, D, nck, S);
    hipLaunchKernelGGL(k_sat_rows, dim3(gr), blk, 0, h->stream, H, W, D, nck, S);
}

// first pass of one view (0 left, 1 right) on the arms of `ca` -> h->pass1[view]
static int cblsm_first_pass(smt_cblsm_flow *h, smt_crossarm *ca, const uint8_t *L8, const uint8_t *R8, int view)
{
    const int H = h->H, W = h->W, D = h->D;
    if (!h->sat) {                                                                  // m > 127: CBLSM.h:327-381, :1179-1224
        int rc = smt_cblsm_ad(L8, R8, H, W, D, view == 0 ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, (float *)h->scratch, (void *)h->stream);
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(ca, (const float *)h->scratch, h->pass1[view], 1, nullptr);
        return rc;
    }
    int *arm[4];
    int rc = smt_crossarm_arm_maps(ca, &arm[0], &arm[1], &arm[2], &arm[3]);
    if (rc != SMT_OK) return rc;
    cblsm_sat_table(h, L8, R8, view);
    hipLaunchKernelGGL(k_sat_box, dim3((unsigned)(((long long)H * W + 3) / 4)), dim3(NT), 0, h->stream,
                       (const uint32_t *)h->scratch, arm[0], arm[1], arm[2], arm[3], H, W, D, h->pass1[view], h->err);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_cblsm_flow_run_batch(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                     float *dispL, float *dispR)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR || !dispL || !dispR) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const size_t N = (size_t)h->H * h->W;
    float *vol2 = (float *)h->scratch;
    for (int b = 0; b < pairs; b++) {
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        int rc = smt_crossarm_arms(h->caL, L8, 1);                                   // CBLSM.cpp:64-67
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                     // :101-104
        if (rc == SMT_OK) rc = cblsm_first_pass(h, h->caL, L8, R8, 0);               // :133, :147
        if (rc == SMT_OK) rc = cblsm_first_pass(h, h->caR, L8, R8, 1);               // :134, :146
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, h->pass1[0], vol2, 1, dispL + b * N);   // :149, :152
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, h->pass1[1], vol2, 1, dispR + b * N);   // :150 (LEFT arms), :153
        if (rc != SMT_OK) return rc;
    }
    return SMT_OK;
}

// CBLSM.cpp with :132 enabled: the window costs of ComputeDispLeft, and ComputeDispRight as the right view's counterpart,
// in place of ComputeAD / ComputeADRight.  No summed-area shortcut here: a window cost is the float nearest to S / n, not
// an integer, so the partial sums of costAggregationV5's float loop round and their order matters -- both passes of both
// views are crossarm.hip's in-order walk (order 1), which adds in the reference's order.  The scratch holds each window
// volume and then each second-pass output, so the handle's three volumes suffice.
SMT_API int smt_cblsm_flow_run_batch_window(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int winSize,
                                            float *dispL, float *dispR)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR || !dispL || !dispR || winSize < 0 || winSize + 1 > CBLSM_WINDOW_MAX_W) return SMT_ERR_ARG;
    const int H = h->H, W = h->W, D = h->D, w = winSize + 1;
    if (W <= w) return SMT_ERR_REF_UB;                                               // ComputeDispRight reads before its buffer
    smt_dev_guard dev_guard(h->device);
    const size_t N = (size_t)H * W;
    float *vol = (float *)h->scratch;
    void *st = (void *)h->stream;
    for (int b = 0; b < pairs; b++) {
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        int rc = smt_crossarm_arms(h->caL, L8, 1);                                   // CBLSM.cpp:64-67
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                     // :101-104
        if (rc == SMT_OK) rc = smt_pad_replicate(L8, H, W, w, h->padL, st);          // :124
        if (rc == SMT_OK) rc = smt_pad_replicate(R8, H, W, w, h->padR, st);          // :125
        if (rc == SMT_OK) rc = smt_cblsm_window_cost_batch(h->padL, h->padR, 1, 0, H, W, D, winSize, SMT_CBLSM_COST_LEFT, vol, 0, st);   // :132
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol, h->pass1[0], 1, nullptr);             // :147
        if (rc == SMT_OK) rc = smt_cblsm_window_cost_batch(h->padL, h->padR, 1, 0, H, W, D, winSize, SMT_CBLSM_COST_RIGHT, vol, 0, st);
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caR, vol, h->pass1[1], 1, nullptr);             // :146
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, h->pass1[0], vol, 1, dispL + b * N);       // :149, :152
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, h->pass1[1], vol, 1, dispR + b * N);       // :150 (LEFT arms), :153
        if (rc != SMT_OK) return rc;
    }
    return SMT_OK;
}

// The per-hypothesis-arm flow (CBLSM.cpp:64-67, 101-104, 108-111, 133, costAggregationV4, 152), left view only.  Within
// the summed-area bound the four arm volumes and the AD volume never exist: the table of the left view's AD and the
// eight arm maps feed one kernel (cblsm_v4.hip).  Past it the handle composes the library's own entry points on six
// volumes: AD in the scratch, the arm volumes in pass1[1] and three more allocated on first use, the result in pass1[0].
SMT_API int smt_cblsm_flow_run_batch_v4(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                        float *dispL)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR || !dispL) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, D = h->D;
    const size_t N = (size_t)H * W, V = N * D;
    if (!h->sat && !h->v4_arms) {
        const int rc = smt_malloc((void **)&h->v4_arms, 3 * V * sizeof(int));
        if (rc != SMT_OK) return rc;
    }
    void *st = (void *)h->stream;
    for (int b = 0; b < pairs; b++) {
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        int *aL[4], *aR[4];
        int rc = smt_crossarm_arms(h->caL, L8, 1);                                   // CBLSM.cpp:64-67
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                     // :101-104
        if (rc == SMT_OK) rc = smt_crossarm_arm_maps(h->caL, &aL[0], &aL[1], &aL[2], &aL[3]);
        if (rc == SMT_OK) rc = smt_crossarm_arm_maps(h->caR, &aR[0], &aR[1], &aR[2], &aR[3]);
        if (rc != SMT_OK) return rc;
        if (h->sat) {
            cblsm_sat_table(h, L8, R8, 0);                                           // :133 as a table
            // :108-111, costAggregationV4, :152; only the last pair's volume is ever lent
            rc = smt_cblsm_v4_box_enqueue((const uint32_t *)h->scratch, aL, aR, H, W, D, b == pairs - 1 ? h->pass1[0] : nullptr,
                                          dispL + b * N, h->err, h->stream);
        } else {
            int *vL = (int *)h->pass1[1], *vR = h->v4_arms, *vU = h->v4_arms + V, *vD = h->v4_arms + 2 * V;
            rc = smt_cblsm_choose_arm_length(0, aL[0], nullptr, aR[0], aR[1], H, W, D, vL, st);                  // :108
            if (rc == SMT_OK) rc = smt_cblsm_choose_arm_length(1, aL[1], nullptr, aR[0], aR[1], H, W, D, vR, st);  // :109
            if (rc == SMT_OK) rc = smt_cblsm_choose_arm_length(2, aL[2], aR[2], aR[0], aR[1], H, W, D, vU, st);    // :110
            if (rc == SMT_OK) rc = smt_cblsm_choose_arm_length(3, aL[3], aR[3], aR[0], aR[1], H, W, D, vD, st);    // :111
            if (rc == SMT_OK) rc = smt_cblsm_ad(L8, R8, H, W, D, SMT_VIEW_LEFT, (float *)h->scratch, st);          // :133
            if (rc == SMT_OK) rc = smt_cblsm_cost_aggregation_v4((const float *)h->scratch, vL, vR, vU, vD, H, W, D, h->pass1[0],
                                                                 dispL + b * N, h->err, st);                    // :152
        }
        if (rc != SMT_OK) return rc;
    }
    return SMT_OK;
}

// run_batch for all pairs, then CBLSM.cpp:160-162 once over the batch (the in-place median's parallel axis is the batch)
SMT_API int smt_cblsm_flow_run_batch_post(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                          float *dispL, float *dispR, uint8_t *cls, int *counts,
                                          const smt_cblsm_post_params *post)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!cls || (post && (post->median_wnd < 1 || post->median_wnd > 7))) return SMT_ERR_ARG;
    int rc = smt_cblsm_flow_run_batch(h, grayL, grayR, pairs, dispL, dispR);
    if (rc != SMT_OK) return rc;
    smt_dev_guard dev_guard(h->device);
    return smt_cblsm_tail_batch(dispL, dispR, pairs, 0, h->H, h->W, post, cls, counts, h->post_err, (void *)h->stream);
}

SMT_API int smt_cblsm_flow_volumes(smt_cblsm_flow *h, float **pass1_left, float **pass1_right)
{
    if (!h) return SMT_ERR_ARG;
    if (pass1_left) *pass1_left = h->pass1[0];
    if (pass1_right) *pass1_right = h->pass1[1];
    return SMT_OK;
}

SMT_API int smt_cblsm_flow_status(smt_cblsm_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return SMT_ERR_HIP;
    int rc = smt_crossarm_status(h->caL);
    { const int c = smt_crossarm_status(h->caR); if (rc == SMT_OK) rc = c; }
    int e = 0;
    if (hipMemcpy(&e, h->err, 4, hipMemcpyDeviceToHost) != hipSuccess) e = 1;
    if (e) { (void)hipMemset(h->err, 0, 4); if (rc == SMT_OK) rc = SMT_ERR_REF_UB; }
    e = 0;
    if (hipMemcpy(&e, h->post_err, 4, hipMemcpyDeviceToHost) != hipSuccess) e = 1;
    if (e) { (void)hipMemset(h->post_err, 0, 4); if (rc == SMT_OK) rc = SMT_ERR_STATE; }
    return rc;
}

// Host only (no GPU): the box arithmetic above against direct sums.  An AD-like uint8 volume (fill 0: random 0..255,
// 1: all 255), random arms up to max_arm (every seventh pixel's may leave the plane, then cblsm_box must say so and
// sum the clipped rectangle), a uint32 summed-area table built as the kernels build it; for sampled pixels the
// four-corner sum must equal the direct integer sum, and (float)S / (float)n must equal costAggregationV5's sequential
// float sum (rows outer, columns inner) over the same count -- the exactness argument, checked.  The centre pixel gets
// max_arm in every direction when that fits.
SMT_API int smt_cblsm_selftest_box(int H, int W, int D, int max_arm, int fill, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || max_arm < 0 || (long long)H * W * D > (1ll << 26)) return SMT_ERR_ARG;
    const size_t N = (size_t)H * W;
    uint8_t *ad = new (std::nothrow) uint8_t[N * D];
    uint32_t *S = new (std::nothrow) uint32_t[N * D];
    int *arm = new (std::nothrow) int[N * 4];
    if (!ad || !S || !arm) { delete[] ad; delete[] S; delete[] arm; return SMT_ERR_ALLOC; }
    uint32_t st = seed;
    auto rnd = [&st]() { st = st * 1664525u + 1013904223u; return st >> 8; };
    for (size_t k = 0; k < N * D; k++) ad[k] = fill ? 255 : (uint8_t)(rnd() & 255);
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            int *a = arm + ((size_t)i * W + j) * 4;
            const bool out = (rnd() % 7) == 0;
            const int lim[4] = {j, W - 1 - j, i, H - 1 - i};
            for (int q = 0; q < 4; q++) {
                const int m = out ? max_arm : (lim[q] < max_arm ? lim[q] : max_arm);
                a[q] = (int)(rnd() % (uint32_t)(m + 1));
            }
        }
    if (H / 2 >= max_arm && H - 1 - H / 2 >= max_arm && W / 2 >= max_arm && W - 1 - W / 2 >= max_arm)
        for (int q = 0; q < 4; q++) arm[((size_t)(H / 2) * W + W / 2) * 4 + q] = max_arm;
    // the kernels' order: column prefix, then row prefix, mod 2^32
    for (size_t k = 0; k < N * D; k++) S[k] = ad[k];
    for (int i = 1; i < H; i++)
        for (size_t k = 0; k < (size_t)W * D; k++) S[(size_t)i * W * D + k] += S[(size_t)(i - 1) * W * D + k];
    for (int i = 0; i < H; i++)
        for (int j = 1; j < W; j++)
            for (int d = 0; d < D; d++) S[((size_t)i * W + j) * D + d] += S[((size_t)i * W + j - 1) * D + d];
    // sample pixels so that the direct sums stay near 2^26 taps; the centre pixel always
    const double area = (double)(2 * max_arm + 1) * (2 * max_arm + 1);
    const size_t step = 1 + (size_t)((double)N * D * (area < (double)N ? area : (double)N) / (double)(1 << 26));
    auto check = [&](size_t q) {
        const int i = (int)(q / W), j = (int)(q % W);
        const int *a = arm + q * 4;
        int c[4], n;
        const bool clip = cblsm_box(i, j, a[0], a[1], a[2], a[3], H, W, c, n);
        const bool leaves = j - a[0] < 0 || j + a[1] > W - 1 || i - a[2] < 0 || i + a[3] > H - 1;
        if (clip != leaves) return false;
        const int i0 = i - a[2] < 0 ? 0 : i - a[2], i1 = i + a[3] > H - 1 ? H - 1 : i + a[3];
        const int j0 = j - a[0] < 0 ? 0 : j - a[0], j1 = j + a[1] > W - 1 ? W - 1 : j + a[1];
        if (n != (i1 - i0 + 1) * (j1 - j0 + 1)) return false;
        for (int d = 0; d < D; d++) {
            uint64_t direct = 0;
            float seq = 0.0f;
            for (int t = i0; t <= i1; t++)
                for (int l = j0; l <= j1; l++) {
                    const uint8_t v = ad[((size_t)t * W + l) * D + d];
                    direct += v;
                    seq = seq + (float)v;
                }
            const uint32_t s = cblsm_box_sum(S, (size_t)D, c, d);
            if ((uint64_t)s != direct) return false;
            const float got = (float)s / (float)n, ref = seq / (float)n;
            if (direct < (1u << 24) && memcmp(&got, &ref, 4) != 0) return false;
        }
        return true;
    };
    int rc = check((size_t)(H / 2) * W + W / 2) ? SMT_OK : SMT_ERR_STATE;
    for (size_t p = 0; p < N && rc == SMT_OK; p += step)
        if (!check(p)) rc = SMT_ERR_STATE;
    delete[] ad; delete[] S; delete[] arm;
    return rc;
}
