// smt_whole_ncc: NCC.h's whole-image ncc() (NCC.h:117-272), the matcher NCC_main.cpp:24 calls in a commented line, and
// bgr_to_grey (:97-115) that belongs with it.  The statement of the function, the exact integer form of its cost and the
// limit of that form are at the head of csrc/ncc_whole_rules.h; include/smt.h says what was decided about its defects.
//
// Two formulations, both splitting the offsets 1 .. O into G consecutive runs over the grid's y axis; a workgroup keeps
// the winner of its run per pixel (nw_offer, the reference's own `>`), writes it to an arena table [G][H][W], and
// k_nw_finish combines the runs in their order with the same statement.  That is exactly the sequential rule (the first
// of equal costs stays, a NaN never wins) for any G, needs no atomics, and no workgroup waits for another.
//   LOOP  k_nw_loop: one lane per pixel, :199-224 loop for loop in float64, with one difference: the reference squares with
//         pow(x, 2) and this kernel with x * x, which is the same double only where libm's pow is correctly rounded for
//         the exponent 2 (the recorded fixture pins maps, not costs).  The independent formulation, and the only one for
//         kernel_size > 35.
//   INT   k_nw_stats + k_nw_box.  The four sums that do not depend on the offset -- Sa, Saa and the shifted image's
//         Sb, Sbb -- come from per-row prefix sums of the clamped vertical window sums of v and v^2, one statistics launch
//         per call: any horizontal range is two loads, and the shifted window is at most two ranges (nw_shift_ranges).
//         Sab is a running sum down the rows (one lane per column, entering and leaving rows gated by the clamps) and a
//         sum over the clamped columns in LDS.  All in uint32; nw_int_cost turns the integers into the cost.
// The cost stores of INT are strided by O doubles across the lanes: the volume is a diagnostic output, the maps are not
// (measured at 450x375: the call with the volume takes 1.5 to 1.7 times the maps-only call).
#include "smt_common.h"
#include "ncc_whole_rules.h"
#include "box_stage.h"
#include <new>
#include <vector>

namespace {

constexpr int NWT = 256;           // lanes per workgroup of every kernel here
constexpr int NWR = 8;             // rows per workgroup of k_nw_box
constexpr long NW_TARGET = 2048;   // workgroups a cost launch aims for when it chooses G (256 CUs x 8)

int g_nw_impl = 0;                 // 0: nw_rule; 1: LOOP; 2: INT wherever it exists
int g_nw_last = 0;                 // SMT_NCC_WHOLE_FORM_* of the last successful call
int g_nw_groups = 0;               // test hook: runs of offsets per launch, 0 = nw_groups' choice
int g_nw_last_groups = 0;          // the G of the last successful call

// Which form serves kernel_size k by default.  Measured on one MI355X (tools/ncc_whole_time.py,
// profiles/ncc_whole_time.json; INT over LOOP, medians of 21 interleaved samples, left type):
//   0.146 at 450x375 k = 5 O = 79, 0.148 at 1242x375 O = 128, 0.129 at 1920x1080 O = 192, 0.025 at 450x375 k = 15.
// INT therefore serves wherever it exists.  Only those four points are timed; every other k <= 35, O and image size is
// extrapolation (INT's work per hypothesis grows with 2k + 1, LOOP's with its square).
int nw_rule(int k) { return k <= NW_INT_MAX_K ? SMT_NCC_WHOLE_FORM_INT : SMT_NCC_WHOLE_FORM_LOOP; }

struct nw_outs {                   // per view slot (a single-view call uses slot 0)
    uint8_t *depth[2];
    int32_t *off[2];
    double *cost[2];
};

struct nw_grey_table { uint8_t t[256]; };

__global__ void __launch_bounds__(NWT) k_nw_add(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, size_t n, int c)
{
    for (size_t t = (size_t)blockIdx.x * NWT + threadIdx.x; t < n; t += (size_t)gridDim.x * NWT) {
        const int v = src[t] + c;
        dst[t] = (uint8_t)(v > 255 ? 255 : v);                 // cv::Mat += int saturates
    }
}

__global__ void __launch_bounds__(NWT) k_nw_grey(const uint8_t *__restrict__ bgr, uint8_t *__restrict__ grey, size_t n, nw_grey_table T)
{
    for (size_t t = (size_t)blockIdx.x * NWT + threadIdx.x; t < n; t += (size_t)gridDim.x * NWT)
        grey[t] = (uint8_t)(T.t[bgr[3 * t + 2]] + T.t[bgr[3 * t + 1]] + T.t[bgr[3 * t]]);   // <= 3 * 84: no wrap
}

// tab: [4][pairs][H][W + 1] -- sums of L, squares of L, sums of R, squares of R.  Row y of a table: entry c is the sum over
// the columns below c of the vertical window sum of rows nw_lo(y) .. nw_hi(y); entry 0 is 0.  grid (H, 2 * pairs):
// blockIdx.y & 1 picks the image.  The row is scanned in chunks of NWT columns with a carry.
__global__ void __launch_bounds__(NWT) k_nw_stats(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int pairs, int H,
                                                  int W, int k, uint32_t *__restrict__ tab)
{
    __shared__ uint32_t s1[NWT], s2[NWT];
    const int y = blockIdx.x, img = blockIdx.y & 1, pair = blockIdx.y >> 1, tid = threadIdx.x;
    const size_t N = (size_t)H * W, TW = (size_t)W + 1, TS = (size_t)pairs * H * TW;
    const uint8_t *src = (img ? R : L) + (size_t)pair * N;
    uint32_t *o1 = tab + (size_t)(2 * img) * TS + ((size_t)pair * H + y) * TW, *o2 = o1 + TS;
    const int sy = nw_lo(y, k), ey = nw_hi(y, k, H);
    uint32_t c1 = 0, c2 = 0;                                   // carries: the sums of the chunks before this one
    if (tid == 0) { o1[0] = 0; o2[0] = 0; }
    for (int x0 = 0; x0 < W; x0 += NWT) {
        const int x = x0 + tid;
        uint32_t v1 = 0, v2 = 0;
        if (x < W)
            for (int i = sy; i <= ey; i++) { const uint32_t v = src[(size_t)i * W + x]; v1 += v; v2 += v * v; }
        s1[tid] = v1; s2[tid] = v2;
        __syncthreads();
        for (int off = 1; off < NWT; off <<= 1) {              // inclusive scan
            const uint32_t a1 = tid >= off ? s1[tid - off] : 0u, a2 = tid >= off ? s2[tid - off] : 0u;
            __syncthreads();
            s1[tid] += a1; s2[tid] += a2;
            __syncthreads();
        }
        if (x < W) { o1[x + 1] = c1 + s1[tid]; o2[x + 1] = c2 + s2[tid]; }
        c1 += s1[NWT - 1]; c2 += s2[NWT - 1];
        __syncthreads();
    }
}

// grid (ceil(H W / NWT), G, pairs * nv)
__global__ void __launch_bounds__(NWT) k_nw_loop(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R, int H, int W, int k,
                                                 int O, int G, int view0, int nv, double *__restrict__ pc, int *__restrict__ po,
                                                 nw_outs outs)
{
    const size_t N = (size_t)H * W, pix = (size_t)blockIdx.x * NWT + threadIdx.x;
    if (pix >= N) return;
    const int g = blockIdx.y, pv = blockIdx.z, pair = pv / nv, vs = pv % nv, vr = (view0 + vs) == SMT_VIEW_RIGHT;
    const uint8_t *Lp = L + (size_t)pair * N, *Rp = R + (size_t)pair * N;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const int sx = nw_lo(x, k), ex = nw_hi(x, k, W), sy = nw_lo(y, k), ey = nw_hi(y, k, H);
    const double n = (double)((ey - sy) * (ex - sx));          // :190
    int o_lo, o_hi;
    nw_group(O, G, g, o_lo, o_hi);
    double best = -2.0;                                        // :137
    int best_o = 0;
    double *cost = outs.cost[vs];
    for (int o = o_lo; o <= o_hi; o++) {
        double am = 0, bm = 0;
        for (int i = sy; i <= ey; i++)
            for (int j = sx; j <= ex; j++) {
                const int sc = nw_shift_col(vr, j, o, W);
                am += (double)Lp[(size_t)i * W + (vr ? sc : j)];
                bm += (double)Rp[(size_t)i * W + (vr ? j : sc)];
            }
        am /= n; bm /= n;
        double as = 0, bs = 0, num = 0;
        for (int i = sy; i <= ey; i++)
            for (int j = sx; j <= ex; j++) {
                const int sc = nw_shift_col(vr, j, o, W);
                const double da = (double)Lp[(size_t)i * W + (vr ? sc : j)] - am;
                const double db = (double)Rp[(size_t)i * W + (vr ? j : sc)] - bm;
                as += da * da; bs += db * db; num += da * db;
            }
        num /= n; as /= n; bs /= n;
        const double res = num / (sqrt(as) * sqrt(bs)) / n;    // :224
        if (cost) cost[((size_t)pair * N + pix) * O + (o - 1)] = res;
        nw_offer(res, o, best, best_o);
    }
    const size_t q = ((size_t)pv * G + g) * N + pix;
    pc[q] = best; po[q] = best_o;
}

// grid (xtiles * ceil(H / NWR), G, pairs * nv).  Lane tid holds column xc = tile * TX - k + tid, TX = NWT - 2k output
// columns per workgroup (k <= 35: at least 186); lanes k .. k + TX - 1 are the outputs, the others their halo.
__global__ void __launch_bounds__(NWT) k_nw_box(const uint8_t *__restrict__ L, const uint8_t *__restrict__ R,
                                                const uint32_t *__restrict__ tab, int pairs, int H, int W, int k, int O, int G,
                                                int view0, int nv, int xtiles, double *__restrict__ pc, int *__restrict__ po,
                                                nw_outs outs)
{
    __shared__ uint32_t s_v[2][NWT];
    const int TX = NWT - 2 * k, tid = threadIdx.x;
    const int tx = blockIdx.x % xtiles, ty = blockIdx.x / xtiles;
    const int g = blockIdx.y, pv = blockIdx.z, pair = pv / nv, vs = pv % nv, vr = (view0 + vs) == SMT_VIEW_RIGHT;
    const size_t N = (size_t)H * W, TW = (size_t)W + 1, TS = (size_t)pairs * H * TW;
    const uint8_t *plain = (vr ? R : L) + (size_t)pair * N, *shifted = (vr ? L : R) + (size_t)pair * N;
    const uint32_t *pl1 = tab + (size_t)(vr ? 2 : 0) * TS + (size_t)pair * H * TW, *pl2 = pl1 + TS;
    const uint32_t *sh1 = tab + (size_t)(vr ? 0 : 2) * TS + (size_t)pair * H * TW, *sh2 = sh1 + TS;
    const int xc = tx * TX - k + tid, y0 = ty * NWR;
    const bool incol = xc >= 0 && xc < W;
    const bool outp = tid >= k && tid < k + TX && xc < W;
    const int sx = nw_lo(xc, k), ex = nw_hi(xc, k, W);         // used by output lanes only
    int o_lo, o_hi;
    nw_group(O, G, g, o_lo, o_hi);
    double best[NWR];
    int best_o[NWR];
#pragma unroll
    for (int r = 0; r < NWR; r++) { best[r] = -2.0; best_o[r] = 0; }
    double *cost = outs.cost[vs];
    int par = 0;
    for (int o = o_lo; o <= o_hi; o++) {
        const int cp = incol ? xc : 0, cs = incol ? nw_shift_col(vr, xc, o, W) : 0;
        unsigned V = 0;                                        // sum of a b down the window rows of row y, this column
        if (incol)
            for (int i = nw_lo(y0, k); i <= nw_hi(y0, k, H); i++)
                V = __builtin_amdgcn_udot4((unsigned)plain[(size_t)i * W + cp], (unsigned)shifted[(size_t)i * W + cs], V, false);
#pragma unroll
        for (int r = 0; r < NWR; r++) {
            const int y = y0 + r;
            if (y < H) {                                       // uniform over the workgroup
                if (r > 0 && incol) {
                    // single products through the intrinsic, as csrc/ncc_box.hip:158-164 writes them: plain byte multiplies in
                    // a sliding sum were folded into v_dot4 with a leaving product added (tools/dot4_fold_probe.hip)
                    if (y + k <= H - 1)
                        V = __builtin_amdgcn_udot4((unsigned)plain[(size_t)(y + k) * W + cp], (unsigned)shifted[(size_t)(y + k) * W + cs], V, false);
                    if (y - 1 - k >= 0)
                        V = V - __builtin_amdgcn_udot4((unsigned)plain[(size_t)(y - 1 - k) * W + cp],
                                                       (unsigned)shifted[(size_t)(y - 1 - k) * W + cs], 0u, false);
                }
                s_v[par][tid] = V;
                __syncthreads();                               // one barrier per step: the next step writes the other half
                if (outp) {
                    unsigned Sab = 0;
                    for (int c = sx; c <= ex; c++) Sab += s_v[par][tid + (c - xc)];
                    const int sy = nw_lo(y, k), ey = nw_hi(y, k, H);
                    const uint32_t *r1 = pl1 + (size_t)y * TW, *r2 = pl2 + (size_t)y * TW;
                    const uint32_t *q1 = sh1 + (size_t)y * TW, *q2 = sh2 + (size_t)y * TW;
                    int f0, f1, m0, m1;
                    nw_shift_ranges(vr, sx, ex, o, W, f0, f1, m0, m1);
                    const uint32_t Sp = nw_range(r1, sx, ex), Spp = nw_range(r2, sx, ex);
                    const uint32_t Ss = nw_range(q1, f0, f1) + nw_range(q1, m0, m1);
                    const uint32_t Sss = nw_range(q2, f0, f1) + nw_range(q2, m0, m1);
                    // symmetric in its two images bit for bit, so (plain, shifted) serves both views
                    const double res = nw_int_cost(ey - sy + 1, ex - sx + 1, Sp, Spp, Ss, Sss, Sab);
                    if (cost) cost[((size_t)pair * N + (size_t)y * W + xc) * O + (o - 1)] = res;
                    nw_offer(res, o, best[r], best_o[r]);
                }
                par ^= 1;
            }
        }
    }
    if (outp) {
#pragma unroll
        for (int r = 0; r < NWR; r++)
            if (y0 + r < H) {
                const size_t q = ((size_t)pv * G + g) * N + (size_t)(y0 + r) * W + xc;
                pc[q] = best[r]; po[q] = best_o[r];
            }
    }
}

// the runs in their order; depth = (uchar)(3 o) (:265), 0 where no offset won (the reference leaves such a pixel unwritten)
__global__ void __launch_bounds__(NWT) k_nw_finish(const double *__restrict__ pc, const int *__restrict__ po, size_t N, int G, int nv,
                                                   size_t total, nw_outs outs)
{
    const size_t t = (size_t)blockIdx.x * NWT + threadIdx.x;
    if (t >= total) return;
    const size_t pv = t / N, pix = t - pv * N, pair = pv / nv;
    const int vs = (int)(pv % nv);
    double best = -2.0;
    int best_o = 0;
    for (int g = 0; g < G; g++) {
        const size_t q = (pv * G + g) * N + pix;
        nw_offer(pc[q], po[q], best, best_o);
    }
    if (outs.depth[vs]) outs.depth[vs][pair * N + pix] = (uint8_t)(3 * best_o);
    if (outs.off[vs]) outs.off[vs][pair * N + pix] = best_o;
}

int nw_groups(long wgs, int O)
{
    long G = g_nw_groups > 0 ? g_nw_groups : (NW_TARGET + wgs - 1) / wgs;
    if (G < 1) G = 1;
    return (int)(G < O ? G : O);
}

int nw_form_for(int impl, int k)
{
    if (impl == 1 || k > NW_INT_MAX_K) return SMT_NCC_WHOLE_FORM_LOOP;
    return impl == 2 ? SMT_NCC_WHOLE_FORM_INT : nw_rule(k);
}

// Views view0 .. view0 + nv - 1 of `pairs` dense pairs, arguments already checked (1 <= O <= W, H, W >= 2, k >= 1).
int nw_enqueue(int form, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, const smt_whole_ncc_params &P, int view0, int nv,
               const nw_outs &outs, hipStream_t st)
{
    const int k = P.kernel_size, O = P.max_offset;
    const size_t N = (size_t)H * W, PN = (size_t)pairs * N;
    scratch_set S(st);
    const uint8_t *Ru = R;
    if (P.add_constant) {                                      // :127-130 on a copy: the caller's image stays as it is
        uint8_t *Rc = (uint8_t *)S.get(PN);
        if (!Rc) return SMT_ERR_ALLOC;
        const unsigned blocks = (unsigned)((PN + NWT - 1) / NWT < 65535 * 16 ? (PN + NWT - 1) / NWT : 65535 * 16);
        hipLaunchKernelGGL(k_nw_add, dim3(blocks), dim3(NWT), 0, st, R, Rc, PN, 10);
        SMT_LAUNCH_CHECK();
        Ru = Rc;
    }
    int G;
    unsigned gx, xtiles = 0;
    if (form == SMT_NCC_WHOLE_FORM_INT) {
        const int TX = NWT - 2 * k;
        xtiles = (unsigned)((W + TX - 1) / TX);
        gx = xtiles * (unsigned)((H + NWR - 1) / NWR);
    } else gx = (unsigned)((N + NWT - 1) / NWT);
    G = nw_groups((long)gx * pairs * nv, O);
    const size_t cells = (size_t)pairs * nv * G * N;
    double *pc = (double *)S.get(cells * 8);
    int *po = pc ? (int *)S.get(cells * 4) : nullptr;
    if (!po) return SMT_ERR_ALLOC;
    const dim3 grid(gx, (unsigned)G, (unsigned)(pairs * nv));
    if (form == SMT_NCC_WHOLE_FORM_INT) {
        uint32_t *tab = (uint32_t *)S.get((size_t)4 * pairs * H * ((size_t)W + 1) * 4);
        if (!tab) return SMT_ERR_ALLOC;
        hipLaunchKernelGGL(k_nw_stats, dim3((unsigned)H, (unsigned)(2 * pairs)), dim3(NWT), 0, st, L, Ru, pairs, H, W, k, tab);
        SMT_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nw_box, grid, dim3(NWT), 0, st, L, Ru, tab, pairs, H, W, k, O, G, view0, nv, (int)xtiles, pc, po, outs);
    } else
        hipLaunchKernelGGL(k_nw_loop, grid, dim3(NWT), 0, st, L, Ru, H, W, k, O, G, view0, nv, pc, po, outs);
    SMT_LAUNCH_CHECK();
    const size_t total = (size_t)pairs * nv * N;
    hipLaunchKernelGGL(k_nw_finish, dim3((unsigned)((total + NWT - 1) / NWT)), dim3(NWT), 0, st, pc, po, N, G, nv, total, outs);
    SMT_LAUNCH_CHECK();
    g_nw_last = form;
    g_nw_last_groups = G;
    return SMT_OK;
}

// what smt_whole_ncc and the flow reject: SMT_OK, SMT_ERR_ARG or SMT_ERR_REF_UB
int nw_check(int H, int W, const smt_whole_ncc_params &P)
{
    if (H < 2 || W < 2 || P.kernel_size < 1 || P.max_offset < 1 || P.max_offset > SMT_MAX_DISPARITY ||
        (size_t)H * W >= ((size_t)1 << 31) || H > 65535 || P.kernel_size > (1 << 14))
        return SMT_ERR_ARG;
    if (P.max_offset > W) return SMT_ERR_REF_UB;               // the shift loops write outside tmp (:149, :169)
    return SMT_OK;
}

}  // namespace

SMT_API void smt_whole_ncc_default_params(smt_whole_ncc_params *p)
{
    if (!p) return;
    p->kernel_size = 5;                                        // NCC.h:122
    p->max_offset = 79;                                        // :121
    p->add_constant = 0;                                       // :117
}

SMT_API int smt_whole_ncc_set_impl(int impl)
{
    if (impl < 0 || impl > 2) return SMT_ERR_ARG;
    g_nw_impl = impl;
    return SMT_OK;
}

SMT_API int smt_whole_ncc_last_form(void) { return g_nw_last; }

SMT_API int smt_whole_ncc_last_groups(void) { return g_nw_last_groups; }

SMT_API int smt_whole_ncc_set_groups(int groups)
{
    if (groups < 0) return SMT_ERR_ARG;
    g_nw_groups = groups;
    return SMT_OK;
}

SMT_API int smt_whole_ncc(const uint8_t *L, const uint8_t *R, int H, int W, const smt_whole_ncc_params *params, int view,
                          uint8_t *depth, int32_t *offset, double *cost, void *stream)
{
    smt_whole_ncc_params P;
    if (params) P = *params; else smt_whole_ncc_default_params(&P);
    if (!L || !R || !depth || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    const int rc = nw_check(H, W, P);
    if (rc != SMT_OK) return rc;
    nw_outs outs = {{depth, nullptr}, {offset, nullptr}, {cost, nullptr}};
    return nw_enqueue(nw_form_for(g_nw_impl, P.kernel_size), L, R, 1, H, W, P, view, 1, outs, smt_stream(stream));
}

SMT_API int smt_bgr_to_grey_batch(const uint8_t *bgr, int n, int H, int W, uint8_t *grey, void *stream)
{
    if (n < 0 || H <= 0 || W <= 0) return SMT_ERR_ARG;
    if (n == 0) return SMT_OK;
    if (!bgr || !grey) return SMT_ERR_ARG;
    nw_grey_table T;
    for (int v = 0; v < 256; v++) T.t[v] = (uint8_t)(0.333 * v);   // `uchar r = 0.333 * bgr...` (:107-109): truncated
    const size_t total = (size_t)n * H * W;
    const unsigned blocks = (unsigned)((total + NWT - 1) / NWT < 65535 * 16 ? (total + NWT - 1) / NWT : 65535 * 16);
    hipLaunchKernelGGL(k_nw_grey, dim3(blocks), dim3(NWT), 0, smt_stream(stream), bgr, grey, total, T);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// ---- host-only check -----------------------------------------------------------------------------------------------
namespace {

// k_nw_stats on the host: the same tables for one image
void nw_host_tables(const uint8_t *img, int H, int W, int k, std::vector<uint32_t> &t1, std::vector<uint32_t> &t2)
{
    const size_t TW = (size_t)W + 1;
    t1.assign((size_t)H * TW, 0u); t2.assign((size_t)H * TW, 0u);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            uint32_t v1 = 0, v2 = 0;
            for (int i = nw_lo(y, k); i <= nw_hi(y, k, H); i++) { const uint32_t v = img[(size_t)i * W + x]; v1 += v; v2 += v * v; }
            t1[y * TW + x + 1] = t1[y * TW + x] + v1;
            t2[y * TW + x + 1] = t2[y * TW + x] + v2;
        }
}

}  // namespace

// Host only (no GPU).  On four pairs of the shape -- pseudo-random, 255 against 255, opposed checkerboards, a shifted
// copy -- k_nw_box's recurrences restated with the kernel's own helpers (the same tiles, row strips, halo lanes, warm-up,
// entering and leaving rows, clamped column sums; the shifted image's Sb and Sbb from the prefix tables through
// nw_shift_ranges) equal the direct double loop over the window of the shifted image for Sab, Sb and Sbb at every
// (y, x, o): the fill columns and all four clamps are inside wherever the shape has them.
SMT_API int smt_whole_ncc_selftest_box(int H, int W, int kernel_size, int max_offset, int view, unsigned seed)
{
    smt_whole_ncc_params P = {kernel_size, max_offset, 0};
    if (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT) return SMT_ERR_ARG;
    const int rc = nw_check(H, W, P);
    if (rc != SMT_OK) return rc;
    if (kernel_size > NW_INT_MAX_K || (long long)H * W * max_offset > (1 << 22)) return SMT_ERR_ARG;
    const int k = kernel_size, O = max_offset, vr = view == SMT_VIEW_RIGHT, TX = NWT - 2 * k;
    const size_t N = (size_t)H * W, TW = (size_t)W + 1;
    std::vector<uint8_t> L(N), R(N);
    std::vector<uint32_t> t1, t2, want(N * O * 3), got(N * O * 3);
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
        const uint8_t *plain = vr ? R.data() : L.data(), *shifted = vr ? L.data() : R.data();
        // the direct statement: the shifted copy tmp (:143-174), then the window loops
        std::vector<uint8_t> tmp(N);
        for (int o = 1; o <= O; o++) {
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    if (!vr) tmp[(size_t)y * W + x] = x < o ? R[(size_t)y * W + x] : R[(size_t)y * W + x - o];
                    else tmp[(size_t)y * W + x] = x < W - o ? L[(size_t)y * W + x + o] : L[(size_t)y * W + x];
                }
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    uint32_t sab = 0, sb = 0, sbb = 0;
                    for (int i = nw_lo(y, k); i <= nw_hi(y, k, H); i++)
                        for (int j = nw_lo(x, k); j <= nw_hi(x, k, W); j++) {
                            const uint32_t a = plain[(size_t)i * W + j], b = tmp[(size_t)i * W + j];
                            sab += a * b; sb += b; sbb += b * b;
                        }
                    uint32_t *w = &want[(((size_t)y * W + x) * O + (o - 1)) * 3];
                    w[0] = sab; w[1] = sb; w[2] = sbb;
                }
        }
        // the kernel's walk
        std::fill(got.begin(), got.end(), 0xdeadbeefu);
        nw_host_tables(shifted, H, W, k, t1, t2);
        std::vector<uint32_t> V(NWT);
        for (int ty = 0; ty * NWR < H; ty++)
            for (int tx = 0; tx * TX < W; tx++)
                for (int o = 1; o <= O; o++) {
                    const int y0 = ty * NWR;
                    auto prod = [&](int i, int xc) {
                        return (uint32_t)plain[(size_t)i * W + xc] * (uint32_t)shifted[(size_t)i * W + nw_shift_col(vr, xc, o, W)];
                    };
                    for (int tid = 0; tid < NWT; tid++) {
                        const int xc = tx * TX - k + tid;
                        V[tid] = 0;
                        if (xc >= 0 && xc < W)
                            for (int i = nw_lo(y0, k); i <= nw_hi(y0, k, H); i++) V[tid] += prod(i, xc);
                    }
                    for (int r = 0; r < NWR && y0 + r < H; r++) {
                        const int y = y0 + r;
                        for (int tid = 0; tid < NWT; tid++) {
                            const int xc = tx * TX - k + tid;
                            if (r > 0 && xc >= 0 && xc < W) {
                                if (y + k <= H - 1) V[tid] += prod(y + k, xc);
                                if (y - 1 - k >= 0) V[tid] -= prod(y - 1 - k, xc);
                            }
                        }
                        for (int tid = k; tid < k + TX; tid++) {
                            const int xc = tx * TX - k + tid;
                            if (xc >= W) break;
                            const int sx = nw_lo(xc, k), ex = nw_hi(xc, k, W);
                            uint32_t sab = 0;
                            for (int c = sx; c <= ex; c++) sab += V[tid + (c - xc)];
                            int f0, f1, m0, m1;
                            nw_shift_ranges(vr, sx, ex, o, W, f0, f1, m0, m1);
                            const uint32_t *q1 = &t1[y * TW], *q2 = &t2[y * TW];
                            uint32_t *w = &got[(((size_t)y * W + xc) * O + (o - 1)) * 3];
                            w[0] = sab;
                            w[1] = nw_range(q1, f0, f1) + nw_range(q1, m0, m1);
                            w[2] = nw_range(q2, f0, f1) + nw_range(q2, m0, m1);
                        }
                    }
                }
        if (got != want) return SMT_ERR_STATE;
    }
    // The winner rule in runs, through the helpers the kernels use (nw_group, nw_offer): for every G the runs tile 1 .. O
    // once and in order (trailing runs may be empty), and the runs' winners combined in their order name the offset the
    // sequential loop of :261-266 names, on rows from a hostile palette: exact ties, NaN first and later, all NaN.
    const double qnan = nan("");
    const double palette[] = {qnan, -1.0, -0.5, 0.0, -0.0, 0.125, 0.125, 0.5, 0.5, 1.0};
    std::vector<double> row(O);
    for (int rep = 0; rep < 8; rep++) {
        for (int o = 0; o < O; o++) row[o] = rep == 0 ? qnan : (rep == 1 ? 0.25 : palette[rng.next() % (rep == 2 ? 4 : 10)]);
        double sb = -2.0;
        int so = 0;
        for (int o = 1; o <= O; o++) nw_offer(row[o - 1], o, sb, so);
        for (int G = 1; G <= O; G++) {
            double best = -2.0;
            int best_o = 0, next = 1;
            for (int g = 0; g < G; g++) {
                int o_lo, o_hi;
                nw_group(O, G, g, o_lo, o_hi);
                if (o_lo <= o_hi && o_lo != next) return SMT_ERR_STATE;
                if (o_lo <= o_hi) next = o_hi + 1;
                double b = -2.0;
                int bo = 0;
                for (int o = o_lo; o <= o_hi; o++) nw_offer(row[o - 1], o, b, bo);
                nw_offer(b, bo, best, best_o);
            }
            if (next != O + 1 || best_o != so) return SMT_ERR_STATE;
        }
    }
    return SMT_OK;
}

// ---- smt_whole_ncc_flow_*: NCC_main.cpp with :24 enabled, both types, for a batch of gray pairs -----------------------
// Both views share one statistics launch (each reads one image plain and the other shifted: the same four tables) and one
// cost launch with the view on a grid axis.  The right type's interior costs equal the left type's at (y, x + o, o) word
// for word (csrc/ncc_whole_rules.h); a flow that takes them from the left pass is not built.  OPEN: whether sharing
// would be faster was to be decided by measurement and has not been measured.  Everything the call needs comes from the arena: the handle owns no device memory.
struct smt_whole_ncc_flow {
    int device;
    int H, W;
    smt_whole_ncc_params P;
    hipStream_t stream;
    int form;                   // 0: as smt_whole_ncc chooses; else SMT_NCC_WHOLE_FORM_*
};

SMT_API int smt_whole_ncc_flow_create_on(int device, int H, int W, const smt_whole_ncc_params *p, smt_whole_ncc_flow **out)
{
    if (!out) return SMT_ERR_ARG;
    smt_whole_ncc_params P;
    if (p) P = *p; else smt_whole_ncc_default_params(&P);
    const int rc = nw_check(H, W, P);
    if (rc != SMT_OK) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    smt_whole_ncc_flow *h = new (std::nothrow) smt_whole_ncc_flow();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->P = P;
    *out = h;
    return SMT_OK;
}

SMT_API int smt_whole_ncc_flow_destroy(smt_whole_ncc_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    delete h;
    return SMT_OK;
}

SMT_API int smt_whole_ncc_flow_set_stream(smt_whole_ncc_flow *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_whole_ncc_flow_set_form(smt_whole_ncc_flow *h, int form)
{
    if (!h || form < 0 || form > SMT_NCC_WHOLE_FORM_INT) return SMT_ERR_ARG;
    if (form == SMT_NCC_WHOLE_FORM_INT && h->P.kernel_size > NW_INT_MAX_K) return SMT_ERR_ARG;
    h->form = form;
    return SMT_OK;
}

SMT_API int smt_whole_ncc_flow_run_batch(smt_whole_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                         uint8_t *depthL, uint8_t *depthR, int32_t *offL, int32_t *offR, int32_t *lastdisp,
                                         uint8_t *cls)
{
    if (!h || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR) return SMT_ERR_ARG;
    if (!depthL && !depthR && !offL && !offR && !lastdisp && !cls) return SMT_OK;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W;
    const size_t N = (size_t)H * W;
    hipStream_t st = h->stream;
    const int form = h->form ? h->form : nw_form_for(g_nw_impl, h->P.kernel_size);
    const bool check = lastdisp || cls;
    scratch_set S(st);
    int32_t *ol = offL, *orr = offR, *last1 = nullptr;
    uint8_t *cls1 = nullptr;
    if (check) {                                               // the cross-check reads both offset maps
        if (!ol && !(ol = (int32_t *)S.get((size_t)pairs * N * 4))) return SMT_ERR_ALLOC;
        if (!orr && !(orr = (int32_t *)S.get((size_t)pairs * N * 4))) return SMT_ERR_ALLOC;
        if (!lastdisp && !(last1 = (int32_t *)S.get(N * 4))) return SMT_ERR_ALLOC;
        if (!cls && !(cls1 = (uint8_t *)S.get(N))) return SMT_ERR_ALLOC;
    }
    const bool needL = depthL || ol, needR = depthR || orr;
    int rc;
    if (needL && needR) {
        nw_outs outs = {{depthL, depthR}, {ol, orr}, {nullptr, nullptr}};
        rc = nw_enqueue(form, grayL, grayR, pairs, H, W, h->P, SMT_VIEW_LEFT, 2, outs, st);
    } else {
        nw_outs outs = {{needL ? depthL : depthR, nullptr}, {needL ? ol : orr, nullptr}, {nullptr, nullptr}};
        rc = nw_enqueue(form, grayL, grayR, pairs, H, W, h->P, needL ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, 1, outs, st);
    }
    if (rc == SMT_OK && check)
        for (int b = 0; b < pairs && rc == SMT_OK; b++)       // Sad.h:184-222 on the call's own offset maps
            rc = smt_sad_crosscheck(ol + b * N, orr + b * N, H, W, lastdisp ? lastdisp + b * N : last1, cls ? cls + b * N : cls1,
                                    (void *)st);
    return rc;
}
