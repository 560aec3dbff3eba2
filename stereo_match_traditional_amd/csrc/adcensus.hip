// AD + 9x7 census cost volume with fused WTA -- replaces class AD_Census
// (AD-CensusV1/AD-Census.h) for both views.
//
// Formulation (different from the reference's per-(i,j,d) census rebuild, AD-Census.h:142-269,
// same results):
//   left  view: census(i,j,d) = popcount((cenA_L[i][j] ^ cenX_R[i][max(j-d,-3)]) & M[i][j])
//               AD(i,j,d)     = |L[i][j] - R[i][max(j-d,0)]|
//   right view: census(i,j,d) = popcount((cenA_R[i][j] ^ cenX_L[i][min(j+d,W+3)]) & M[i][j])
//               AD(i,j,d)     = |L[i][min(j+d,W-1)] - R[i][j]|
// with cenA_* the ordinary 63-bit census of the anchor image (invalid taps = 0), M the
// in-image tap mask of the anchor pixel (validity is tested on anchor coordinates,
// AD-Census.h:173 / :238), cenX_R the right image's census on a left-replicate-extended
// row (:159-160, :177-178) and cenX_L the left image's census with the reference's
// "column 0 past the right edge" rule for neighbours and "column W-1" rule for the
// centre (:224-225, :242-243).  The "copy d-1" branches of ComputeAD (:88-92, :116-120)
// are exactly the clamps above.
//   cost = lutA[AD] + lutC[census], lutA[k] = 1-expf(-(k/sigmaC)), lutC[k] = 1-expf(-(k/sigmaS))
// built on the HOST with the reference's own float expression (:287-289), so the device
// never evaluates exp.  AD in 0..255 and census in 0..63 because images are integer-valued.
//
// Main kernel: one wavefront spans the disparity axis of one pixel; lane l owns the C =
// D/64 consecutive hypotheses d = l*C .. l*C+C-1 and stores them with one
// dword/x2/x3/x4 store (64*C*4 contiguous bytes per wave).  Row operands are staged in
// LDS once per workgroup; WTA is a wave min + ballot (first strict minimum, :355-373).
#include "smt_common.h"
#include "adcensus_internal.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include <type_traits>

namespace {

constexpr int TJ = 64;        // pixels per workgroup
constexpr int NT = 256;       // threads per workgroup (4 waves)

struct Tables {
    // per view v (0 = left anchor, 1 = right anchor)
    uint64_t *cenA[2];   // [H][W]
    uint64_t *cenX[2];   // [H][WX]   view0: index x+3, x in [-3,W-1]; view1: index x, x in [0,W+3]
    uint64_t *mask;      // [H][W]
    uint8_t *u8[2];      // [H][W] left, right as bytes
    float *lut;          // 256 + 64 floats
    uint16_t *rank;      // [256][64]: dense rank of lut[ad] + lut[256 + hd] (build_rank), maps-only kernel
    int *flag;           // domain flag
    int WX;
    int edge_col;        // cenX_L's column for neighbours past the right edge (prep_edges): 0 as the reference reads,
                         // W-1 (replicate) with SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE
    unsigned long long *stamp;   // diagnostics only (smt_adcensus_diag): 4 counters per workgroup, else null
};

// ---- tap validity mask + the four census tables --------------------------------------
// bit layout: tap t = (r+4)*7 + (c+3), r in [-4,4] outer, c in [-3,3] inner, MSB first:
// bit (62 - t)  (63 left shifts of a 64-bit word, AD-Census.h:171-172).
//
// Away from the left/right borders the extended tables equal the ordinary censuses:
//   cenX_R[xr] == cenA_R[xr] for xr >= 3      (no neighbour column is clamped to 0)
//   cenX_L[xl] == cenA_L[xl] for xl <= W-4    (no neighbour wraps to column 0, centre unclamped)
// so k_prep computes the two ordinary censuses + mask once per pixel from an LDS-staged 64x32 tile and
// writes them to both places; prep_edges (extra workgroups of the same launch) fills the 6 + 7 special
// columns per row.
constexpr int PTW = 64;                                     // tile: 64 columns x 32 rows per workgroup
constexpr int PTH = 32;
constexpr int PNT = 256;                                    // each thread does one column of 8 rows

__device__ __forceinline__ unsigned to_u8_checked(float a, bool &bad)
{
    const int ia = (int)a;
    bad = bad || !(a >= 0.0f && a <= 255.0f && (float)ia == a);
    return (unsigned)ia & 0xffu;
}

// the border columns of the extended tables: xr in [-3, 2] and xl in [W-3, W+3], by the general rule.
// Runs in extra workgroups of the k_prep launch (16 rows each, 13 of 16 lanes per row), reading the
// float images directly (their domain is checked by the tile workgroups).
__device__ __forceinline__ void prep_edges(const float *__restrict__ Lf, const float *__restrict__ Rf, int H, int W,
                                           const Tables &T, int block)
{
    const int i = block * (PNT / 16) + (threadIdx.x >> 4);
    const int e = threadIdx.x & 15;
    if (i >= H || e >= 13) return;
    const int WX = T.WX;
    if (e < 6) {
        const int xr = e - 3;
        if (xr > W - 1) return;                          // narrower than 3 columns
        const int cc = xr < 0 ? 0 : xr;
        const unsigned rc = (unsigned)(int)Rf[(size_t)i * W + cc];
        uint64_t w = 0;
#pragma unroll 1
        for (int r = -4; r <= 4; r++) {
            const int ii = i + r;
            const bool rv = (ii >= 0 && ii < H);
            const int ic = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii);
#pragma unroll
            for (int c = -3; c <= 3; c++) {
                int jj = xr + c;
                jj = jj < 0 ? 0 : jj;                    // left replicate (:177-178)
                const bool v = rv && jj < W;
                const unsigned val = (unsigned)(int)Rf[(size_t)ic * W + (jj < W ? jj : W - 1)];
                w = (w << 1) | (uint64_t)(v && rc > val);
            }
        }
        T.cenX[0][(size_t)i * WX + e] = w;
    } else {
        const int xl = W - 3 + (e - 6);
        if (xl < 0) return;
        const int cc = xl > W - 1 ? W - 1 : xl;          // centre clamps to W-1 (:224-225)
        const unsigned lc = (unsigned)(int)Lf[(size_t)i * W + cc];
        uint64_t w = 0;
#pragma unroll 1
        for (int r = -4; r <= 4; r++) {
            const int ii = i + r;
            const bool rv = (ii >= 0 && ii < H);
            const int ic = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii);
#pragma unroll
            for (int c = -3; c <= 3; c++) {
                int jj = xl + c;
                jj = jj >= W ? T.edge_col : jj;          // neighbour wraps to column 0 (:242-243), or replicates the edge
                const bool v = rv && jj >= 0;
                const unsigned val = (unsigned)(int)Lf[(size_t)ic * W + (jj < 0 ? 0 : jj)];
                w = (w << 1) | (uint64_t)(v && lc > val);
            }
        }
        T.cenX[1][(size_t)i * WX + xl] = w;
    }
}

// Census words of PRR consecutive rows of one column of one image (IMG 0 = left, 1 = right) from the staged tile.
// The two images are processed one after the other and a thread's rows in groups of PRR, so the live window is
// (PRR + 8) x 2 dwords and only PRR rows' store addresses are in flight: with PRR = 1 prep_tile takes 51 VGPRs (122 in
// the form that kept 16 rows of both images in registers) and fits beside the cost kernel it is fused with (below) at
// 8 waves per SIMD.
constexpr int PSC = PTW + 6;                                // staged columns (3-column halo)
constexpr int PSW = (PSC + 2 + 3) / 4 + 1;                  // row stride in dwords (one spare for the 3rd dword)
constexpr int PRR = 1;
template <int IMG>
__device__ __forceinline__ void prep_rows(const uint32_t (*__restrict__ sw)[PSW], int i0, int row0, int x, int col,
                                          unsigned colbits, int H, int W, const Tables &T)
{
    // The thread's 7-byte window [col, col+6] of each of the PRR+8 staged rows it needs, as two dwords: three
    // aligned LDS dwords shifted by col%4 bytes.  Bytes past col+6 are never used.
    const int cw = col >> 2;
    const unsigned sh = (unsigned)(col & 3);
    uint32_t w0[PRR + 8], w1[PRR + 8];
#pragma unroll
    for (int r = 0; r < PRR + 8; r++) {
        const uint32_t a0 = sw[row0 + r][cw], a1 = sw[row0 + r][cw + 1], a2 = sw[row0 + r][cw + 2];
        w0[r] = __builtin_amdgcn_alignbyte(a1, a0, sh); w1[r] = __builtin_amdgcn_alignbyte(a2, a1, sh);
    }
#pragma unroll
    for (int rr = 0; rr < PRR; rr++) {
        const int i = i0 + row0 + rr;
        if (i >= H) break;
        // centre = byte 3 of the window of staged row rr+4
        const int cc = (int)(w0[rr + 4] >> 24);
        T.u8[IMG][(size_t)i * W + x] = (uint8_t)cc;
        // census word, MSB first over taps t = r*7 + c: bit = centre > neighbour = sign of
        // (neighbour - centre), shifted in with one v_alignbit per tap.  Taps 0..30 fill the high word
        // (bits 62..32), taps 31..62 the low word; every staged byte is readable, the raw bits are
        // masked afterwards with the tap-validity word.
        uint32_t ch = 0, cl = 0;
        uint64_t m = 0;
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int ii = i + r - 4;
            if (ii >= 0 && ii < H) m |= (uint64_t)colbits << (56 - 7 * r);
#pragma unroll
            for (int c = 0; c < 7; c++) {
                const int t = r * 7 + c;
                const uint32_t w = c < 4 ? w0[rr + r] : w1[rr + r];
                const int dv = (int)((w >> (8 * (c & 3))) & 0xffu) - cc;
                if (t < 31) ch = __builtin_amdgcn_alignbit(ch, (uint32_t)dv, 31);
                else cl = __builtin_amdgcn_alignbit(cl, (uint32_t)dv, 31);
            }
        }
        const uint64_t cen = (((uint64_t)ch << 32) | cl) & m;
        const size_t p = (size_t)i * W + x;
        T.cenA[IMG][p] = cen;
        if (IMG == 0) {
            T.mask[p] = m;
            if (x <= W - 4) T.cenX[1][(size_t)i * T.WX + x] = cen;      // cenX_L index = xl
        } else {
            if (x >= 3) T.cenX[0][(size_t)i * T.WX + x + 3] = cen;      // cenX_R index = xr + 3
        }
    }
}

// One workgroup of the table launch: (bx, by) of a (gdx, ...) grid -- a 64 x 32 tile, or past the tile rows a block
// of border columns.  Called with workgroup-uniform arguments by k_prep and by the table workgroups of k_cost_fast2p /
// k_cost_maps2p, each of which passes its own LDS staging area (PSR rows of PSW dwords per image).
constexpr int PSR = PTH + 8;                                // staged rows (4-row halo)
__device__ __forceinline__ void prep_tile(const float *__restrict__ Lf, const float *__restrict__ Rf, int H, int W,
                                          const Tables &T, int bx, int by, int gdx, uint32_t (*__restrict__ sLw)[PSW],
                                          uint32_t (*__restrict__ sRw)[PSW])
{
    constexpr int SR = PSR;
    const int tiles_y = (H + PTH - 1) / PTH;
    if (by >= tiles_y) {                                    // workgroup-uniform, before any barrier
        prep_edges(Lf, Rf, H, W, T, (by - tiles_y) * gdx + bx);
        return;
    }
    const int i0 = by * PTH;
    const int x0 = bx * PTW;
    const int tid = threadIdx.x;
    // stage the tile + halo straight from the float images (coordinates clamped; out-of-image taps
    // are masked); this also is the float -> u8 conversion + domain check
    bool bad = false;
#pragma unroll 2
    for (int e = tid; e < SR * PSC; e += PNT) {
        const int r = e / PSC, c = e - r * PSC;
        int ii = i0 + r - 4, jj = x0 + c - 3;
        ii = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii);
        jj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
        ((uint8_t *)sLw[r])[c] = (uint8_t)to_u8_checked(Lf[(size_t)ii * W + jj], bad);
        ((uint8_t *)sRw[r])[c] = (uint8_t)to_u8_checked(Rf[(size_t)ii * W + jj], bad);
    }
    if (__syncthreads_or(bad) && tid == 0) atomicOr(T.flag, 1);
    const int col = tid & (PTW - 1);
    const int x = x0 + col;
    if (x >= W) return;
    constexpr int RPT = PTH / (PNT / PTW);                  // output rows per thread (consecutive)
    static_assert(RPT % PRR == 0, "");
    // column validity of the 7 taps, MSB = leftmost tap
    unsigned colbits = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) colbits |= (unsigned)(x + c - 3 >= 0 && x + c - 3 < W) << (6 - c);
#pragma unroll 1
    for (int s = 0; s < RPT / PRR; s++) {
        const int row0 = (tid / PTW) * RPT + s * PRR;
        prep_rows<0>(sLw, i0, row0, x, col, colbits, H, W, T);
        __builtin_amdgcn_sched_barrier(0);                  // one image's window at a time in registers
        prep_rows<1>(sRw, i0, row0, x, col, colbits, H, W, T);
    }
}

__global__ void __launch_bounds__(PNT) k_prep(const float *__restrict__ Lf, const float *__restrict__ Rf,
                                              int H, int W, Tables T)
{
    __shared__ uint32_t sLw[PSR][PSW];
    __shared__ uint32_t sRw[PSR][PSW];
    prep_tile(Lf, Rf, H, W, T, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, sLw, sRw);
}

template <int C> struct vecf { float v[C]; };          // C = 5..8 (D > 256): plain struct, the kernels there use the per-element paths
template <> struct vecf<1> { float v[1]; };
template <> struct __attribute__((aligned(8))) vecf<2> { float v[2]; };
template <> struct vecf<3> { float v[3]; };
template <> struct __attribute__((aligned(16))) vecf<4> { float v[4]; };

// ---- cost volume + WTA ---------------------------------------------------------------
// grid: (ceil(W/TJ), H, nviews)   block: 256
// FULL: D == 64*C (every lane active, vector store); otherwise C = ceil(D/64) with tail
// lanes masked and scalar stores.
template <int C, bool FULL>
__global__ void __launch_bounds__(NT) k_cost(int H, int W, int D, Tables T, int view0,
                                             float *__restrict__ vol0, float *__restrict__ vol1,
                                             float *__restrict__ disp0, float *__restrict__ disp1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int view = view0 + blockIdx.z;
    const int i = blockIdx.y;
    const int j0 = blockIdx.x * TJ;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int NX = TJ + D;                                  // staged ext entries (>= TJ + D - 1)

    uint64_t *s_cenx = (uint64_t *)smem;                    // NX
    uint64_t *s_cena = s_cenx + NX;                         // TJ
    uint64_t *s_mask = s_cena + TJ;                         // TJ
    float *s_lutA = (float *)(s_mask + TJ);                 // 256
    float *s_lutC = s_lutA + 256;                           // 64
    uint8_t *s_valx = (uint8_t *)(s_lutC + 64);             // NX
    uint8_t *s_vala = s_valx + NX;                          // TJ

    const int WX = T.WX;
    const uint64_t *cenX = T.cenX[view] + (size_t)i * WX;
    const uint8_t *extv = T.u8[view ^ 1] + (size_t)i * W;   // left view reads R, right view reads L
    const uint8_t *ancv = T.u8[view] + (size_t)i * W;
    // staged entry e <-> ext coordinate x:  view 0: x = j0 - (D-1) + e ; view 1: x = j0 + e
    const int xbase = (view == 0) ? (j0 - (D - 1)) : j0;
    for (int e = tid; e < NX; e += NT) {
        int x = xbase + e;
        int xc, xv;
        if (view == 0) {
            xc = x < -3 ? -3 : (x > W - 1 ? W - 1 : x);
            xv = xc < 0 ? 0 : xc;
            xc += 3;
        } else {
            xc = x > W + 3 ? W + 3 : x;
            xv = x > W - 1 ? W - 1 : x;
        }
        s_cenx[e] = cenX[xc];
        s_valx[e] = extv[xv];
    }
    for (int e = tid; e < TJ; e += NT) {
        int j = j0 + e;
        if (j > W - 1) j = W - 1;
        s_cena[e] = T.cenA[view][(size_t)i * W + j];
        s_mask[e] = T.mask[(size_t)i * W + j];
        s_vala[e] = ancv[j];
    }
    for (int e = tid; e < 320; e += NT) s_lutA[e] = T.lut[e];
    __syncthreads();

    float *vol = view == 0 ? vol0 : vol1;
    float *disp = view == 0 ? disp0 : disp1;
    const int dl = lane * C;                                // first hypothesis of this lane

    for (int p = wid; p < TJ; p += NT / 64) {
        const int j = j0 + p;
        if (j >= W) break;
        const uint64_t ca = s_cena[p], mk = s_mask[p];
        const int va = s_vala[p];
        // ext entry of hypothesis d: view 0: e = p + (D-1) - d ; view 1: e = p + d
        float c[C];
        float best = 0.0f; int bestk = 0;
#pragma unroll
        for (int k = 0; k < C; k++) {
            const int d = dl + k;
            int e = (view == 0) ? (p + (D - 1) - d) : (p + d);
            if (!FULL) e = (d < D) ? e : 0;
            const uint64_t x = (ca ^ s_cenx[e]) & mk;
            const int hd = __popcll(x);
            int ad = va - (int)s_valx[e];
            ad = ad < 0 ? -ad : ad;
            const float cost = s_lutA[ad] + s_lutC[hd];
            c[k] = cost;
            if (k == 0) { best = cost; bestk = 0; }
            else if (best > cost) { best = cost; bestk = k; }
        }
        float *out = vol + ((size_t)i * W + j) * D + dl;
        if (FULL) {
            vecf<C> pk;
#pragma unroll
            for (int k = 0; k < C; k++) pk.v[k] = c[k];
            *reinterpret_cast<vecf<C> *>(out) = pk;
        } else {
#pragma unroll
            for (int k = 0; k < C; k++)
                if (dl + k < D) out[k] = c[k];
        }
        if (disp) {
            float bv = best;
            if (!FULL) {
                // lanes past D must never win; lanes straddling D keep only their valid prefix
                if (dl >= D) bv = INFINITY;
                else if (dl + C > D) {
                    bv = c[0]; bestk = 0;
#pragma unroll
                    for (int k = 1; k < C; k++)
                        if (dl + k < D && bv > c[k]) { bv = c[k]; bestk = k; }
                }
            }
            const int wd = wave_argmin_first(bv, dl + bestk);
            if (lane == 0) disp[(size_t)i * W + j] = (float)wd;
        }
    }
}

// ---- production path (any D <= 256; FULL specialisation for D == 64*C) -------------------
// Same mapping (one wave per pixel, lane l owns d = l*C..l*C+C-1) with the instruction count
// cut down: VIEW is a template parameter; each wave walks FPW CONSECUTIVE pixels so that
// a lane's C ext operands form a register sliding window (one new LDS entry per pixel
// instead of C); values are staged pre-multiplied by 4 so v_sad_u16 yields the lutA byte
// address directly; the WTA is a DPP min over the cost bit patterns (costs are >= +0, so
// uint order == float order) + ballot + scalar pick, no LDS round trips; the FPW winners
// are collected one per lane and stored once per wave.
#ifndef SMT_FTJ
#define SMT_FTJ 64
#endif
constexpr int FTJ = SMT_FTJ;      // pixels per workgroup
constexpr int FPW = FTJ / 4;      // consecutive pixels per wave

// Streaming (non-temporal) store of C consecutive floats: the volumes are written once and are far
// larger than L2 + Infinity Cache, so they should not displace the tables the next workgroups read.
// With the XCD-contiguous chunk order this is worth 5-6 % of the kernel (A/B); with chunks in
// dispatch order it cost 4 %.
// The volume stores are buffer stores: SGPR resource (base = the wave's first pixel, range = the wave's run, so a
// store past the run is dropped by the hardware) + a constant VGPR lane offset + an SGPR offset that advances by
// one pixel (D * 4 bytes) with a scalar add -- no vector instruction is spent on store addresses.  aux = 2 is the
// nt bit of gfx940+ (what __builtin_nontemporal_store puts on a global_store).
typedef int si2 __attribute__((ext_vector_type(2)));
typedef int si3 __attribute__((ext_vector_type(3)));
typedef int si4 __attribute__((ext_vector_type(4)));
template <int C, bool NTS = true>
__device__ __forceinline__ void st_stream(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const float (&v)[C])
{
    constexpr int AUX = NTS ? 2 : 0;
    if (C == 1) __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(v[0]), r, voff, soff, AUX);
    else if (C == 2) {
        si2 x; x.x = __float_as_int(v[0]); x.y = __float_as_int(v[C > 1 ? 1 : 0]);
        __builtin_amdgcn_raw_buffer_store_b64(x, r, voff, soff, AUX);
    } else if (C == 3) {
        si3 x; x.x = __float_as_int(v[0]); x.y = __float_as_int(v[C > 1 ? 1 : 0]); x.z = __float_as_int(v[C > 2 ? 2 : 0]);
        __builtin_amdgcn_raw_buffer_store_b96(x, r, voff, soff, AUX);
    } else {
        si4 x; x.x = __float_as_int(v[0]); x.y = __float_as_int(v[C > 1 ? 1 : 0]); x.z = __float_as_int(v[C > 2 ? 2 : 0]);
        x.w = __float_as_int(v[C > 3 ? 3 : 0]);
        __builtin_amdgcn_raw_buffer_store_b128(x, r, voff, soff, AUX);
    }
}

// ---- rules of the shared maps-only form (k_cost_maps_shared), host and device ----------------------------------------
// For 3 <= j' and j' + d <= W-4 the right view's cost(i, j', d) is bit for bit the left view's cost(i, j' + d, d): the
// edge-extended censuses equal the ordinary ones there, both column masks are all ones and the row masks are the same
// row, and neither AD clamp acts.  The left pass publishes these costs as keys to the right columns they belong to:
//   key = cost bits << 32 | d; costs are >= +0, so the unsigned minimum is the smallest cost, then the smallest d --
//   the reference's first strict minimum.  SH_NOKEY (all ones) is no key: d < 512.
// A left hypothesis (j, d) publishes when j <= W-4 and 3 <= j - d <= pubhi (shared_publishes), pubhi = W-4
// (shared_pub_hi): every shareable cost is published.  The columns of the IDENTITY SET 3 <= j' <= W-3-D get all their D
// hypotheses that way.  A column j' > W-3-D lacks the EDGE HYPOTHESES with j' + d >= W-3; the VIEW 1 staging clamps the
// census index to W+3 and the value index to W-1, so the cost is constant in d from W+3-j' on and only d <= W+3-j' can
// be a first minimum: at most 7 per column (shared_edge_range).  Columns 0..2 share nothing.  The launch's edge items evaluate
// the edge hypotheses from the tables and merge them with the column's key (shared_edge_item).
// Runs of chunks are those of chunk_decode (below).
#ifndef SMT_SHARED_KNOCKOUT
#define SMT_SHARED_KNOCKOUT 0      // measurement builds only (wrong maps): 1 no LDS publishes, 2 no key-map merges
#endif
constexpr int SH_RING = 512;                                 // key ring, indexed by right column mod 512
constexpr int SH_RING_N = SH_RING + 4;                       // + the spill slots of shared_ring_base() / shared_ring_slot()
constexpr unsigned long long SH_NOKEY = ~0ull;
__host__ __device__ inline int shared_id_hi(int W, int D) { return W - 3 - D; }           // the set is [3, hi]; empty when hi < 3
__host__ __device__ inline int shared_pub_hi(int W) { return W - 4; }                     // last published right column
__host__ __device__ inline bool shared_in_set(int c, int hi) { return (unsigned)(c - 3) <= (unsigned)(hi - 3) && hi >= 3; }
// left pixel j publishes a hypothesis to right column c = j - d
__host__ __device__ inline bool shared_publishes(int j, int c, int W, int pubhi) { return j <= W - 4 && shared_in_set(c, pubhi); }
__host__ __device__ inline unsigned long long shared_key(unsigned cost_bits, int d) { return ((unsigned long long)cost_bits << 32) | (unsigned)d; }
// A lane publishes its C hypotheses d = dl .. dl+C-1 of left pixel j to the right columns t - k, t = j - dl: ring slot
// base + (C-1-k) with base = (t - (C-1)) mod 512, one address computation per pixel.  A column c with c mod 512 < C-1
// can therefore land in slot c mod 512 or in the spill slot 512 + c mod 512; the flush takes the minimum of the two.
__host__ __device__ inline int shared_ring_base(int t, int C) { return (int)((unsigned)(t - (C - 1)) & (unsigned)(SH_RING - 1)); }
// The GROUPED form (shared_ring_grouped: the D = 192 kernel) computes the base once per group of C pixels, for the
// group's first pixel, column t0 = j0 - dl: pixel j0 + u publishes hypothesis k to slot base(t0) + u + (C-1-k), the
// offset a compile-time constant in [0, 2 (C-1)].  That is the slot ((c - o) mod 512) + o of column c = t0 + u - k
// with o = u + C-1-k, so a column c with c mod 512 < 2 (C-1) can land in c mod 512 or in the spill slot 512 + c mod
// 512: SH_SPILL = 4 spill slots at C <= 3 (C = 4 would need 6).  The flush takes the minimum of the two for every s
// below shared_ring_spill(): the slots the form can reach.
// A wave's groups start at its first pixel: pixel q of wave w of a run of n chunks is pixel 16 n w + q of the run.
constexpr int SH_SPILL = SH_RING_N - SH_RING;
// shared_walk_groups: the walk takes whole groups of C pixels without a per-pixel exit, then the pixels left over.
// Both are switched per instantiation (Dfull: 64 C, or 0 when D != 64 C); measured at D = 192 and D = 128, DESIGN.md
// section 4.  The grouped ring needs the group loop.
__host__ __device__ constexpr bool shared_walk_groups(int C, int Dfull) { return C == 3 && Dfull == 192; }
__host__ __device__ constexpr bool shared_ring_grouped(int C, int Dfull) { return C == 3 && Dfull == 192; }
static_assert(!shared_ring_grouped(3, 192) || shared_walk_groups(3, 192), "");
__host__ __device__ inline int shared_ring_slot(int t0, int u, int k, int C) { return shared_ring_base(t0, C) + u + (C - 1 - k); }
__host__ __device__ constexpr int shared_ring_spill(int C, bool grouped) { return grouped ? 2 * (C - 1) : C - 1; }
static_assert(shared_ring_spill(3, true) <= SH_SPILL && shared_ring_spill(4, false) <= SH_SPILL, "");
// A whole run of at most SH_RUN = 4 chunks is published before its one flush (shared_run_flush_range), so at most
// 256 + D - 1 <= 511 columns are live (D <= 256): no two live columns share a slot of the ring of 512.
// Run walk.  A workgroup's chunks (chunk_decode over the left view alone, t = 0 .. K-1) are consecutive in the linear
// (row, chunk-in-row) space, so its first chunk (i, bx) and their number describe them: shared_wg_chunks, one division
// per workgroup.  Consecutive chunks of one row form a run; a run longer than SH_RUN chunks is cut into sub-runs of
// SH_RUN from its start, each a run in every respect (shared_run_len: chunks of the run that starts at chunk bx with
// `left` chunks of the workgroup to go).  The one flush of run [S, E] takes every column the run published to.
constexpr int SH_RUN = 4;
// Span rule of the maps-only launches (k_cost_maps_shared, k_cost_maps2p): how the `per` chunks of one XCD's slice are
// cut into workgroups.  Group g = b >> 3 of slice b & 7 takes maps_span()'s chunks [first, first + n) of the slice.
// The slice's last n1 groups take 1 chunk each, the n2 groups before them max(1, K / 2) each, every group before
// those K (the last of them what is left): a TAPERED TAIL, so that the workgroups of the launch's last round end
// closer together.  n2 = n1 = 0 is the plain rule, group g takes [g K, g K + K).  A slice too
// short for the tails shrinks them (maps_span_tails: first n1, then n2), so the body never goes negative and no
// group before maps_span_groups() is empty.  Workgroup-uniform, once per workgroup; the divisions are taken by the
// tail groups and by shrunk tails only.
__host__ __device__ inline long maps_span_tails(long per, int K, int &n2, int &n1)   // -> chunks of the body
{
    const int K2 = K > 1 ? K >> 1 : 1;
    if (n1 < 0) n1 = 0;
    if (n2 < 0) n2 = 0;
    if (n1 > per) n1 = (int)per;
    const long rem = per - n1;
    if ((long)n2 * K2 > rem) n2 = (int)(rem / K2);
    return rem - (long)n2 * K2;
}
__host__ __device__ inline int maps_span(long per, int K, int n2, int n1, long g, long &first)
{
    const long body = maps_span_tails(per, K, n2, n1);
    first = g * K;
    if (first < body) return (int)(body - first < K ? body - first : K);
    const int K2 = K > 1 ? K >> 1 : 1;
    const long gt = g - (body + K - 1) / K;                          // group of the tails
    if (gt < n2) { first = body + gt * K2; return K2; }
    first = body + (long)n2 * K2 + (gt - n2);
    return gt - n2 < n1 ? 1 : 0;
}
// groups of the body: the first tapered group, if any, is this one
__host__ __device__ inline long maps_span_body(long per, int K, int n2, int n1)
{
    return (maps_span_tails(per, K, n2, n1) + K - 1) / K;
}
__host__ __device__ inline long maps_span_groups(long per, int K, int n2, int n1)
{
    const long nbody = maps_span_body(per, K, n2, n1);               // shrinks n2, n1 by value only: shrink again
    (void)maps_span_tails(per, K, n2, n1);
    return nbody + n2 + n1;
}
__host__ __device__ inline int shared_wg_chunks(int nbx, int H, int K, long b, int &i, int &bx, int n2 = 0, int n1 = 0)
{
    const long nb = (long)nbx * H, per = (nb + 7) >> 3;
    long cl;
    const int m = maps_span(per, K, n2, n1, b >> 3, cl);
    if (m <= 0) return 0;
    const long c = (b & 7) * per + cl;
    if (c >= nb) return 0;
    i = (int)(c / nbx);
    bx = (int)(c - (long)i * nbx);
    const long n = nb - c;
    return (int)(n < m ? n : m);
}
__host__ __device__ inline int shared_run_len(int nbx, int bx, int left)
{
    const int n = nbx - bx < SH_RUN ? nbx - bx : SH_RUN;
    return n < left ? n : left;
}
__host__ __device__ inline void shared_run_flush_range(int S, int E, int D, int pubhi, int &lo, int &hi)
{
    lo = S - D + 1 < 3 ? 3 : S - D + 1; hi = E > pubhi ? pubhi : E;
}
// The whole diagonal j' .. j'+D-1 of right column c lies in the run's left columns [S, E] and in the identity set: the
// ring holds its final key, written straight to the map.  Otherwise the key is partial and merged through the handle's
// key map: with the other runs' keys, and past the identity set with the edge hypotheses (never complete).
__host__ __device__ inline bool shared_complete(int c, int S, int E, int D) { return c >= S && c + D - 1 <= E; }
__host__ __device__ inline bool shared_complete(int c, int S, int E, int D, int idhi) { return c <= idhi && shared_complete(c, S, E, D); }
// Edge hypotheses of right column c, evaluated by the edge items: d in [lo, hi] (columns 0..2: every d that can win).
__host__ __device__ inline void shared_edge_range(int c, int W, int D, int &lo, int &hi)
{
    lo = c >= 3 && W - 3 - c > 0 ? W - 3 - c : 0;
    hi = W + 3 - c < D - 1 ? W + 3 - c : D - 1;
}
// Auxiliary work items of a shared launch.  The workgroups of the fused grid's "table" class (fused_grid / fused_decode)
// take the items b = 0 .. naux-1 of one list: nprep table tiles of the NEXT pair, then nconv conversion items of the
// PREVIOUS pair, then nedge edge items of THIS pair (shared_aux_decode).
//   conversion item: SH_CONV_PX consecutive entries of the previous pair's key map, taken as a flat array of H*W keys,
//     two per 16-byte load: k != SH_NOKEY -> map entry (float)d, key reset.  Needs no tables.
//   edge item < shared_edge_col_items(): SH_EDGE_PX pixels of the columns idhi+1 .. W-1 in row-major order, one thread
//     per pixel at a time.  Columns <= W-4 merge their minimum over shared_edge_range into the key map with an atomic
//     min (minima commute with the cost workgroups' merges); the columns W-3 .. W-1 get no publishes and write the map.
//   the other edge items: SH_EDGE0_PX pixels of the columns 0..2, one wave per pixel, every hypothesis an edge one,
//     written to the map.
// INVARIANT: the key map holds keys only at the columns 3 .. W-4; the entries of the columns 0..2 and W-3 .. W-1 stay
// SH_NOKEY for ever, so a conversion over the whole flat array never touches the map entries the edge items wrote.
constexpr int SH_CONV_PX = 16 * 256;                         // 16 keys per thread (NT threads)
constexpr int SH_EDGE_PX = 4 * 256;
constexpr int SH_EDGE0_PX = 16 * 4;                          // 16 pixels per wave
__host__ __device__ inline int shared_conv_items(int H, int W) { return (int)(((long)H * W + SH_CONV_PX - 1) / SH_CONV_PX); }
__host__ __device__ inline int shared_edge_cols(int W, int D) { return W - 1 - shared_id_hi(W, D); }   // idhi+1 .. W-1
__host__ __device__ inline int shared_edge_col_items(int H, int W, int D)
{
    return (int)(((long)H * shared_edge_cols(W, D) + SH_EDGE_PX - 1) / SH_EDGE_PX);
}
__host__ __device__ inline int shared_edge_items(int H, int W, int D)
{
    return shared_edge_col_items(H, W, D) + (3 * H + SH_EDGE0_PX - 1) / SH_EDGE0_PX;
}
constexpr int AUX_PREP = 0, AUX_CONV = 1, AUX_EDGE = 2, AUX_NONE = 3;
__host__ __device__ inline int shared_aux_decode(int b, int nprep, int nconv, int nedge, int &item)
{
    item = b;
    if (item < nprep) return AUX_PREP;
    item -= nprep;
    if (item < nconv) return AUX_CONV;
    item -= nconv;
    return item < nedge ? AUX_EDGE : AUX_NONE;
}
// Pixel arithmetic of the items, step `it` of thread `tid` (wave `wv`): false past the end of the item's set.
__host__ __device__ inline bool shared_conv_px(int item, int it, int tid, long N, long &p)    // the keys p and p + 1
{
    p = (long)item * SH_CONV_PX + 2 * ((long)it * 256 + tid);
    return p < N;
}
__host__ __device__ inline bool shared_edge_px(int item, int it, int tid, int H, int W, int D, int &i, int &c)
{
    const int nc = shared_edge_cols(W, D);
    const long q = (long)item * SH_EDGE_PX + (long)it * 256 + tid;
    if (q >= (long)H * nc) return false;
    i = (int)(q / nc);
    c = shared_id_hi(W, D) + 1 + (int)(q - (long)i * nc);
    return true;
}
__host__ __device__ inline bool shared_edge0_px(int item, int it, int wv, int H, int &i, int &c)
{
    const int w = item * SH_EDGE0_PX + it * 4 + wv;
    if (w >= 3 * H) return false;
    i = w / 3; c = w - 3 * i;
    return true;
}

struct __attribute__((aligned(16))) Anchor { uint64_t cen, mask; };

// LDS of the maps-only kernel (k_cost_maps2p): its table plus the staged operands, one set shared by both views
// (the volume-writing kernels keep per-instantiation static arrays).  The table workgroups stage their tile in tab.
constexpr int MODE_VOLUME = 0, MODE_MAPS_FLOAT = 1, MODE_MAPS_RANK = 2;         // cost_fast_body's forms
constexpr int RANK_N = 256 * 64;
constexpr int XPAD = 4;
constexpr int PREP_LDS_U16 = 2 * PSR * PSW * 2;            // prep_tile's staging area in uint16 units
// NBUF staging sets: with two, chunk t+1 is written while chunk t is read (one barrier per chunk instead of two).
template <int C, int TABN = RANK_N, int NBUF = 1> struct MapsLds {
    uint16_t tab[TABN];                   // rank table (MODE_MAPS_RANK) or the 320-float LUT (MODE_MAPS_FLOAT)
    struct {
        Anchor anc[FTJ];
        uint64_t cenx[FTJ + 64 * C + 2 * XPAD];
        uint16_t valx[FTJ + 64 * C + 2 * XPAD];
        uint16_t vala[FTJ];
    } st[NBUF];
};
template <int MODE> struct MapsCfg {
    static constexpr int TABN = MODE == MODE_MAPS_FLOAT ? PREP_LDS_U16 : RANK_N;
    static constexpr int NBUF = MODE == MODE_MAPS_FLOAT ? 2 : 1;        // the rank form has no LDS to spare
};

// FULL: D == 64*C (no lane / element predication anywhere).  Otherwise C = ceil(D/64): lanes whose
// first hypothesis is >= D compute a harmless duplicate of lane 0, elements past D are neither
// stored nor allowed to win the WTA, and the staged arrays carry XPAD spare entries on both sides for
// the window slots those elements would touch.
// MODE 0 writes the volume (and the map when disp != null).  MODE 1 and 2 write the map only (disp != null, vol
// unused) and use the LDS of k_cost_maps2p (`ml`: staged operands in set `buf`, written by MapsStage, and the table the
// kernel has filled: MODE 1 the 320-float LUT, MODE 2 the 256 x 64 rank table, Tables::rank).  MODE 2 stages the image values x64, so that v_sad_u16(va, vx, hd) is the rank
// index 64*AD + hd, and its WTA key is rank << 16 | d: one wave min, no tie-break.
// The left pass of the shared form (shared_run_walk, below) has a walk of its own over a staged run of chunks: the same
// window, arithmetic and WTA, plus the publishes.
template <int C, int VIEW, bool FULL, bool NTS = true, int MODE = MODE_VOLUME>
__device__ __forceinline__ void cost_fast_body(int H, int W, int Drt, const Tables &T, float *__restrict__ vol,
                                               float *__restrict__ disp, int i, int bx,
                                               MapsLds<C, MapsCfg<MODE>::TABN, MapsCfg<MODE>::NBUF> *ml = nullptr, int buf = 0)
{
    constexpr bool STORE = MODE == MODE_VOLUME;
    constexpr unsigned VSCALE = MODE == MODE_MAPS_RANK ? 64u : 4u;
    constexpr int DM = 64 * C;                               // largest D this instantiation serves
    constexpr int NXM = FTJ + DM + 2 * XPAD;
    const int D = FULL ? DM : Drt;
    const int NX = FTJ + D;
    __shared__ Anchor s_anc_v[FTJ];
    __shared__ uint64_t s_cenx_v[NXM];
    __shared__ float s_lut[320];
    __shared__ uint16_t s_valx_v[NXM];
    __shared__ uint16_t s_vala_v[FTJ];
    Anchor *s_anc = STORE ? s_anc_v : ml->st[buf].anc;
    uint16_t *s_vala = STORE ? s_vala_v : ml->st[buf].vala;
    uint64_t *s_cenx = (STORE ? s_cenx_v : ml->st[buf].cenx) + XPAD;   // entry e in [-XPAD, NX + XPAD)
    uint16_t *s_valx = (STORE ? s_valx_v : ml->st[buf].valx) + XPAD;
    const void *tab = STORE ? nullptr : (const void *)ml->tab;

    const int j0 = bx * FTJ;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

    if (STORE) {                                             // the maps-only kernel stages through MapsStage
        const uint64_t *cenX = T.cenX[VIEW] + (size_t)i * T.WX;
        const uint8_t *extv = T.u8[VIEW ^ 1] + (size_t)i * W;
        const uint8_t *ancv = T.u8[VIEW] + (size_t)i * W;
        const int xbase = (VIEW == 0) ? (j0 - (D - 1)) : j0;
        for (int e = tid - (FULL ? 0 : XPAD); e < NX + (FULL ? 0 : XPAD); e += NT) {
            const int x = xbase + e;
            int xc, xv;
            if (VIEW == 0) {
                xc = x < -3 ? -3 : (x > W - 1 ? W - 1 : x);
                xv = xc < 0 ? 0 : xc;
                xc += 3;
            } else {
                xc = x > W + 3 ? W + 3 : (x < 0 ? 0 : x);
                xv = x > W - 1 ? W - 1 : (x < 0 ? 0 : x);
            }
            s_cenx[e] = cenX[xc];
            s_valx[e] = (uint16_t)(VSCALE * extv[xv]);
        }
        for (int e = tid; e < FTJ; e += NT) {
            int j = j0 + e;
            if (j > W - 1) j = W - 1;
            Anchor a;
            a.cen = T.cenA[VIEW][(size_t)i * W + j];
            a.mask = T.mask[(size_t)i * W + j];
            s_anc[e] = a;
            s_vala[e] = (uint16_t)(VSCALE * ancv[j]);
        }
        for (int e = tid; e < 320; e += NT) s_lut[e] = T.lut[e];
        __syncthreads();
    }

    const int p0 = wid * FPW;
    const int dlr = lane * C;                                // first hypothesis of this lane
    const int dl = (FULL || dlr < D) ? dlr : 0;              // lanes entirely past D shadow lane 0
    bool ok[C];
#pragma unroll
    for (int k = 0; k < C; k++) ok[k] = FULL || (dlr + k < D);
    // ext entry of (pixel p, hypothesis dl+k):  VIEW 0: p + (D-1) - dl - k ;  VIEW 1: p + dl + k
    // With E(n) = staged entry e0 + n, pixel q needs  VIEW 0: E(q-k)  /  VIEW 1: E(q+k), k = 0..C-1.
    // The C live entries sit in a register ring R[n mod C] = E(n); the pixel loop is unrolled by C so
    // every ring index is a compile-time constant (no register shuffling), and one new entry is
    // fetched per pixel.
    const int e0 = (VIEW == 0) ? (p0 + (D - 1) - dl) : (p0 + dl);
    uint64_t rc[C];
    unsigned rv[C];
#pragma unroll
    for (int k = 0; k < C; k++) {
        // ring slot of E(n) is n mod C;  VIEW 0 starts with E(0), E(-1), ..., E(-(C-1));  VIEW 1 with E(0..C-1)
        const int n = (VIEW == 0) ? -k : k;
        const int slot = ((n % C) + C) % C;
        rc[slot] = s_cenx[e0 + n];
        rv[slot] = s_valx[e0 + n];
    }
    const float *lut = STORE ? s_lut : (const float *)tab;
    const char *lutA = (const char *)lut;
    const float *lutC = lut + 256;
    const char *rankt = (const char *)tab;
    const unsigned ooff = (unsigned)dlr * 4u;
    unsigned osoff = 0;                                      // scalar byte offset of the current pixel in the wave's run
    int res = 0;
    const int npx = min(FPW, W - (j0 + p0));                 // uniform; may be <= 0
    __amdgpu_buffer_rsrc_t orsrc;
    if (STORE)
        orsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(vol + ((size_t)i * W + j0 + p0) * D), 0,
                                                  (npx > 0 ? npx : 0) * D * 4, 0x00020000);
    // interior run: every pixel of this wave has all 63 taps inside the image, so the tap mask is
    // all ones and the two ANDs per hypothesis can be dropped (bit 63 is 0 in every table entry)
    const bool interior = (i >= 4) && (i < H - 4) && (j0 + p0 >= 3) && (j0 + p0 + npx - 1 <= W - 4);

    auto run = [&](auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        // The anchor entries are read at wave-uniform LDS addresses.  The two addresses live in VGPRs that advance
        // once per group of C pixels (the pixels of a group use immediate offsets); left to itself the compiler keeps
        // them in SGPRs and spends two v_mov per pixel to feed the ds_read.
        typedef const __attribute__((address_space(3))) uint64_t *lds_u64_p;
        typedef const __attribute__((address_space(3))) uint16_t *lds_u16_p;
        uint32_t anc_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) Anchor *)(s_anc + p0);
        uint32_t val_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint16_t *)(s_vala + p0);
        asm volatile("" : "+v"(anc_a), "+v"(val_a));
        // maps-only forms: the same for the entry that joins the ring; the volume-writing form keeps its measured code
        uint32_t nx_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint64_t *)(s_cenx + e0);
        uint32_t nv_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint16_t *)(s_valx + e0);
        if (!STORE) asm volatile("" : "+v"(nx_a), "+v"(nv_a));
        for (int g = 0; g < npx; g += C) {
#pragma unroll
            for (int u = 0; u < C; u++) {
                const int q = g + u;
                if (q < npx) {
                    Anchor a;
                    if (MASKED) {                                            // one ds_read_b128
                        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
                        const u64x2 v = *(const __attribute__((address_space(3))) u64x2 *)(size_t)(anc_a + 16u * u);
                        a.cen = v.x; a.mask = v.y;
                    }
                    else { a.cen = *(lds_u64_p)(size_t)(anc_a + 16u * u); a.mask = 0; }
                    const unsigned va = *(lds_u16_p)(size_t)(val_a + 2u * u);
                    // entry that joins the ring for the next pixel (always inside the staged range)
                    const int nn = (VIEW == 0) ? (q + 1) : (q + C);
                    const uint64_t nc = STORE ? s_cenx[e0 + nn] : *(lds_u64_p)(size_t)(nx_a + 8u * (unsigned)(nn - g));
                    const unsigned nv = STORE ? s_valx[e0 + nn] : *(lds_u16_p)(size_t)(nv_a + 2u * (unsigned)(nn - g));
                    float c[C];
                    unsigned key[C];
#pragma unroll
                    for (int k = 0; k < C; k++) {
                        // E(q-k) / E(q+k) with q = u (mod C)
                        constexpr int dummy = 0; (void)dummy;
                        const int slot = (VIEW == 0) ? (((u - k) % C) + C) % C : (u + k) % C;
                        uint64_t x = a.cen ^ rc[slot];
                        if (MASKED) x &= a.mask;
                        if (MODE == MODE_MAPS_RANK) {
                            // 64*AD + hd, the popcount accumulated into the SAD; rank table entries are 2 bytes
                            const unsigned hd = __builtin_amdgcn_sad_u16(va, rv[slot], (unsigned)__popcll(x));
                            const unsigned rk = *(const uint16_t *)(rankt + 2u * hd);
                            key[k] = ok[k] ? ((rk << 16) | (unsigned)(dl + k)) : 0xFFFFFFFFu;
                        } else {
                            const int hd = __popcll(x);
                            const unsigned ad4 = __builtin_amdgcn_sad_u16(va, rv[slot], 0u);   // 4*|va - vx|
                            c[k] = *(const float *)(lutA + ad4) + lutC[hd];
                            key[k] = ok[k] ? __float_as_uint(c[k]) : 0xFFFFFFFFu;
                        }
                    }
                    if (STORE) {
                        if (FULL) st_stream<C, NTS>(orsrc, ooff, osoff, c);
                        else {
#pragma unroll
                            for (int k = 0; k < C; k++)
                                if (ok[k]) __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(c[k]), orsrc, ooff + 4u * k, osoff, NTS ? 2 : 0);
                        }
                        osoff += (unsigned)D * 4u;
                    }
                    if (MODE == MODE_MAPS_RANK) {
                        // smallest rank, then smallest d: the first strict minimum of the costs
                        unsigned ml = key[0];
#pragma unroll
                        for (int k = 1; k < C; k++) ml = min(ml, key[k]);
                        const int wd = (int)(wave_min_u32(ml) & 0xFFFFu);     // wave-uniform
                        res = (lane == q) ? wd : res;
                    } else if (!STORE || disp) {
                        unsigned ml = key[0];
#pragma unroll
                        for (int k = 1; k < C; k++) ml = min(ml, key[k]);
                        const unsigned m = wave_min_u32(ml);
                        const unsigned long long b = __ballot(ml == m);
                        const int first = __builtin_ctzll(b);
                        int kk = C - 1;
#pragma unroll
                        for (int k = C - 2; k >= 0; k--)
                            if ((unsigned)__builtin_amdgcn_readlane((int)key[k], first) == m) kk = k;
                        const int wd = first * C + kk;       // wave-uniform
                        res = (lane == q) ? wd : res;
                    }
                    // the new entry replaces the one that just left the window
                    const int ns = (VIEW == 0) ? (u + 1) % C : u % C;
                    rc[ns] = nc; rv[ns] = nv;
                }
            }
            anc_a += 16u * C; val_a += 2u * C;
            nx_a += 8u * C; nv_a += 2u * C;
        }
    };
    if (interior) run(std::false_type{});
    else run(std::true_type{});
    const int jw = j0 + p0 + lane;
    if (disp && lane < npx) disp[(size_t)i * W + jw] = (float)res;
}

// Workgroup -> 64-pixel chunk.  The chunks of a launch form one linear space (view, row, chunk-in-row)
// and workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md), so XCD x takes the x-th contiguous eighth of
// that space: every XCD then streams its own region of the volumes instead of every eighth 48 KB piece
// of the same region.  A store-only kernel with this mapping writes 10 % faster (6.9 vs 6.25 TB/s,
// same box) than with chunks in dispatch order.  The grid is 1-D, padded to a multiple of 8.
// chunk_decode is the general form: workgroup b takes the K consecutive chunks (b >> 3) * K + t, t = 0 .. K-1, of its
// XCD's eighth (the maps-only kernel, which fills a 32 KB table once per workgroup); K = 1 is chunk_of_block.
// maps_groups() is the number of workgroups that covers a launch.  With a tapered tail (n2, n1: maps_span) the
// workgroup's chunks are the span's, still consecutive; chunk_at is the decode of one of them.
__host__ __device__ inline bool chunk_at(int nbx, int H, int nviews, long b, long cl, int &view, int &i, int &bx)
{
    const long nb = (long)nbx * H * nviews;
    const long per = (nb + 7) >> 3;
    const long c = (b & 7) * per + cl;
    if (c >= nb) return false;
    const long rows = (long)nbx * H;
    view = (int)(c / rows);
    const long r = c - (long)view * rows;
    i = (int)(r / nbx);
    bx = (int)(r - (long)i * nbx);
    return true;
}
__host__ __device__ inline bool chunk_decode(int nbx, int H, int nviews, int K, long b, int t, int &view, int &i, int &bx,
                                             int n2 = 0, int n1 = 0)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    long first;
    if (t >= maps_span(per, K, n2, n1, b >> 3, first)) return false;
    return chunk_at(nbx, H, nviews, b, first + t, view, i, bx);
}
__host__ __device__ inline int maps_groups(int nbx, int H, int nviews, int K, int n2 = 0, int n1 = 0)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    return (int)(8 * maps_span_groups(per, K, n2, n1));
}
// cost groups in front of the first tapered one (fused_grid's body), 0 without a taper
__host__ __device__ inline int maps_body_groups(int nbx, int H, int nviews, int K, int n2, int n1)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    (void)maps_span_tails(per, K, n2, n1);
    return n2 + n1 > 0 ? (int)maps_span_body(per, K, n2, n1) : 0;
}
__device__ __forceinline__ bool chunk_of_block(int nbx, int H, int nviews, int &view, int &i, int &bx, long b = -1)
{
    const long nb = (long)nbx * H * nviews;
    const long per = (nb + 7) >> 3;
    if (b < 0) b = blockIdx.x;
    const long c = (b & 7) * per + (b >> 3);
    if (c >= nb) return false;
    const long rows = (long)nbx * H;
    view = (int)(c / rows);
    const long r = c - (long)view * rows;
    i = (int)(r / nbx);
    bx = (int)(r - (long)i * nbx);
    return true;
}

template <int C, int VIEW, bool FULL>
__global__ void __launch_bounds__(NT) k_cost_fast(int H, int W, int D, Tables T, float *__restrict__ vol,
                                                  float *__restrict__ disp, int nbx)
{
    int view, i, bx;
    if (!chunk_of_block(nbx, H, 1, view, i, bx)) return;
    cost_fast_body<C, VIEW, FULL>(H, W, D, T, vol, disp, i, bx);
}

// both views in one launch (no gap / tail between two launches)
template <int C, bool FULL, bool NTS = true>
__global__ void __launch_bounds__(NT) k_cost_fast2(int H, int W, int D, Tables T, float *__restrict__ vol0,
                                                   float *__restrict__ vol1, float *__restrict__ disp0,
                                                   float *__restrict__ disp1, int nbx)
{
    int view, i, bx;
    if (!chunk_of_block(nbx, H, 2, view, i, bx)) return;
    // diagnostic launches only (T.stamp != null, smt_adcensus_diag): the shader-clock and the 100 MHz
    // real-time counters around the first wave's work; their ratio is the clock the kernel ran at
    // (MI355X_MICROARCH.md, DVFS item 6).  Ordinary launches take the null branch and execute no stamp.
    unsigned long long t0 = 0, r0 = 0;
    if (T.stamp) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    if (view == 0) cost_fast_body<C, 0, FULL, NTS>(H, W, D, T, vol0, disp0, i, bx);
    else cost_fast_body<C, 1, FULL, NTS>(H, W, D, T, vol1, disp1, i, bx);
    if (T.stamp && threadIdx.x == 0) {
        unsigned long long *s = T.stamp + 4 * (size_t)blockIdx.x;
        s[0] = t0; s[1] = r0; s[2] = __builtin_amdgcn_s_memtime(); s[3] = __builtin_amdgcn_s_memrealtime();
    }
}

// k_cost_fast2 of pair n with the table workgroups of pair n + 1 spread through its grid (smt_adcensus_compute_batch):
// one launch per pair on one stream -- no second stream, no events between the table and cost kernels -- with the
// table workgroups (VALU / LDS work) running beside the store-bound cost workgroups instead of in front of them.
// Workgroups come in groups of 8 (one per XCD, so a cost workgroup keeps the XCD of its chunk, chunk_of_block): after
// every `every` cost groups one group of table workgroups, tile (p % ptx, p / ptx) of the table launch for the next
// pair's images, writing the OTHER table set (Tn); what does not fit that pattern follows at the end of the grid.
// fused_grid() is the host's side of the same arithmetic.  Measured against the two-stream form (tables of pair
// n + 1 on an internal stream, two event edges per pair): DESIGN.md section 4.
struct FusedGrid { int cgroups, pgroups, every, slots, groups; };
// With a tapered tail (cbody > 0: the cost groups in front of the first tapered one, maps_body_groups) the table groups
// are spread through the body alone, one after every cbody / pgroups cost groups and none in further slots: a table
// tile lasts about as long as a 4-chunk cost workgroup and would undo the taper from inside the tail.  A body with
// fewer groups than there are table groups keeps the placement below.
__host__ __device__ inline FusedGrid fused_grid(int ncost, int nprep, int cbody = 0)
{
    FusedGrid f;
    f.cgroups = ncost >> 3;                                  // ncost is a multiple of 8
    f.pgroups = (nprep + 7) >> 3;
    if (cbody > 0 && f.pgroups > 0 && cbody >= f.pgroups && cbody < f.cgroups) {
        f.every = cbody / f.pgroups;
        f.slots = f.pgroups;
        f.groups = f.cgroups + f.pgroups;
        return f;
    }
    f.every = f.cgroups / (f.pgroups > 0 ? f.pgroups : 1);
    if (f.every < 1) f.every = 1;
    f.slots = f.cgroups / f.every;                           // table groups inside the cost range (>= pgroups unless every == 1)
    f.groups = f.cgroups + (f.pgroups > f.slots ? f.pgroups : f.slots);
    return f;
}
// group g of the fused grid -> (true, table group) or (false, cost group)
__host__ __device__ inline bool fused_decode(const FusedGrid &f, int g, int &idx)
{
    const int period = f.every + 1, inter = f.slots * period;
    if (g < inter) {
        const int q = g / period, r = g - q * period;
        if (r == f.every) { idx = q; return true; }
        idx = q * f.every + r;
        return false;
    }
    const int g2 = g - inter, crest = f.cgroups - f.slots * f.every;
    if (g2 < crest) { idx = f.slots * f.every + g2; return false; }
    idx = f.slots + (g2 - crest);
    return true;
}

template <int C, bool FULL, bool NTS = true>
__global__ void __launch_bounds__(NT, 8) k_cost_fast2p(int H, int W, int D, Tables T, float *__restrict__ vol0,
                                                       float *__restrict__ vol1, float *__restrict__ disp0,
                                                       float *__restrict__ disp1, int nbx, int ncost, int nprep,
                                                       const float *__restrict__ nL, const float *__restrict__ nR, Tables Tn,
                                                       int ptx)
{
    static_assert(PNT == NT, "");
    const FusedGrid f = fused_grid(ncost, nprep);
    int idx;
    const bool table = fused_decode(f, (int)(blockIdx.x >> 3), idx);   // workgroup-uniform
    const int b = idx * 8 + (int)(blockIdx.x & 7);
    if (table) {
        __shared__ uint32_t sLw[PSR][PSW];
        __shared__ uint32_t sRw[PSR][PSW];
        if (b < nprep) prep_tile(nL, nR, H, W, Tn, b % ptx, b / ptx, ptx, sLw, sRw);
        return;
    }
    int view, i, bx;
    if (!chunk_of_block(nbx, H, 2, view, i, bx, b)) return;
    if (view == 0) cost_fast_body<C, 0, FULL, NTS>(H, W, D, T, vol0, disp0, i, bx);
    else cost_fast_body<C, 1, FULL, NTS>(H, W, D, T, vol1, disp1, i, bx);
}

// Maps-only form of k_cost_fast2p / k_cost_fast2 for the pairs of a batch whose volumes no caller can read (every
// pair but the last, smt_adcensus_compute_batch): no volume stores, so the kernel is bound by its arithmetic and LDS
// reads, not by HBM.  MODE_MAPS_RANK reads one 2-byte rank per hypothesis from a 32 KB LDS table instead of two LUT
// entries and a float add, and its WTA is a single wave min; the table is filled once per workgroup, which then walks
// K consecutive chunks of its XCD's range (chunk_decode).  A view whose map is null does no cost work.  With nprep > 0
// the table workgroups of the next pair are placed as in k_cost_fast2p (fused_grid over the maps_groups() cost
// workgroups); they stage their tile in the same LDS array.
// Operands of one chunk of the maps-only kernel: loaded into registers, so that the loads of the workgroup's next chunk
// are in flight while the current one is computed (at 4 workgroups per CU nothing else hides them), then written to
// LDS.  Same entries, clamps and scaling as the staging block of cost_fast_body; the view is a runtime argument.
template <int C, bool FULL>
struct MapsStage {
    static constexpr int NE = (FTJ + 64 * C + 2 * XPAD + NT - 1) / NT;      // staged entries per thread
    uint64_t cen[NE];
    unsigned val[NE];
    Anchor anc;
    unsigned va;
    __device__ __forceinline__ void load(int view, int i, int bx, int W, int Drt, const Tables &T)
    {
        const int D = FULL ? 64 * C : Drt, NX = FTJ + D, j0 = bx * FTJ, tid = threadIdx.x;
        const uint64_t *cenX = T.cenX[view] + (size_t)i * T.WX;
        const uint8_t *extv = T.u8[view ^ 1] + (size_t)i * W;
        const int xbase = (view == 0) ? (j0 - (D - 1)) : j0;
#pragma unroll
        for (int n = 0; n < NE; n++) {
            const int e = tid - (FULL ? 0 : XPAD) + n * NT;
            if (e < NX + (FULL ? 0 : XPAD)) {
                const int x = xbase + e;
                int xc, xv;
                if (view == 0) {
                    xc = x < -3 ? -3 : (x > W - 1 ? W - 1 : x);
                    xv = xc < 0 ? 0 : xc;
                    xc += 3;
                } else {
                    xc = x > W + 3 ? W + 3 : (x < 0 ? 0 : x);
                    xv = x > W - 1 ? W - 1 : (x < 0 ? 0 : x);
                }
                cen[n] = cenX[xc];
                val[n] = extv[xv];
            }
        }
        if (tid < FTJ) {
            const int j = min(j0 + tid, W - 1);
            anc.cen = T.cenA[view][(size_t)i * W + j];
            anc.mask = T.mask[(size_t)i * W + j];
            va = T.u8[view][(size_t)i * W + j];
        }
    }
    template <unsigned VSCALE, int TABN, int NBUF>
    __device__ __forceinline__ void store(MapsLds<C, TABN, NBUF> &ml, int buf, int Drt) const
    {
        const int D = FULL ? 64 * C : Drt, NX = FTJ + D, tid = threadIdx.x;
#pragma unroll
        for (int n = 0; n < NE; n++) {
            const int e = tid - (FULL ? 0 : XPAD) + n * NT;
            if (e < NX + (FULL ? 0 : XPAD)) {
                ml.st[buf].cenx[XPAD + e] = cen[n];
                ml.st[buf].valx[XPAD + e] = (uint16_t)(VSCALE * val[n]);
            }
        }
        if (tid < FTJ) { ml.st[buf].anc[tid] = anc; ml.st[buf].vala[tid] = (uint16_t)(VSCALE * va); }
    }
};

template <int C, bool FULL, int MODE>
__global__ void __launch_bounds__(NT) k_cost_maps2p(int H, int W, int D, Tables T, float *__restrict__ disp0,
                                                    float *__restrict__ disp1, int nbx, int K, int ncost, int nprep,
                                                    const float *__restrict__ nL, const float *__restrict__ nR,
                                                    Tables Tn, int ptx, int n2, int n1, int cbody)
{
    static_assert(PNT == NT, "");
    constexpr int TABN = MapsCfg<MODE>::TABN, NBUF = MapsCfg<MODE>::NBUF;
    static_assert(2 * PSR * PSW * 4 <= TABN * 2 && 320 * 4 <= TABN * 2, "");
    __shared__ MapsLds<C, TABN, NBUF> lds;
    uint16_t *s_tab = lds.tab;
    long b = blockIdx.x;
    if (nprep > 0) {
        const FusedGrid f = fused_grid(ncost, nprep, cbody);
        int idx;
        const bool table = fused_decode(f, (int)(blockIdx.x >> 3), idx);   // workgroup-uniform
        b = idx * 8 + (int)(blockIdx.x & 7);
        if (table) {
            uint32_t (*sw)[PSW] = (uint32_t (*)[PSW])s_tab;
            if (b < nprep) prep_tile(nL, nR, H, W, Tn, (int)b % ptx, (int)b / ptx, ptx, sw, sw + PSR);
            return;
        }
    }
    const int tid = threadIdx.x;
    if (MODE == MODE_MAPS_RANK) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        for (int e = tid; e < RANK_N / 8; e += NT) ((u32x4 *)s_tab)[e] = ((const u32x4 *)T.rank)[e];
    } else {
        for (int e = tid; e < 320; e += NT) ((float *)s_tab)[e] = T.lut[e];
    }
    // the workgroup's chunks: c0 .. c0 + m - 1 of its slice (maps_span; m < K in a tapered tail)
    long c0;
    const int m = maps_span((((long)nbx * H * 2) + 7) >> 3, K, n2, n1, b >> 3, c0);
    // the workgroup's next chunk at or after t whose map is requested (workgroup-uniform), K when there is none
    auto next = [&](int t, int &view, int &i, int &bx) {
        for (; t < m; t++) {
            if (!chunk_at(nbx, H, 2, b, c0 + t, view, i, bx)) return K;
            if (view == 0 ? disp0 : disp1) return t;
        }
        return K;
    };
    MapsStage<C, FULL> st;
    int view = 0, i = 0, bx = 0;
    int t = next(0, view, i, bx);
    if (t < K) st.load(view, i, bx, W, D, T);
    // With one staging set a barrier must follow the reads of chunk t before chunk t+1 is written.  With two, the barrier
    // after the write of chunk t+1 is only passed once every wave has finished chunk t-1, the last reader of that set.
    bool first = true;
    int buf = 0;
    while (t < K) {
        if (NBUF == 1 && !first) __syncthreads();
        first = false;
        st.template store<MODE == MODE_MAPS_RANK ? 64u : 4u>(lds, buf, D);
        __syncthreads();
        const int cv = view, ci = i, cbx = bx;
        t = next(t + 1, view, i, bx);
        if (t < K) st.load(view, i, bx, W, D, T);                       // in flight during this chunk's arithmetic
        if (cv == 0) cost_fast_body<C, 0, FULL, true, MODE>(H, W, D, T, nullptr, disp0, ci, cbx, &lds, buf);
        else cost_fast_body<C, 1, FULL, true, MODE>(H, W, D, T, nullptr, disp1, ci, cbx, &lds, buf);
        buf = NBUF == 1 ? 0 : buf ^ 1;
    }
}

// One flush of the key ring (shared_run_flush_range's columns lo .. hi of row i, run [S, E]): complete keys go to the map,
// partial ones to the handle's key map with one agent-scope atomic min each; the slots are reset.
template <int C, bool GROUPED>
__device__ __forceinline__ void shared_flush(unsigned long long *ring, int i, int W, int D, int lo, int hi, int S, int E,
                                             int idhi, float *__restrict__ dispR, unsigned long long *__restrict__ keys)
{
    for (int c = lo + (int)threadIdx.x; c <= hi; c += NT) {
        const int s = c & (SH_RING - 1);
        unsigned long long k = ring[s];
        ring[s] = SH_NOKEY;
        if (s < shared_ring_spill(C, GROUPED)) { k = min(k, ring[SH_RING + s]); ring[SH_RING + s] = SH_NOKEY; }
        const size_t p = (size_t)i * W + c;
        if (shared_complete(c, S, E, D, idhi)) dispR[p] = (float)(unsigned)k;
        else if (k != SH_NOKEY && SMT_SHARED_KNOCKOUT != 2) atomicMin(&keys[p], k);
    }
}

// ---- the shared form: runs walked in one pass ----------------------------------------------------------------------
// LDS of k_cost_maps_shared: the table area of MapsLds (the LUT; a table workgroup's tile) and ONE staging set that holds
// a whole run of up to SH_RUN chunks: its anchors and the ext entries S-(D-1)-XPAD .. E+XPAD.
template <int C> struct RunLds {
    static constexpr int NA = SH_RUN * FTJ;                  // anchors of a run
    static constexpr int NXR = NA + 64 * C + 2 * XPAD;       // ext entries of a run
    uint16_t tab[PREP_LDS_U16];
    Anchor anc[NA];
    uint64_t cenx[NXR];
    uint16_t valx[NXR];
    uint16_t vala[NA];
};

// Operands of one run, through registers like MapsStage: same entries, clamps and x4 value scaling, VIEW 0.  Unlike
// MapsStage's, the loads of a workgroup's second run (a row change inside it, or K > SH_RUN) are issued behind the first
// run's walk, not held across it, so only the barrier and the flush cover their latency.
template <int C, bool FULL>
struct RunStage {
    static constexpr int NE = (RunLds<C>::NXR + NT - 1) / NT;               // staged entries per thread
    static_assert(RunLds<C>::NA <= NT, "one anchor per thread");
    uint64_t cen[NE];
    unsigned val[NE];
    Anchor anc;
    unsigned va;
    __device__ __forceinline__ void load(int i, int S, int n, int W, int Drt, const Tables &T)
    {
        const int D = FULL ? 64 * C : Drt, NX = n * FTJ + D, tid = threadIdx.x;
        const uint64_t *cenX = T.cenX[0] + (size_t)i * T.WX;
        const uint8_t *extv = T.u8[1] + (size_t)i * W;
        const int xbase = S - (D - 1);
#pragma unroll
        for (int m = 0; m < NE; m++) {
            const int e = tid - (FULL ? 0 : XPAD) + m * NT;
            if (e < NX + (FULL ? 0 : XPAD)) {
                const int x = xbase + e;
                int xc = x < -3 ? -3 : (x > W - 1 ? W - 1 : x);
                const int xv = xc < 0 ? 0 : xc;
                xc += 3;
                cen[m] = cenX[xc];
                val[m] = extv[xv];
            }
        }
        if (tid < n * FTJ) {
            const int j = min(S + tid, W - 1);
            anc.cen = T.cenA[0][(size_t)i * W + j];
            anc.mask = T.mask[(size_t)i * W + j];
            va = T.u8[0][(size_t)i * W + j];
        }
    }
    __device__ __forceinline__ void store(RunLds<C> &ml, int n, int Drt) const
    {
        const int D = FULL ? 64 * C : Drt, NX = n * FTJ + D, tid = threadIdx.x;
#pragma unroll
        for (int m = 0; m < NE; m++) {
            const int e = tid - (FULL ? 0 : XPAD) + m * NT;
            if (e < NX + (FULL ? 0 : XPAD)) {
                ml.cenx[XPAD + e] = cen[m];
                ml.valx[XPAD + e] = (uint16_t)(4u * val[m]);
            }
        }
        if (tid < n * FTJ) { ml.anc[tid] = anc; ml.vala[tid] = (uint16_t)(4u * va); }
    }
};

// The left pass of the shared form over a staged run of n chunks from left column S of row i: the left map, and every
// shareable cost published as a key to the ring slot of its right column.  Wave w walks the 16 n consecutive pixels
// from S + 16 n w in one pass; lane l owns the hypotheses d = l*C .. l*C+C-1 of each.  Per pixel: the C costs
// lut[4 AD] + lut[256 + census] from the anchor entry (read at a wave-uniform LDS address) and the lane's register
// window of C ext entries, which takes in one new entry per pixel; the WTA, a wave minimum over the cost bit patterns
// (costs are >= +0, so unsigned order is float order), the first lane that holds it and that lane's first such
// hypothesis, i.e. the first strict minimum; then one LDS 64-bit atomic min per hypothesis that shared_publishes().
// The window and the four LDS address registers carry through the walk; the interior and all-in tests are taken per
// wave (per 16-pixel segment inside one loop, the four variants' loop invariants are all live at once and the kernel
// spills).  cost_fast_body computes the same costs and winners chunk by chunk for the kernels that do not share.
template <int C, bool FULL>
__device__ __forceinline__ void shared_run_walk(int H, int W, int Drt, float *__restrict__ disp, int i, int S, int n,
                                                const RunLds<C> *ml, unsigned long long *ring, int pubhi)
{
    const int D = FULL ? 64 * C : Drt;
    // The vector-instruction trims below (the winner's v_writelane, the untied first DPP step, 32-bit window values, the
    // stepped ring address) are taken by the D = 192 kernel only: it is the form they were measured to pay in.  At
    // C = 2 the same four measured slower at 720p x 128 in every run, with the stepped address (64 -> 70 VGPRs, 8 -> 7
    // waves per SIMD) and without it, and the other forms gain scratch with the stepped address; those compile to the
    // code they had.  The stepped address has since become one base per group of C pixels
    // (GROUPED, below) in a group loop without per-pixel exits (GROUP_LOOP), again in the D = 192 kernel only: at C = 2
    // the two together gained 4x the run-to-run spread at 720p x 128 and cost a wave per SIMD.
    constexpr bool TRIM = C == 3 && FULL;
    const Anchor *s_anc = ml->anc;
    const uint16_t *s_vala = ml->vala;
    const uint64_t *s_cenx = ml->cenx + XPAD;                // entry e in [-XPAD, n * FTJ + D + XPAD): column S-(D-1)+e
    const uint16_t *s_valx = ml->valx + XPAD;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = wid * (FPW * n);                          // the wave's first pixel in the run
    const int dlr = lane * C;                                // first hypothesis of this lane
    const int dl = (FULL || dlr < D) ? dlr : 0;              // lanes entirely past D shadow lane 0
    bool ok[C];
#pragma unroll
    for (int k = 0; k < C; k++) ok[k] = FULL || (dlr + k < D);
    // ext entry of (pixel p, hypothesis dl+k): p + (D-1) - dl - k.  With E(n) = staged entry e0 + n, pixel q needs
    // E(q-k), k = 0..C-1: the C live entries sit in a register ring R[n mod C] = E(n), and the pixel loop is unrolled by
    // C so that every ring index is a compile-time constant.  It starts with E(0), E(-1), ..., E(-(C-1)).
    const int e0 = p0 + (D - 1) - dl;
    uint64_t rc[C];
    unsigned rv[C];
#pragma unroll
    for (int k = 0; k < C; k++) {
        const int slot = ((-k % C) + C) % C;
        rc[slot] = s_cenx[e0 - k];
        rv[slot] = s_valx[e0 - k];
    }
#pragma unroll
    for (int k = 0; k < C; k++) if constexpr (TRIM) asm("" : "+v"(rv[k]));   // 32-bit values from here on (see the walk)
    const char *lutA = (const char *)ml->tab;
    const float *lutC = (const float *)ml->tab + 256;
    int res = 0;
    const int jw0 = S + p0;
    const int npx = min(FPW * n, W - jw0);                   // uniform; may be <= 0
    typedef __attribute__((address_space(3))) unsigned long long *lds_key_p;
    typedef const __attribute__((address_space(3))) uint64_t *lds_u64_p;
    typedef const __attribute__((address_space(3))) uint16_t *lds_u16_p;
    const lds_key_p ring3 = (lds_key_p)ring;
    // wave-uniform anchor addresses and the lane's ext addresses in VGPRs, advanced once per group of C pixels
    uint32_t anc_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) Anchor *)(s_anc + p0);
    uint32_t val_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint16_t *)(s_vala + p0);
    uint32_t nx_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint64_t *)(s_cenx + e0);
    uint32_t nv_a = (uint32_t)(size_t)(const __attribute__((address_space(3))) uint16_t *)(s_valx + e0);
    asm volatile("" : "+v"(anc_a), "+v"(val_a), "+v"(nx_a), "+v"(nv_a));
    // byte offset in the ring of slot shared_ring_base(t, C) of the group's first pixel, t = j - dl: advanced by C slots
    // per group and wrapped, the group's other pixels at immediate offsets from it (shared_ring_slot), where computing it
    // from the column takes two vector instructions per pixel, at the price of one more live register
    constexpr bool GROUPED = shared_ring_grouped(C, FULL ? 64 * C : 0);
    constexpr bool GROUP_LOOP = shared_walk_groups(C, FULL ? 64 * C : 0);
    static_assert(GROUP_LOOP || !GROUPED, "");
    const uint32_t ring_b = (uint32_t)(size_t)ring3;
    uint32_t ra = 8u * (uint32_t)shared_ring_base(jw0 - dl, C);

    auto walk = [&](auto masked_tag, auto allin_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        constexpr bool ALLIN = decltype(allin_tag)::value;
        // pixel q = g + u of the walk; u = q mod C is a constant once the group is unrolled (the register window's
        // indices and the immediate offsets from the group's addresses depend on it)
        auto pixel = [&](const int u, const int q) __attribute__((always_inline)) {
            Anchor a;
            if (MASKED) {                                            // one ds_read_b128
                typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
                const u64x2 v = *(const __attribute__((address_space(3))) u64x2 *)(size_t)(anc_a + 16u * u);
                a.cen = v.x; a.mask = v.y;
            }
            else { a.cen = *(lds_u64_p)(size_t)(anc_a + 16u * u); a.mask = 0; }
            const unsigned va = *(lds_u16_p)(size_t)(val_a + 2u * u);
            // entry that joins the ring for the next pixel (always inside the staged range)
            const uint64_t nc = *(lds_u64_p)(size_t)(nx_a + 8u * (unsigned)(u + 1));
            const unsigned nv = *(lds_u16_p)(size_t)(nv_a + 2u * (unsigned)(u + 1));
            float c[C];
            unsigned key[C];
#pragma unroll
            for (int k = 0; k < C; k++) {
                const int slot = (((u - k) % C) + C) % C;            // E(q-k) with q = u (mod C)
                uint64_t x = a.cen ^ rc[slot];
                if (MASKED) x &= a.mask;
                const int hd = __popcll(x);
                const unsigned ad4 = __builtin_amdgcn_sad_u16(va, rv[slot], 0u);   // 4*|va - vx|
                c[k] = *(const float *)(lutA + ad4) + lutC[hd];
                key[k] = ok[k] ? __float_as_uint(c[k]) : 0xFFFFFFFFu;
            }
            unsigned ml0 = key[0];
#pragma unroll
            for (int k = 1; k < C; k++) ml0 = min(ml0, key[k]);
            // ml0 is compared against the minimum below, so the untied form saves its copy per pixel
            unsigned m;
            if constexpr (TRIM) m = wave_min_u32_untied(ml0);
            else m = wave_min_u32(ml0);
            const unsigned long long b = __ballot(ml0 == m);
            const int first = __builtin_ctzll(b);
            int kk = C - 1;
#pragma unroll
            for (int k = C - 2; k >= 0; k--)
                if ((unsigned)__builtin_amdgcn_readlane((int)key[k], first) == m) kk = k;
            const int wd = first * C + kk;           // wave-uniform
            // lane q keeps pixel q's winner (q <= 63): one v_writelane where (lane == q) ? wd : res took a
            // compare and a move under a saved exec mask.  This compiler has no writelane builtin, hence the
            // statement.  Both sources are scalar and gfx9 reads one SGPR per vector instruction, so the lane
            // goes in m0.  No wait states are needed: on gfx9 only a lane select in an SGPR that a vector
            // instruction wrote has a hazard, and m0 is written by the s_mov.  The compiler warns about the m0
            // clobber (-Winline-asm) at each instantiation; the kernel uses m0 nowhere else.
            if constexpr (TRIM)
                asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(res) : "s"(__builtin_amdgcn_readfirstlane(wd)), "s"(q) : "m0");
            else res = (lane == q) ? wd : res;
            if constexpr (SMT_SHARED_KNOCKOUT != 1) {
                const int tcol = (jw0 + q) - dl;                     // right column of hypothesis k = 0
                lds_key_p rp;
                if constexpr (GROUPED) rp = (lds_key_p)(size_t)(ring_b + ra) + u;   // the group's base: immediate offsets
                else rp = ring3 + shared_ring_base(tcol, C);
#pragma unroll
                for (int k = 0; k < C; k++)
                    if (ok[k] && (ALLIN || shared_publishes(jw0 + q, tcol - k, W, pubhi)))
                        (void)__hip_atomic_fetch_min(rp + (C - 1 - k), shared_key(__float_as_uint(c[k]), dl + k),
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            // the new entry replaces the one that just left the window.  The value is made a 32-bit one here:
            // carried round the loop as the 16 bits it was loaded as, it is zero-extended again at every use
            // (one v_and per pixel), though ds_read_u16 already returned it so
            unsigned nv32 = nv;
            if constexpr (TRIM) asm("" : "+v"(nv32));
            rc[(u + 1) % C] = nc; rv[(u + 1) % C] = nv32;
        };
        if constexpr (GROUP_LOOP) {
            // whole groups without a per-pixel exit -- one basic block, so the group's addresses are advanced once and a
            // pixel's arithmetic can fill the wait states of its neighbour's DPP chain -- then the at most C-1 pixels left
            // over, from the same base
            int g = 0;
#pragma unroll 1
            for (; g + C <= npx; g += C) {
#pragma unroll
                for (int u = 0; u < C; u++) pixel(u, g + u);
                anc_a += 16u * C; val_a += 2u * C;
                nx_a += 8u * C; nv_a += 2u * C;
                if constexpr (GROUPED) ra = (ra + 8u * C) & (8u * SH_RING - 1u);
            }
#pragma unroll
            for (int u = 0; u < C - 1; u++)
                if (g + u < npx) pixel(u, g + u);
        } else {
#pragma unroll 1
            for (int g = 0; g < npx; g += C) {
#pragma unroll
                for (int u = 0; u < C; u++) {
                    const int q = g + u;
                    if (q < npx) pixel(u, q);
                }
                anc_a += 16u * C; val_a += 2u * C;
                nx_a += 8u * C; nv_a += 2u * C;
            }
        }
    };
    // per wave.  interior: every pixel has all 63 taps inside the image, so the tap mask is all ones and the AND per
    // hypothesis is dropped (bit 63 is 0 in every table entry); all-in: every (pixel, hypothesis) publishes
    // (pubhi <= W-4), no per-hypothesis column test
    const bool interior = (i >= 4) && (i < H - 4) && jw0 >= 3 && jw0 + npx - 1 <= W - 4;
    const bool allin = jw0 - (D - 1) >= 3 && jw0 + npx - 1 <= pubhi;
    if (allin) { if (interior) walk(std::false_type{}, std::true_type{}); else walk(std::true_type{}, std::true_type{}); }
    else { if (interior) walk(std::false_type{}, std::false_type{}); else walk(std::true_type{}, std::false_type{}); }
    if (lane < npx) disp[(size_t)i * W + jw0 + lane] = (float)res;
}

// Right-view cost of (i, j', d) straight from the tables, with the arithmetic of cost_fast_body's VIEW 1: the census
// index clamped to W+3, the value index to W-1, the anchor's tap mask, lut[ad] + lut[256 + hd].  j' + d >= 0.
__device__ __forceinline__ unsigned long long shared_edge_key(const Tables &T, int i, int W, uint64_t acen, uint64_t amask,
                                                              int va, int x, int d)
{
    const int xc = x > W + 3 ? W + 3 : x, xv = x > W - 1 ? W - 1 : x;
    const int hd = __popcll((acen ^ T.cenX[1][(size_t)i * T.WX + xc]) & amask);
    const int vx = T.u8[0][(size_t)i * W + xv];
    const int ad = va > vx ? va - vx : vx - va;
    const float c = T.lut[ad] + T.lut[256 + hd];
    return shared_key(__float_as_uint(c), d);
}

// The auxiliary items of a shared launch (rules: shared_aux_decode and the functions next to it).  None uses LDS.
// Conversion: partial keys -> map entries, the consumed keys reset for the pair after the next.  All 8 loads of a
// thread are issued before the first store.
__device__ __forceinline__ void shared_conv_item(unsigned long long *__restrict__ keys, float *__restrict__ dispR, long N,
                                                 int item)
{
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    constexpr int NI = SH_CONV_PX / (2 * NT);
    u64x2 k[NI];
    // step `it` takes the keys p0 + 512 it and the one behind it (shared_conv_px is linear in `it`)
    long p0;
    (void)shared_conv_px(item, 0, (int)threadIdx.x, N, p0);
    const long left = N - p0;                                              // <= 0: nothing for this thread
    unsigned long long *__restrict__ kp = keys + p0;
    float *__restrict__ dp = dispR + p0;
#pragma unroll
    for (int it = 0; it < NI; it++) {
        constexpr int ST = 2 * NT;
        k[it].x = k[it].y = SH_NOKEY;
        if (it * ST + 1 < left) k[it] = *reinterpret_cast<const u64x2 *>(kp + it * ST);   // p is even: 16-byte aligned
        else if (it * ST < left) k[it].x = kp[it * ST];
    }
#pragma unroll
    for (int it = 0; it < NI; it++) {
        constexpr int ST = 2 * NT;
        if (k[it].x != SH_NOKEY) { dp[it * ST] = (float)(unsigned)k[it].x; kp[it * ST] = SH_NOKEY; }
        if (k[it].y != SH_NOKEY) { dp[it * ST + 1] = (float)(unsigned)k[it].y; kp[it * ST + 1] = SH_NOKEY; }
    }
}

// Edge hypotheses of this pair from its tables T (read-only in this launch: the table workgroups write the other set).
__device__ __forceinline__ void shared_edge_item(const Tables &T, int H, int W, int D, float *__restrict__ dispR,
                                                 unsigned long long *__restrict__ keys, int item)
{
    const int ncol = shared_edge_col_items(H, W, D);
    if (item < ncol) {
#pragma unroll 1
        for (int it = 0; it < SH_EDGE_PX / NT; it++) {
            int i, c;
            if (!shared_edge_px(item, it, (int)threadIdx.x, H, W, D, i, c)) return;
            const size_t p = (size_t)i * W + c;
            const uint64_t acen = T.cenA[1][p], amask = T.mask[p];
            const int va = T.u8[1][p];
            int lo, hi;
            shared_edge_range(c, W, D, lo, hi);
            unsigned long long k = SH_NOKEY;
            for (int d = lo; d <= hi; d++) k = min(k, shared_edge_key(T, i, W, acen, amask, va, c + d, d));
            if (c > W - 4) dispR[p] = (float)(unsigned)k;                  // nothing is published to the last three
            else if (k != SH_NOKEY && SMT_SHARED_KNOCKOUT != 2) atomicMin(&keys[p], k);
        }
        return;
    }
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int it = 0; it < SH_EDGE0_PX / 4; it++) {                         // columns 0..2
        int i, c;
        if (!shared_edge0_px(item - ncol, it, (int)(threadIdx.x >> 6), H, i, c)) return;
        const size_t p = (size_t)i * W + c;
        const uint64_t acen = T.cenA[1][p], amask = T.mask[p];
        const int va = T.u8[1][p];
        int lo, hi;
        shared_edge_range(c, W, D, lo, hi);
        unsigned long long k = SH_NOKEY;
        for (int d = lo + lane; d <= hi; d += 64) k = min(k, shared_edge_key(T, i, W, acen, amask, va, c + d, d));
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) k = min(k, (unsigned long long)__shfl_xor((long long)k, s));
        if (lane == 0) dispR[p] = (float)(unsigned)k;
    }
}

// Shared maps-only form: both maps of a pair from one cost evaluation per shareable hypothesis.  A cost workgroup takes
// K consecutive chunks of the left view alone (shared_wg_chunks: chunk_decode's, in its XCD's eighth) and publishes the
// keys of the right columns [3, pubhi] to its ring.  Per run (shared_run_len) of n <= SH_RUN chunks: stage once,
// barrier, every wave walks its quarter of the run and publishes, barrier, flush every column the run published to
// (shared_run_flush_range) -- complete keys to the map, partial ones to the key map, slots reset.  The next run's
// staging store follows the flush, and the barrier behind it frees the ring and shows the staged set.  A column yields
// one key per run and the merges are minima, so their order does not matter.  The launch's edge items merge the edge
// hypotheses into the same key map; the conversion items of the NEXT shared launch (or k_shared_convert) turn the merged
// keys into map entries.  The workgroups of the fused grid's table class take the auxiliary items (shared_aux_decode):
// table tiles as in k_cost_maps2p, conversion items of the previous pair (ckeys -> cdisp), edge items of this pair.
#ifndef SMT_SHARED_MIN_WAVES
#define SMT_SHARED_MIN_WAVES 7     // waves per SIMD the register allocation must allow; measured 1 / 7 / 8: DESIGN.md section 4
#endif
template <int C, bool FULL>
__global__ void __launch_bounds__(NT, SMT_SHARED_MIN_WAVES) k_cost_maps_shared(int H, int W, int D, Tables T, float *__restrict__ disp0,
                                                         float *__restrict__ disp1, unsigned long long *__restrict__ keys,
                                                         int nbx, int K, int pubhi, int ncost, int nprep,
                                                         const float *__restrict__ nL, const float *__restrict__ nR,
                                                         Tables Tn, int ptx, int nconv, int nedge,
                                                         unsigned long long *__restrict__ ckeys, float *__restrict__ cdisp,
                                                         int n2, int n1, int cbody)
{
    static_assert(PNT == NT && NT == 256, "");
    static_assert(2 * PSR * PSW * 4 <= PREP_LDS_U16 * 2 && 320 * 4 <= PREP_LDS_U16 * 2, "");
    __shared__ RunLds<C> lds;
    __shared__ unsigned long long ring[SH_RING_N];
    long b;
    {
        const FusedGrid f = fused_grid(ncost, nprep + nconv + nedge, cbody);
        int idx;
        const bool table = fused_decode(f, (int)(blockIdx.x >> 3), idx);   // workgroup-uniform
        b = idx * 8 + (int)(blockIdx.x & 7);
        if (table) {                                                       // an auxiliary item, or none
            int item;
            const int kind = shared_aux_decode((int)b, nprep, nconv, nedge, item);
            if (kind == AUX_PREP) {
                uint32_t (*sw)[PSW] = (uint32_t (*)[PSW])lds.tab;
                prep_tile(nL, nR, H, W, Tn, item % ptx, item / ptx, ptx, sw, sw + PSR);
            } else if (kind == AUX_CONV) shared_conv_item(ckeys, cdisp, (long)H * W, item);
            else if (kind == AUX_EDGE) shared_edge_item(T, H, W, FULL ? 64 * C : D, disp1, keys, item);
            return;
        }
    }
    const int tid = threadIdx.x;
    int i = 0, bx = 0;
    int left = shared_wg_chunks(nbx, H, K, b, i, bx, n2, n1);              // workgroup-uniform
    if (left == 0) return;
    for (int e = tid; e < 320; e += NT) ((float *)lds.tab)[e] = T.lut[e];
    const int Dd = FULL ? 64 * C : D;
    const int idhi = shared_id_hi(W, Dd);
    for (int e = tid; e < SH_RING_N; e += NT) ring[e] = SH_NOKEY;
    RunStage<C, FULL> st;
    int n = shared_run_len(nbx, bx, left);
    st.load(i, FTJ * bx, n, W, D, T);
    for (;;) {
        st.store(lds, n, D);
        __syncthreads();                                                   // the set is staged; the ring is free
        const int ci = i, cS = FTJ * bx, cn = n;
        left -= n; bx += n;
        if (bx == nbx) { bx = 0; i++; }
        n = shared_run_len(nbx, bx, left);
        shared_run_walk<C, FULL>(H, W, D, disp0, ci, cS, cn, &lds, ring, pubhi);
        // A second run (a row change inside the workgroup, or K > SH_RUN) loads behind the walk, in flight across the
        // barrier and the flush: held across the walk its 11 registers would push the walk into scratch.  At K = 4
        // about one workgroup in ten has a second run; the exposed latency at K > 4 has not been measured.
        if (n > 0) st.load(i, FTJ * bx, n, W, D, T);
        __syncthreads();                                                   // every wave has published the run
        const int cE = cS + FTJ * cn - 1;
        int lo, hi;
        shared_run_flush_range(cS, cE, Dd, pubhi, lo, hi);
        shared_flush<C, shared_ring_grouped(C, FULL ? 64 * C : 0)>(ring, ci, W, Dd, lo, hi, cS, cE, idhi, disp1, keys);
        if (n <= 0) break;
    }
}

// The conversion items of a pair that no later shared launch carries (the last shared pair of a batch loop, or every
// pair under SMT_SHARED_FINISH=apart): shared_conv_items() workgroups.
__global__ void __launch_bounds__(NT) k_shared_convert(unsigned long long *__restrict__ keys, float *__restrict__ dispR, long N)
{
    shared_conv_item(keys, dispR, N, (int)blockIdx.x);
}

// Store-only twin of k_cost_fast2<C, true>: the same grid, workgroup -> chunk order and streaming stores
// of 64*C*4 bytes per pixel-wave, no tables, no arithmetic.  What it reaches on the handle's own volumes
// is the ceiling the memory system gives this store pattern in this process (smt_adcensus_diag).
template <int C>
__global__ void __launch_bounds__(NT) k_store_only2(int H, int W, float *__restrict__ vol0,
                                                    float *__restrict__ vol1, int nbx)
{
    constexpr int D = 64 * C;
    int view, i, bx;
    if (!chunk_of_block(nbx, H, 2, view, i, bx)) return;
    float *vol = view ? vol1 : vol0;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j0 = bx * FTJ, p0 = wid * FPW;
    const int npx = min(FPW, W - (j0 + p0));
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(vol + ((size_t)i * W + j0 + p0) * D), 0, (npx > 0 ? npx : 0) * D * 4, 0x00020000);
    const unsigned ooff = (unsigned)(lane * C) * 4u;
    unsigned osoff = 0;
    float x[C];
#pragma unroll
    for (int k = 0; k < C; k++) x[k] = (float)(lane + k);
    for (int q = 0; q < npx; q++) {
        st_stream<C>(orsrc, ooff, osoff, x);
        osoff += (unsigned)D * 4u;
        x[0] += 1.0f;
    }
}

// WTA over an existing volume: one wave per pixel, lane owns C consecutive d (one vector load when
// D == 64*C), DPP argmin.
template <int C, bool FULL>
__global__ void __launch_bounds__(NT) k_wta(const float *__restrict__ vol, int N, int D,
                                            float *__restrict__ disp)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= N) return;
    const int dl = lane * C;
    const float *c = vol + (size_t)p * D + dl;
    float v[C];
    if (FULL) {
        const vecf<C> x = *reinterpret_cast<const vecf<C> *>(c);
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = x.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = (dl + k < D) ? c[k] : INFINITY;
    }
    const int wd = wave_wta<C, FULL>(v, dl, D);
    if (lane == 0) disp[p] = (float)wd;
}

}  // namespace

thread_local int g_smt_last_hip = 0;

// Chains of the chained batch schedule (chain_plan).  Three at the most: a process has four hardware queues here and
// the caller's stream is one of them.
constexpr int SMT_MAX_CHAINS = 3;
constexpr int SMT_CHAINS_DEFAULT = 2;
// The chained schedule is the default of smt_adcensus_compute_batch wherever the fused one would be (batch_schedule).
constexpr bool SMT_CHAINED_DEFAULT = true;
struct ChainState {
    long n_pairs;        // pairs issued on this chain ([0]: and by every schedule that is not chained)
    bool conv_pending;
    int conv_map;        // index into skeys[]
    float *conv_dR;
};
// Table set and key map that chain c's pair number n (the chain's own counter) uses: TS[] / skeys[] index.
static inline int chain_slot(int c, long n) { return 2 * c + (int)(n & 1); }

struct smt_adcensus {
    int device;          // HIP device the handle lives on
    int H, W, D;
    float sigmaC, sigmaS;
    hipStream_t stream;
    float *vol[2];
    Tables T;            // table set used by the pair being issued (= TS[chain_slot(cur, its chain's n_pairs)])
    // Two sets per chain (chain c owns 2c and 2c+1): the tables of a chain's next pair are built while its pair runs.
    // Chain 0 is the state of every schedule but the chained one (smt_adcensus_compute, schedules 0 .. 2, host-fed flow).
    Tables TS[2 * SMT_MAX_CHAINS];
    hipStream_t prep_stream;                 // internal, non-blocking: schedule 1's table stream and chain 1's stream
    hipStream_t chain2_stream;               // internal, non-blocking: chain 2's stream
    hipEvent_t in_ready, prep_done[2], cost_done[2];
    hipEvent_t fork_ev, join_ev[SMT_MAX_CHAINS];   // the chained schedule's edges per call (chain_plan); join_ev[0] unused
    ChainState chain[SMT_MAX_CHAINS];
    // The chain whose state the pair being issued uses, and the internal stream each chain runs on in the call being
    // issued (0: the caller's stream).  All 0 outside adcensus_batch_chained.
    int cur, chain_on[SMT_MAX_CHAINS];
    // The pair being issued runs beside another chain's launch, which fills its drain: the tapered tail's default rule
    // is off for it (maps_taper, chain_taper).  False outside adcensus_batch_chained.
    bool beside;
    hipEvent_t *ev;      // SMT_TIMING_SLOTS * 4, lazily created
    bool timing;
    bool force_generic;  // test hook: route D%64==0 through the generic kernel too
    long n_timed;        // pairs recorded since timing was (re-)enabled
    long n_seen;         // pairs processed since timing was (re-)enabled
    int timing_stride;   // every timing_stride-th pair is recorded
    bool *ev_merged;     // slot recorded 3 events (tables end == cost start, one stream)
    bool plain_stores;   // both-views cost kernel with ordinary instead of streaming stores (chosen at create)
    float store_mode_ms[2];   // calibration: kernel ms with streaming / plain stores (0: not calibrated)
    int place_tries;     // candidate volume pairs tried by place_volumes
    float place_ms;      // store-only time of the pair that was kept (0: no search)
    // Two [H][W] key maps of the shared maps-only form per chain; a chain's pair n merges into map chain_slot(c, n).
    // All are SH_NOKEY after create and whenever no conversion is pending.  chain[c].conv_pending: the shared pair the
    // chain issued last has its partial keys in skeys[conv_map], still to be converted into its right map conv_dR -- by
    // the chain's next shared launch, or by flush_conversion().  Never true when an entry point returns (the caller may
    // free its maps).
    unsigned long long *skeys[2 * SMT_MAX_CHAINS];
    // Deferred volumes of a batch's last pair (smt_adcensus_compute_batch, smt_adcensus_volume).  vol_lent: a caller
    // has been given a volume pointer, so every batch from then on writes its last pair's volumes itself.
    // vol_pending: the last pair took the maps-only path and its volumes are still to be written, by the both-views
    // cost kernel on T.  All that launch needs stays in the handle until the next compute replaces the pending state:
    // T is the pair's table set (nothing rebuilds it; the quirk state of the pair is in the tables' contents, and
    // smt_adcensus_set_quirks changes only edge_col, which the table kernels alone read) and plain_stores is fixed at
    // create.
    bool vol_lent, vol_pending;
    // Workgroups that one slice's CUs (an eighth of the device) hold at a time, of the maps-only kernel this handle's D
    // launches: [0] k_cost_maps_shared, [1] k_cost_maps2p float, [2] k_cost_maps2p rank.  From the occupancy query at
    // create; 0 (unknown, or D > 256) leaves the tapered tail's default rule off (maps_taper).
    int maps_resident[3];
};

SMT_API const char *smt_strerror(int s)
{
    switch (s) {
    case SMT_OK: return "ok";
    case SMT_ERR_ARG: return "invalid argument";
    case SMT_ERR_HIP: return "HIP runtime error";
    case SMT_ERR_ALLOC: return "device allocation failed";
    case SMT_ERR_DOMAIN: return "image values outside the integer 0..255 domain";
    case SMT_ERR_REF_UB: return "reference behaviour undefined for these inputs";
    case SMT_ERR_STATE: return "call order violated";
    default: return "unknown status";
    }
}
SMT_API int smt_version(void) { return SMT_VERSION; }
SMT_API int smt_last_hip_error(void) { return g_smt_last_hip; }
SMT_API int smt_device_count(int *n)
{
    if (!n) return SMT_ERR_ARG;
    SMT_HIP(hipGetDeviceCount(n));
    return SMT_OK;
}
SMT_API int smt_set_device(int d) { SMT_HIP(hipSetDevice(d)); return SMT_OK; }
SMT_API int smt_malloc(void **p, size_t n)
{
    if (!p) return SMT_ERR_ARG;
    hipError_t e = hipMalloc(p, n ? n : 1);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    return SMT_OK;
}
SMT_API int smt_free(void *p) { SMT_HIP(hipFree(p)); return SMT_OK; }
SMT_API int smt_memcpy_h2d(void *d, const void *s, size_t n, void *st)
{
    SMT_HIP(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_memcpy_d2h(void *d, const void *s, size_t n, void *st)
{
    SMT_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_memset(void *d, int b, size_t n, void *st)
{
    SMT_HIP(hipMemsetAsync(d, b, n, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_stream_create(void **s)
{
    if (!s) return SMT_ERR_ARG;
    hipStream_t st;
    SMT_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *s = (void *)st;
    return SMT_OK;
}
SMT_API int smt_stream_destroy(void *s) { SMT_HIP(hipStreamDestroy(smt_stream(s))); return SMT_OK; }
SMT_API int smt_stream_sync(void *s) { SMT_HIP(hipStreamSynchronize(smt_stream(s))); return SMT_OK; }

template <int C>
static void launch_store_only(smt_adcensus *h, float *v0, float *v1, hipStream_t st)
{
    const int nbx = (h->W + FTJ - 1) / FTJ;
    const unsigned nblk = (unsigned)(((long)nbx * h->H * 2 + 7) / 8 * 8);
    hipLaunchKernelGGL((k_store_only2<C>), dim3(nblk), dim3(NT), 0, st, h->H, h->W, v0, v1, nbx);
}
static void store_only(smt_adcensus *h, float *v0, float *v1, hipStream_t st)
{
    switch (h->D / 64) {
    case 1: launch_store_only<1>(h, v0, v1, st); break;
    case 2: launch_store_only<2>(h, v0, v1, st); break;
    case 3: launch_store_only<3>(h, v0, v1, st); break;
    default: launch_store_only<4>(h, v0, v1, st); break;
    }
}

// Placement-aware allocation of the two cost volumes.  The cost kernel is a pure store stream (8 XCDs,
// each writing its own contiguous eighth of the two volumes), and what that stream reaches depends on
// WHICH physical pages hipMalloc handed out: on one MI355X, in one process, at a constant 2.37 GHz shader
// clock, the store-only twin of the kernel runs at either ~7.0 TB/s or ~5.9 TB/s on successive
// allocations of the same size, and the same virtual range re-allocated later lands in the other mode
// (tools/alloc_probe.hip).  Nothing in the kernel can change that afterwards, so
// Initialize takes up to PLACE_TRIES candidate pairs, times the store-only twin on each (a few launches,
// ~5 ms per candidate at 1080p x 192), keeps the fastest and frees the rest.  Rejected candidates stay
// allocated until the end so that every try gets different pages.  SMT_PLACEMENT=0 in the environment
// turns the search off (first allocation is used).
static int place_volumes(smt_adcensus *h, bool allow_search)
{
    const size_t V = (size_t)h->H * h->W * h->D;
    constexpr int PLACE_TRIES = 6;
    const char *env = getenv("SMT_PLACEMENT");
    const bool search = allow_search && !(env && env[0] == '0') && h->D % 64 == 0 && h->D <= 256 && V >= ((size_t)1 << 22);
    float *cand[PLACE_TRIES][2] = {};
    float ms[PLACE_TRIES];
    int n = 0, best = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (search && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) return SMT_ERR_HIP;
    // a candidate at this rate is in the fast mode (7.0 TB/s measured at 1080p x 192): stop looking
    const double good_ms = 2.0 * V * 4 / 6.75e12 * 1e3;
    for (; n < (search ? PLACE_TRIES : 1); n++) {
        if (smt_malloc((void **)&cand[n][0], V * 4) != SMT_OK) break;
        if (smt_malloc((void **)&cand[n][1], V * 4) != SMT_OK) { (void)hipFree(cand[n][0]); cand[n][0] = nullptr; break; }
        if (!search) { best = n; n++; break; }
        const int reps = 8;
        for (int k = 0; k < 3; k++) store_only(h, cand[n][0], cand[n][1], nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int k = 0; k < reps; k++) store_only(h, cand[n][0], cand[n][1], nullptr);
        (void)hipEventRecord(e1, nullptr);
        float t = 0;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) t = 1e30f;
        ms[n] = t / reps;
        if (best < 0 || ms[n] < ms[best]) best = n;
        if (ms[n] <= good_ms) { n++; break; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (int k = 0; k < n; k++)
        if (k != best) { (void)hipFree(cand[k][0]); (void)hipFree(cand[k][1]); }
    if (best < 0) return SMT_ERR_ALLOC;
    h->vol[0] = cand[best][0]; h->vol[1] = cand[best][1];
    h->place_tries = n;
    h->place_ms = search ? ms[best] : 0.0f;
    return SMT_OK;
}

// launch_fast<C, FULL> (below) by runtime C = 1..4 hypotheses per lane and full: D == 64 C; false for any other C
static bool launch_fast_as(int C, bool full, smt_adcensus *h, int views, float *dL, float *dR, const float *nL = nullptr,
                           const float *nR = nullptr, bool maps = false);

// Streaming (non-temporal) or ordinary stores for the volumes?  Streaming stores were worth 8-19 % on the
// devices of round 1; on another device the store-only twin is 5 % FASTER with ordinary stores (DESIGN.md
// section 4).  Like the placement this is a property of the device, so Initialize times the real both-views
// kernel a few launches each way on the handle's own (zeroed) tables and volumes and keeps ordinary stores
// only when they win by more than 2 %.  SMT_STORE_MODE=nt / plain in the environment fixes the choice.
static void calibrate_store_mode(smt_adcensus *h, bool allow)
{
    h->plain_stores = false; h->store_mode_ms[0] = h->store_mode_ms[1] = 0.0f;
    const char *env = getenv("SMT_STORE_MODE");
    if (env && env[0] == 'p') { h->plain_stores = true; return; }
    if (env && env[0] == 'n') return;
    if (!allow) return;
    const size_t V = (size_t)h->H * h->W * h->D;
    if (h->D % 64 != 0 || V < ((size_t)1 << 22)) return;
    const size_t N = (size_t)h->H * h->W;
    // zeroed tables are valid inputs (census 0, bytes 0); the speed of a store-bound kernel does not depend on them
    for (int t = 0; t < 2; t++) {
        for (int v = 0; v < 2; v++) {
            if (hipMemset(h->TS[t].cenA[v], 0, N * 8) != hipSuccess || hipMemset(h->TS[t].u8[v], 0, N) != hipSuccess ||
                hipMemset(h->TS[t].cenX[v], 0, (size_t)h->H * h->TS[t].WX * 8) != hipSuccess) return;
        }
        if (hipMemset(h->TS[t].mask, 0, N * 8) != hipSuccess) return;
    }
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
    const hipStream_t keep = h->stream;
    h->stream = nullptr;
    float best[2] = {1e30f, 1e30f};
    for (int round = 0; round < 2; round++)                    // interleaved: nt, plain, nt, plain
        for (int mode = 0; mode < 2; mode++) {
            h->plain_stores = mode == 1;
            const int reps = 4;
            auto launch = [&]() { (void)launch_fast_as(std::min(h->D / 64, 4), true, h, SMT_VIEW_BOTH, nullptr, nullptr); };
            launch();
            (void)hipEventRecord(e0, nullptr);
            for (int k = 0; k < reps; k++) launch();
            (void)hipEventRecord(e1, nullptr);
            float t = 1e30f;
            if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) t /= reps;
            if (t < best[mode]) best[mode] = t;
        }
    h->stream = keep;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    h->store_mode_ms[0] = best[0]; h->store_mode_ms[1] = best[1];
    h->plain_stores = best[1] < 0.98f * best[0];
    // Initialize's contract: the volumes read as zeros until the first Compute* (AD-Census.h:341-342)
    (void)hipMemset(h->vol[0], 0, V * 4); (void)hipMemset(h->vol[1], 0, V * 4);
    (void)hipMemset(h->TS[0].flag, 0, 4);
}

SMT_API int smt_adcensus_store_mode(smt_adcensus *h, int *plain, float *nt_ms, float *plain_ms)
{
    if (!h) return SMT_ERR_ARG;
    if (plain) *plain = h->plain_stores ? 1 : 0;
    if (nt_ms) *nt_ms = h->store_mode_ms[0];
    if (plain_ms) *plain_ms = h->store_mode_ms[1];
    return SMT_OK;
}

SMT_API int smt_adcensus_placement(smt_adcensus *h, int *tries, float *store_only_ms)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (tries) *tries = h->place_tries;
    if (store_only_ms) *store_only_ms = h->place_ms;
    return SMT_OK;
}

// fusion tables, the reference's own float expression (AD-Census.h:287-288)
static void build_lut(float sigmaC, float sigmaS, float *lut)
{
    for (int k = 0; k < 256; k++) lut[k] = 1.0f - expf(-((float)k / sigmaC));
    for (int k = 0; k < 64; k++) lut[256 + k] = 1.0f - expf(-((float)k / sigmaS));
}

// Rank table of the maps-only kernel: rank[64*ad + hd] = dense rank of the f32 sum lut[ad] + lut[256 + hd] (the one
// IEEE round-to-nearest add the kernels perform) among all 256 x 64 sums.  sigmaC, sigmaS > 0, so every sum is finite
// and >= +0 and the order of the bit patterns as uint32 is the order of the costs: equal bits get an equal rank,
// larger bits a larger one.  At most 16384 ranks, so rank << 16 | d is a WTA key for d < 65536.
static bool build_rank(const float *lut, uint16_t *rank)
{
    static_assert(RANK_N <= 65536, "");
    uint64_t *kv = new (std::nothrow) uint64_t[RANK_N];
    if (!kv) return false;
    for (int a = 0; a < 256; a++)
        for (int c = 0; c < 64; c++) {
            const float f = lut[a] + lut[256 + c];
            uint32_t bits;
            memcpy(&bits, &f, 4);
            kv[a * 64 + c] = ((uint64_t)bits << 32) | (uint32_t)(a * 64 + c);
        }
    std::sort(kv, kv + RANK_N);
    int r = -1;
    uint32_t prev = 0;
    for (int n = 0; n < RANK_N; n++) {
        const uint32_t bits = (uint32_t)(kv[n] >> 32);
        if (n == 0 || bits != prev) r++;
        prev = bits;
        rank[(uint32_t)kv[n]] = (uint16_t)r;
    }
    delete[] kv;
    return true;
}

// The stream chain c runs on in the call being issued: the caller's, or the internal one the chained schedule gave it.
static hipStream_t chain_stream(const smt_adcensus *h, int c)
{
    return h->chain_on[c] == 0 ? h->stream : h->chain_on[c] == 1 ? h->prep_stream : h->chain2_stream;
}
// The stream of the pair being issued.
static hipStream_t run_stream(const smt_adcensus *h) { return chain_stream(h, h->cur); }

// The pending conversion of chain c's shared form, if any, as a launch of its own on the chain's stream.  Every path
// that is not the chain's next shared launch calls this before it does anything else on that stream.
static void flush_conversion(smt_adcensus *h, int c)
{
    ChainState &ch = h->chain[c];
    if (!ch.conv_pending) return;
    const long N = (long)h->H * h->W;
    hipLaunchKernelGGL(k_shared_convert, dim3((unsigned)shared_conv_items(h->H, h->W)), dim3(NT), 0, chain_stream(h, c),
                       h->skeys[ch.conv_map], ch.conv_dR, N);
    ch.conv_pending = false;
}

// maps_resident of the handle: CUs / 8 x the workgroups per CU the runtime reports for the instantiation that D selects
// (launch_fast_as).  A query that fails leaves 0: the tapered tail's default rule stays off.
template <int C, bool FULL>
static void query_maps_resident(smt_adcensus *h, int cus)
{
    int n[3] = {0, 0, 0};
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[0], k_cost_maps_shared<C, FULL>, NT, 0) != hipSuccess) n[0] = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[1], k_cost_maps2p<C, FULL, MODE_MAPS_FLOAT>, NT, 0) != hipSuccess) n[1] = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[2], k_cost_maps2p<C, FULL, MODE_MAPS_RANK>, NT, 0) != hipSuccess) n[2] = 0;
    for (int t = 0; t < 3; t++) h->maps_resident[t] = n[t] > 0 ? cus / 8 * n[t] : 0;
}
static void set_maps_resident(smt_adcensus *h)
{
    h->maps_resident[0] = h->maps_resident[1] = h->maps_resident[2] = 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 8) return;
    switch ((h->D + 63) / 64 * 2 + (h->D % 64 == 0 ? 1 : 0)) {
    case 3: query_maps_resident<1, true>(h, cus); break;
    case 5: query_maps_resident<2, true>(h, cus); break;
    case 7: query_maps_resident<3, true>(h, cus); break;
    case 9: query_maps_resident<4, true>(h, cus); break;
    case 2: query_maps_resident<1, false>(h, cus); break;
    case 4: query_maps_resident<2, false>(h, cus); break;
    case 6: query_maps_resident<3, false>(h, cus); break;
    case 8: query_maps_resident<4, false>(h, cus); break;
    default: break;
    }
    (void)hipGetLastError();
}

static int adcensus_create(int H, int W, int D, float sigmaC, float sigmaS, unsigned flags, smt_adcensus **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || !(sigmaC > 0.0f) || !(sigmaS > 0.0f) ||
        (long long)H * W >= (1ll << 31))                 // pixel counts and key-map items are int
        return SMT_ERR_ARG;
    smt_adcensus *h = new (std::nothrow) smt_adcensus();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->sigmaC = sigmaC; h->sigmaS = sigmaS;
    h->stream = nullptr; h->timing = false; h->force_generic = false; h->ev = nullptr; h->n_timed = 0; h->n_seen = 0; h->timing_stride = 1; h->ev_merged = nullptr;
    const size_t N = (size_t)H * W, V = N * D;
    const int WX = W + 4;
    int rc = place_volumes(h, !(flags & SMT_ADCENSUS_NO_PLACEMENT_SEARCH));
    auto alloc = [&](void **p, size_t bytes) { if (rc == SMT_OK) rc = smt_malloc(p, bytes); };
    alloc((void **)&h->TS[0].lut, 320 * 4);
    alloc((void **)&h->TS[0].rank, RANK_N * 2);
    alloc((void **)&h->TS[0].flag, 4);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) {
        h->TS[t].WX = WX;
        h->TS[t].stamp = nullptr;
        h->TS[t].lut = h->TS[0].lut;                     // shared
        h->TS[t].rank = h->TS[0].rank;
        h->TS[t].flag = h->TS[0].flag;
        for (int v = 0; v < 2; v++) {
            alloc((void **)&h->TS[t].cenA[v], N * 8);
            alloc((void **)&h->TS[t].cenX[v], (size_t)H * WX * 8);
            alloc((void **)&h->TS[t].u8[v], N);
        }
        alloc((void **)&h->TS[t].mask, N * 8);
    }
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) alloc((void **)&h->skeys[t], N * 8);
    h->T = h->TS[0];
    if (rc != SMT_OK) { smt_adcensus_destroy(h); return rc; }
    if (hipStreamCreateWithFlags(&h->prep_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->chain2_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->in_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) != hipSuccess) {
        smt_adcensus_destroy(h);
        return SMT_ERR_HIP;
    }
    for (int c = 1; c < SMT_MAX_CHAINS; c++)
        if (hipEventCreateWithFlags(&h->join_ev[c], hipEventDisableTiming) != hipSuccess) {
            smt_adcensus_destroy(h);
            return SMT_ERR_HIP;
        }
    for (int t = 0; t < 2; t++)
        if (hipEventCreateWithFlags(&h->prep_done[t], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->cost_done[t], hipEventDisableTiming) != hipSuccess) {
            smt_adcensus_destroy(h);
            return SMT_ERR_HIP;
        }
    float lut[320];
    build_lut(sigmaC, sigmaS, lut);
    uint16_t *rank = new (std::nothrow) uint16_t[RANK_N];
    if (!rank || !build_rank(lut, rank)) { delete[] rank; smt_adcensus_destroy(h); return SMT_ERR_ALLOC; }
    const bool rank_ok = hipMemcpy(h->TS[0].rank, rank, RANK_N * 2, hipMemcpyHostToDevice) == hipSuccess;
    delete[] rank;
    // the reference's `new float[size*dispRange]()` value-initialises the volumes (AD-Census.h:341-342):
    // GetPtrLeft/Right before the first Compute* reads zeros
    if (!rank_ok || hipMemcpy(h->TS[0].lut, lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->vol[0], 0, V * 4) != hipSuccess || hipMemset(h->vol[1], 0, V * 4) != hipSuccess ||
        hipMemset(h->TS[0].flag, 0, 4) != hipSuccess) {
        smt_adcensus_destroy(h);
        return SMT_ERR_HIP;
    }
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++)
        if (hipMemset(h->skeys[t], 0xFF, N * 8) != hipSuccess) { smt_adcensus_destroy(h); return SMT_ERR_HIP; }
    calibrate_store_mode(h, !(flags & SMT_ADCENSUS_NO_STORE_CALIBRATION));
    set_maps_resident(h);
    *out = h;
    return SMT_OK;
}

SMT_API int smt_adcensus_create(int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out)
{
    return adcensus_create(H, W, D, sigmaC, sigmaS, 0u, out);
}

SMT_API int smt_adcensus_create_ex(int device, int H, int W, int D, float sigmaC, float sigmaS, unsigned flags, smt_adcensus **out)
{
    if (flags & ~(unsigned)(SMT_ADCENSUS_NO_PLACEMENT_SEARCH | SMT_ADCENSUS_NO_STORE_CALIBRATION)) return SMT_ERR_ARG;
    if (device < 0) return adcensus_create(H, W, D, sigmaC, sigmaS, flags, out);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return adcensus_create(H, W, D, sigmaC, sigmaS, flags, out);
}

SMT_API int smt_adcensus_create_on(int device, int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return smt_adcensus_create(H, W, D, sigmaC, sigmaS, out);
}

SMT_API int smt_adcensus_destroy(smt_adcensus *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    for (int c = 0; c < SMT_MAX_CHAINS; c++)                 // never pending here; chain_on is all 0: the handle's stream
        if (h->chain[c].conv_pending) { flush_conversion(h, c); (void)hipStreamSynchronize(h->stream); }
    if (h->prep_stream) { (void)hipStreamSynchronize(h->prep_stream); (void)hipStreamDestroy(h->prep_stream); }
    if (h->chain2_stream) { (void)hipStreamSynchronize(h->chain2_stream); (void)hipStreamDestroy(h->chain2_stream); }
    if (h->in_ready) (void)hipEventDestroy(h->in_ready);
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (int c = 1; c < SMT_MAX_CHAINS; c++)
        if (h->join_ev[c]) (void)hipEventDestroy(h->join_ev[c]);
    for (int t = 0; t < 2; t++) {
        if (h->prep_done[t]) (void)hipEventDestroy(h->prep_done[t]);
        if (h->cost_done[t]) (void)hipEventDestroy(h->cost_done[t]);
    }
    (void)hipFree(h->vol[0]); (void)hipFree(h->vol[1]);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) {
        for (int v = 0; v < 2; v++) {
            (void)hipFree(h->TS[t].cenA[v]); (void)hipFree(h->TS[t].cenX[v]); (void)hipFree(h->TS[t].u8[v]);
        }
        (void)hipFree(h->TS[t].mask);
    }
    (void)hipFree(h->TS[0].lut); (void)hipFree(h->TS[0].rank); (void)hipFree(h->TS[0].flag);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) (void)hipFree(h->skeys[t]);
    if (h->ev) {
        for (int k = 0; k < SMT_TIMING_SLOTS * 4; k++) (void)hipEventDestroy(h->ev[k]);
        delete[] h->ev_merged;
        delete[] h->ev;
    }
    delete h;
    return SMT_OK;
}

SMT_API int smt_adcensus_set_stream(smt_adcensus *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_adcensus_set_quirks(smt_adcensus *h, unsigned quirks)
{
    if (!h || (quirks & ~SMT_QUIRK_FIX_ALL)) return SMT_ERR_ARG;
    // every launch takes its Tables (this pair's and, for the table workgroups riding in a cost launch, the next
    // pair's) by value from these at issue time; no call leaves tables built for the next one
    const int col = (quirks & SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE) ? h->W - 1 : 0;
    h->T.edge_col = col;
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) h->TS[t].edge_col = col;
    return SMT_OK;
}

template <int C, bool FULL>
static void launch_cost(smt_adcensus *h, int view0, int nviews, float *d0, float *d1)
{
    const int D = h->D;
    dim3 grid((h->W + TJ - 1) / TJ, h->H, nviews);
    const int NX = TJ + D;
    size_t shm = (size_t)NX * 8 + TJ * 16 + 320 * 4 + NX + TJ;
    shm = (shm + 15) & ~(size_t)15;
    hipLaunchKernelGGL((k_cost<C, FULL>), grid, dim3(NT), shm, run_stream(h), h->H, h->W, D, h->T,
                       view0, h->vol[0], h->vol[1], d0, d1);
}

// Chunks per workgroup of the maps-only kernel (k_cost_maps2p).  SMT_MAPS_CHUNKS=<1..64> in the environment is a
// tuning hook (read at every call); SMT_MAPS_KERNEL=rank selects the rank-key form in place of the float LUT (A/B,
// at the 4 workgroups per CU its 32 KB table leaves room for, it is the slower one).
static int maps_chunks()
{
    const char *env = getenv("SMT_MAPS_CHUNKS");
    const int k = env ? atoi(env) : 0;
    return k >= 1 && k <= 64 ? k : 4;
}

// Tapered tail of a maps-only launch (maps_span): the counts n2, n1 per slice for a launch whose slices have `per`
// chunks, from S = the workgroups of the launching kernel that one slice's CUs hold at a time (maps_resident, queried
// at create; 0: unknown).  THE DEFAULT RULE: off when the slice has no more than S groups -- a launch of at most one
// round has no last round to taper -- and otherwise n2 = S * TAPER_N2_HALVES / 2, n1 = S * TAPER_N1_HALVES / 2, the
// sizing chosen by the sweep of DESIGN.md section 4 "Tapered tail": one resident set of 1-chunk workgroups and no
// half-sized ones, the only sizing of the sweep that won at all three workloads (more 1-chunk workgroups, or any
// half-sized ones, lose 4 % at 1080p x 192, where a 1-chunk workgroup flushes four ring columns per pixel).
//   SMT_MAPS_TAPER in the environment (read at every call): `0` is off -- the plain rule and the plain placement of the
//   auxiliary groups; `n2,n1` are these counts per slice whatever the launch size (tests, the sweep).
// Returns the counts shrunk to the slice (maps_span_tails), so the kernels' span arithmetic takes no division for them.
constexpr int TAPER_N2_HALVES = 0, TAPER_N1_HALVES = 2;
static void maps_taper(int S, long per, int K, int &n2, int &n1)
{
    n2 = n1 = 0;
    const char *env = getenv("SMT_MAPS_TAPER");
    if (env && env[0]) {
        int a = 0, b = 0;
        if (sscanf(env, "%d,%d", &a, &b) == 2 && a >= 0 && b >= 0) { n2 = a; n1 = b; }
    } else if (S > 0 && maps_span_groups(per, K, 0, 0) > S) {
        n2 = (int)((long)S * TAPER_N2_HALVES / 2);
        n1 = (int)((long)S * TAPER_N1_HALVES / 2);
    }
    (void)maps_span_tails(per, K, n2, n1);
}

// SMT_MAPS_SHARED=0 in the environment (read at every call) keeps the two-view k_cost_maps2p where the shared form
// (k_cost_maps_shared) would run: same-process A/Bs and tests.
static bool maps_shared()
{
    const char *env = getenv("SMT_MAPS_SHARED");
    return !(env && env[0] == '0' && env[1] == 0);
}
// The shapes the shared form serves: an identity set that is not empty, and D <= 192.  With four hypotheses per lane
// (192 < D <= 256) the lanes' publishes are 32 bytes apart, a 4-way bank conflict, the kernel needs 93 VGPRs and the
// identity set is a smaller part of the row; measured at 1242 x 375 D = 256 it loses 7 % to the two-view kernel
// (DESIGN.md section 4).  SMT_MAPS_SHARED=force in the environment takes it wherever the set is not empty (tests).
static bool maps_shared_shape(int W, int D)
{
    if (shared_id_hi(W, D) < 3) return false;
    const char *env = getenv("SMT_MAPS_SHARED");
    return D <= 192 || (env && env[0] == 'f');
}

// SMT_SHARED_FINISH=apart in the environment (read at every call) converts every shared pair's keys with a launch of
// its own right behind the pair's launch, instead of inside the next pair's: same-process A/Bs and tests.
static bool shared_finish_apart()
{
    const char *env = getenv("SMT_SHARED_FINISH");
    return env && strcmp(env, "apart") == 0;
}

// The pair takes the shared form (k_cost_maps_shared); every other pair flushes a pending conversion first.
static bool pair_takes_shared(const smt_adcensus *h, int views, const float *dL, const float *dR, bool maps)
{
    if (!(views == SMT_VIEW_BOTH && maps) || h->force_generic || (h->D + 63) / 64 > 4) return false;
    const char *env = getenv("SMT_MAPS_KERNEL");
    return !(env && env[0] == 'r') && dL && dR && maps_shared_shape(h->W, h->D) && maps_shared();
}

// Table workgroups of one pair: the tiles and the workgroups of the 13 border columns (16 rows each).
static int prep_items(int H, int W, int &ptx)
{
    ptx = (W + PTW - 1) / PTW;
    const int pty = (H + PTH - 1) / PTH, eb = (H + PNT / 16 - 1) / (PNT / 16);
    return ptx * (pty + (eb + ptx - 1) / ptx);
}

template <int C, bool FULL>
static void launch_fast(smt_adcensus *h, int views, float *dL, float *dR, const float *nL, const float *nR, bool maps)
{
    const int nbx = (h->W + FTJ - 1) / FTJ;
    auto blocks = [&](int nviews) { return dim3((unsigned)(((long)nbx * h->H * nviews + 7) / 8 * 8)); };
    ChainState &ch = h->chain[h->cur];
    const hipStream_t st = run_stream(h);
    if (views == SMT_VIEW_BOTH && maps) {
        // pair of a batch whose volumes nobody can read: maps only, the next pair's table workgroups (if any) fused in
        const int K = maps_chunks();
        int nprep = 0, ptx = 1;
        if (nL) nprep = prep_items(h->H, h->W, ptx);
        const Tables &Tn = h->TS[chain_slot(h->cur, ch.n_pairs + 1)];
        const char *env = getenv("SMT_MAPS_KERNEL");
        int n2, n1;
        if (pair_takes_shared(h, views, dL, dR, maps)) {
            // One launch on the chain's stream: the left-view runs, this pair's edge items, the table tiles of the
            // chain's next pair and the conversion of its previous shared pair.  This pair's own conversion stays pending.
            const int km = chain_slot(h->cur, ch.n_pairs);
            if (ch.conv_pending && ch.conv_map == km) flush_conversion(h, h->cur);   // cannot happen: shared pairs in a row alternate
            const bool carried = ch.conv_pending;
            maps_taper(h->beside ? 0 : h->maps_resident[0], ((long)nbx * h->H + 7) >> 3, K, n2, n1);
            const int ncs = maps_groups(nbx, h->H, 1, K, n2, n1), Dd = FULL ? 64 * C : h->D;
            const int cbody = maps_body_groups(nbx, h->H, 1, K, n2, n1);
            const int nconv = carried ? shared_conv_items(h->H, h->W) : 0, nedge = shared_edge_items(h->H, h->W, Dd);
            const unsigned gs = 8u * (unsigned)fused_grid(ncs, nprep + nconv + nedge, cbody).groups;
            hipLaunchKernelGGL((k_cost_maps_shared<C, FULL>), dim3(gs), dim3(NT), 0, st, h->H, h->W, h->D, h->T, dL, dR,
                               h->skeys[km], nbx, K, shared_pub_hi(h->W), ncs, nprep, nL, nR, Tn, ptx, nconv, nedge,
                               carried ? h->skeys[ch.conv_map] : nullptr, carried ? ch.conv_dR : nullptr, n2, n1, cbody);
            if (SMT_SHARED_KNOCKOUT != 2) { ch.conv_pending = true; ch.conv_map = km; ch.conv_dR = dR; }
            else ch.conv_pending = false;
            if (shared_finish_apart()) flush_conversion(h, h->cur);
            return;
        }
        const bool rank = env && env[0] == 'r';
        maps_taper(h->beside ? 0 : h->maps_resident[rank ? 2 : 1], ((long)nbx * h->H * 2 + 7) >> 3, K, n2, n1);
        const int ncost = maps_groups(nbx, h->H, 2, K, n2, n1), cbody = maps_body_groups(nbx, h->H, 2, K, n2, n1);
        const unsigned grid = nL ? 8u * (unsigned)fused_grid(ncost, nprep, cbody).groups : (unsigned)ncost;
        if (rank)
            hipLaunchKernelGGL((k_cost_maps2p<C, FULL, MODE_MAPS_RANK>), dim3(grid), dim3(NT), 0, st, h->H, h->W,
                               h->D, h->T, dL, dR, nbx, K, ncost, nprep, nL, nR, Tn, ptx, n2, n1, cbody);
        else
            hipLaunchKernelGGL((k_cost_maps2p<C, FULL, MODE_MAPS_FLOAT>), dim3(grid), dim3(NT), 0, st, h->H, h->W,
                               h->D, h->T, dL, dR, nbx, K, ncost, nprep, nL, nR, Tn, ptx, n2, n1, cbody);
        return;
    }
    if (views == SMT_VIEW_BOTH && nL) {
        // this pair's cost workgroups + the next pair's table workgroups (into the other table set) in one launch
        const int ncost = (int)blocks(2).x;
        const int ptx = (h->W + PTW - 1) / PTW, pty = (h->H + PTH - 1) / PTH;
        const int eb = (h->H + PNT / 16 - 1) / (PNT / 16);
        const int nprep = ptx * (pty + (eb + ptx - 1) / ptx);
        const unsigned grid = 8u * (unsigned)fused_grid(ncost, nprep).groups;
        const Tables &Tn = h->TS[chain_slot(h->cur, ch.n_pairs + 1)];
        if (h->plain_stores)
            hipLaunchKernelGGL((k_cost_fast2p<C, FULL, false>), dim3(grid), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                               h->vol[0], h->vol[1], dL, dR, nbx, ncost, nprep, nL, nR, Tn, ptx);
        else
            hipLaunchKernelGGL((k_cost_fast2p<C, FULL, true>), dim3(grid), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                               h->vol[0], h->vol[1], dL, dR, nbx, ncost, nprep, nL, nR, Tn, ptx);
        return;
    }
    if (views == SMT_VIEW_BOTH) {
        if (h->plain_stores)
            hipLaunchKernelGGL((k_cost_fast2<C, FULL, false>), blocks(2), dim3(NT), 0, st, h->H, h->W, h->D, h->T, h->vol[0],
                               h->vol[1], dL, dR, nbx);
        else
            hipLaunchKernelGGL((k_cost_fast2<C, FULL, true>), blocks(2), dim3(NT), 0, st, h->H, h->W, h->D, h->T, h->vol[0],
                               h->vol[1], dL, dR, nbx);
        return;
    }
    if (views & SMT_VIEW_LEFT)
        hipLaunchKernelGGL((k_cost_fast<C, 0, FULL>), blocks(1), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                           h->vol[0], dL, nbx);
    if (views & SMT_VIEW_RIGHT)
        hipLaunchKernelGGL((k_cost_fast<C, 1, FULL>), blocks(1), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                           h->vol[1], dR, nbx);
}

static bool launch_fast_as(int C, bool full, smt_adcensus *h, int views, float *dL, float *dR, const float *nL,
                           const float *nR, bool maps)
{
    switch (C * 2 + (full ? 1 : 0)) {
    case 3: launch_fast<1, true>(h, views, dL, dR, nL, nR, maps); break;
    case 5: launch_fast<2, true>(h, views, dL, dR, nL, nR, maps); break;
    case 7: launch_fast<3, true>(h, views, dL, dR, nL, nR, maps); break;
    case 9: launch_fast<4, true>(h, views, dL, dR, nL, nR, maps); break;
    case 2: launch_fast<1, false>(h, views, dL, dR, nL, nR, maps); break;
    case 4: launch_fast<2, false>(h, views, dL, dR, nL, nR, maps); break;
    case 6: launch_fast<3, false>(h, views, dL, dR, nL, nR, maps); break;
    case 8: launch_fast<4, false>(h, views, dL, dR, nL, nR, maps); break;
    default: return false;
    }
    return true;
}

// One pair into its chain's table set chain_slot(cur, n).  Three schedules for the pairs of a batch on chain 0, and the
// chained one (chain_plan below), which issues every pair as a `prepped` pair of the fused schedule on its chain:
//   fused (default, both views through the register-window kernel): the table workgroups of pair n + 1 ride in the
//     grid of pair n's cost kernel (k_cost_fast2p) -- one stream, one launch per pair, no events; `prepped` says this
//     pair's tables were built that way, `nL / nR` are the next pair's images (null for the last pair of a batch);
//   overlap (SMT_OVERLAP=1, and the schedule of single views / D > 256): the table kernels run on the handle's internal
//     stream beside the previous pair's cost kernel on the caller's stream; event edges:
//       cost_done[n-2] --> prep stream               (table set n&1 is free again)
//       prep_done[n]   --> caller stream --> cost kernel(s) --> cost_done[n]
//     only for pairs b >= 1 of a batch (their inputs were already ordered behind the caller's stream by pair 0);
//   in order on the caller's stream (single pairs, the first pair of a batch, SMT_OVERLAP=0).
// Measured on MI355X the overlap gives +18 % at 1242x375 D=256 and +2-3.5 % at 1920x1080 D=192 over the in-order form
// (the table kernels then take 0.09 instead of 0.04 ms, hidden behind a cost kernel that gets 1 % slower); the fused
// form against the overlap: DESIGN.md section 4.
static bool fast_both_views(const smt_adcensus *h, int views)
{
    return views == SMT_VIEW_BOTH && !h->force_generic && (h->D + 63) / 64 <= 4;
}

// The stand-alone table kernel of one pair: tile workgroups + the workgroups of the 13 border columns (16 rows each)
// in one launch.
static void launch_prep(const smt_adcensus *h, hipStream_t st, const float *L, const float *R, const Tables &T)
{
    const int tx = (h->W + PTW - 1) / PTW, ty = (h->H + PTH - 1) / PTH;
    const int eb = (h->H + PNT / 16 - 1) / (PNT / 16);
    hipLaunchKernelGGL(k_prep, dim3(tx, ty + (eb + tx - 1) / tx), dim3(PNT), 0, st, L, R, h->H, h->W, T);
}

// maps: the pair's volumes are not written (a batch pair before the last; fast_both_views only).
static int adcensus_pair(smt_adcensus *h, const float *L, const float *R, int views, float *dL,
                         float *dR, bool overlap, bool prepped = false, const float *nL = nullptr,
                         const float *nR = nullptr, bool maps = false)
{
    const int D = h->D;
    ChainState &ch = h->chain[h->cur];
    const int set = chain_slot(h->cur, ch.n_pairs);
    const hipStream_t st = run_stream(h);                    // the caller's stream unless a chain runs on an internal one
    h->T = h->TS[set];
    h->vol_pending = false;                                  // never observable: dropped with the tables they would come from
    if (!pair_takes_shared(h, views, dL, dR, maps)) flush_conversion(h, h->cur);
    const bool timed = h->timing && (h->n_seen++ % h->timing_stride) == 0;
    const long slot = h->n_timed % SMT_TIMING_SLOTS;
    hipEvent_t *ev = timed ? h->ev + 4 * slot : nullptr;
    // overlap == false: everything in order on the caller's stream (single pairs, first pair of a batch)
    hipStream_t ps = overlap ? h->prep_stream : st;          // overlap: chain 0 only, set is 0 or 1
    if (overlap && ch.n_pairs >= 2) SMT_HIP(hipStreamWaitEvent(ps, h->cost_done[set], 0));
    if (timed) (void)hipEventRecord(ev[0], ps);
    if (!prepped) launch_prep(h, ps, L, R, h->T);
    if (timed) (void)hipEventRecord(ev[1], ps);
    if (overlap) {
        SMT_HIP(hipEventRecord(h->prep_done[set], ps));
        SMT_HIP(hipStreamWaitEvent(st, h->prep_done[set], 0));
    }
    // one stream: the event after the table kernels is also the cost kernel's start
    if (timed) { h->ev_merged[slot] = !overlap; if (overlap) (void)hipEventRecord(ev[2], st); }
    const int view0 = (views & SMT_VIEW_LEFT) ? 0 : 1;
    const int nviews = (views == SMT_VIEW_BOTH) ? 2 : 1;
    const int C = (D + 63) / 64;
    const bool full = (D % 64) == 0;
    if (h->force_generic || C > 4) {
        // the table-lookup kernel of the first version: kept as an independent formulation, and the kernel for
        // 256 < D <= 512 (a lane then owns 5..8 consecutive hypotheses; the register-window kernel stops at 4)
        switch (C) {
        case 1: launch_cost<1, false>(h, view0, nviews, dL, dR); break;
        case 2: launch_cost<2, false>(h, view0, nviews, dL, dR); break;
        case 3: launch_cost<3, false>(h, view0, nviews, dL, dR); break;
        case 4: launch_cost<4, false>(h, view0, nviews, dL, dR); break;
        case 5: launch_cost<5, false>(h, view0, nviews, dL, dR); break;
        case 6: launch_cost<6, false>(h, view0, nviews, dL, dR); break;
        case 7: launch_cost<7, false>(h, view0, nviews, dL, dR); break;
        default: launch_cost<8, false>(h, view0, nviews, dL, dR); break;
        }
    } else if (!launch_fast_as(C, full, h, views, dL, dR, nL, nR, maps)) return SMT_ERR_ARG;
    if (timed) { (void)hipEventRecord(ev[3], st); h->n_timed++; }
    // the two-stream schedule waits on this before it reuses the table set; the fused one is ordered by its stream and
    // a chain > 0 by the call's join
    if (!prepped && !nL && h->cur == 0) SMT_HIP(hipEventRecord(h->cost_done[set], st));
    ch.n_pairs++;
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_adcensus_compute(smt_adcensus *h, const float *L, const float *R, int views,
                                 float *dispL, float *dispR)
{
    if (!h || !L || !R || views < 1 || views > 3) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    return adcensus_pair(h, L, R, views, dispL, dispR, false);
}

// schedule of the pairs b >= 1 of a batch: 0 in order, 1 two streams, 2 fused launches (adcensus_pair), 3 fused
// launches in chains (chain_plan); smt_adcensus_compute_batch keeps 2 where 3 does not apply
static int batch_schedule(const smt_adcensus *h, int views)
{
    const char *env = getenv("SMT_OVERLAP");             // tuning hook: 0 / 1 / 2 / 3 forces the choice
    int want = SMT_CHAINED_DEFAULT ? 3 : 2;
    if (env && env[0] >= '0' && env[0] <= '3' && env[1] == 0) want = env[0] - '0';
    if (want >= 2 && !fast_both_views(h, views)) want = 1;
    return want;
}

// ---- The chained schedule (3): pair b of a call belongs to chain b % NC; inside a chain everything is the fused
// schedule with a stride of NC, on the chain's own two table sets and two key maps; chain 0 runs on the caller's
// stream, chain c > 0 on internal stream c, forked from and joined into the caller's stream by events.  chain_plan
// writes the call down as a list of operations in issue order; adcensus_batch_chained issues that list and
// smt_adcensus_selftest_chains proves its order.  DESIGN.md section 4 "Chained launches".
enum { CH_PREP, CH_PAIR, CH_CONVERT, CH_RECORD, CH_WAIT };
constexpr int SMT_CHAIN_TAPER_DEFAULT = 0;               // CHAIN_TAPER_NONE
enum { CHAIN_ORDER_BESIDE = 0, CHAIN_ORDER_PAIRS, CHAIN_ORDER_AB, CHAIN_ORDER_BA };
enum { CHAIN_SHARED = 1, CHAIN_LAST_VOLUMES = 2, CHAIN_FORK_START = 4, CHAIN_FINISH_APART = 8, CHAIN_FLAGS = 15 };
struct ChainOp {
    int kind;
    int stream;            // 0: the caller's stream, c: the internal stream of chain c
    int chain;
    int pair;              // CH_PREP: the pair whose tables it builds; CH_PAIR: the pair; CH_CONVERT: -1
    int ts_read;           // CH_PAIR: TS[] index the launch reads; else -1
    int ts_built;          // CH_PREP, CH_PAIR: TS[] index the launch builds, for pair `built_for`; -1: none
    int built_for;
    int key_merged;        // CH_PAIR in the shared form: skeys[] index the launch merges into; else -1
    int key_conv;          // CH_PAIR, CH_CONVERT: skeys[] index converted, into the right map of pair `conv_pair`; -1: none
    int conv_pair;
    int ev;                // CH_RECORD, CH_WAIT: 0 the fork event, c the join event of chain c
};

// n pairs on nc chains whose pair counters stand at count0[] (only their parity matters).  flags: CHAIN_SHARED the
// maps-only pairs take the shared form; CHAIN_LAST_VOLUMES the last pair writes its volumes (never shared, converts
// nothing of its own); CHAIN_FORK_START fork from the call's first event instead of behind chain 0's k_prep;
// CHAIN_FINISH_APART every shared pair is converted right behind its launch (SMT_SHARED_FINISH=apart).  order: the
// SMT_CHAIN_ORDER forms; each keeps the state indexing and changes only streams and edges.
static int chain_plan(int n, int nc, const long *count0, int order, unsigned flags, std::vector<ChainOp> &ops)
{
    ops.clear();
    if (n < 1 || nc < 1 || nc > SMT_MAX_CHAINS || !count0 || order < CHAIN_ORDER_BESIDE || order > CHAIN_ORDER_BA ||
        (flags & ~(unsigned)CHAIN_FLAGS))
        return SMT_ERR_ARG;
    long cnt[SMT_MAX_CHAINS];
    int pend_key[SMT_MAX_CHAINS], pend_pair[SMT_MAX_CHAINS];
    for (int c = 0; c < SMT_MAX_CHAINS; c++) {
        if (count0[c] < 0) return SMT_ERR_ARG;
        cnt[c] = count0[c]; pend_key[c] = pend_pair[c] = -1;
    }
    if (nc > n) nc = n;                                      // a chain without pairs issues nothing
    auto on = [&](int c) { return order == CHAIN_ORDER_PAIRS ? 0 : c; };
    auto blank = [&](int kind, int c) { return ChainOp{kind, on(c), c, -1, -1, -1, -1, -1, -1, -1, -1}; };
    auto event = [&](int kind, int stream, int ev) {
        if (order == CHAIN_ORDER_PAIRS || nc < 2) return;    // one stream: no edges
        ChainOp o = blank(kind, stream); o.stream = stream; o.ev = ev; ops.push_back(o);
    };
    auto prep = [&](int c) {
        ChainOp o = blank(CH_PREP, c); o.pair = o.built_for = c; o.ts_built = chain_slot(c, cnt[c]); ops.push_back(o);
    };
    auto convert = [&](int c) {
        if (pend_key[c] < 0) return;
        ChainOp o = blank(CH_CONVERT, c); o.key_conv = pend_key[c]; o.conv_pair = pend_pair[c]; ops.push_back(o);
        pend_key[c] = pend_pair[c] = -1;
    };
    auto pair = [&](int b) {
        const int c = b % nc;
        const bool shared = (flags & CHAIN_SHARED) && !(b + 1 == n && (flags & CHAIN_LAST_VOLUMES));
        if (!shared) convert(c);
        ChainOp o = blank(CH_PAIR, c);
        o.pair = b; o.ts_read = chain_slot(c, cnt[c]);
        if (b + nc < n) { o.ts_built = chain_slot(c, cnt[c] + 1); o.built_for = b + nc; }
        if (shared) {
            o.key_merged = chain_slot(c, cnt[c]); o.key_conv = pend_key[c]; o.conv_pair = pend_pair[c];
            pend_key[c] = o.key_merged; pend_pair[c] = b;
        }
        ops.push_back(o);
        cnt[c]++;
        if (flags & CHAIN_FINISH_APART) convert(c);
    };
    auto whole_chain = [&](int c) { prep(c); for (int b = c; b < n; b += nc) pair(b); convert(c); };
    switch (order) {
    case CHAIN_ORDER_BESIDE: case CHAIN_ORDER_PAIRS:
        if (flags & CHAIN_FORK_START) event(CH_RECORD, 0, 0);
        prep(0);
        if (!(flags & CHAIN_FORK_START)) event(CH_RECORD, 0, 0);
        for (int c = 1; c < nc; c++) { event(CH_WAIT, c, 0); prep(c); }
        for (int b = 0; b < n; b++) pair(b);
        for (int c = 0; c < nc; c++) convert(c);
        for (int c = 1; c < nc; c++) event(CH_RECORD, c, c);
        for (int c = 1; c < nc; c++) event(CH_WAIT, 0, c);
        break;
    case CHAIN_ORDER_AB:                                     // chain c + 1 behind the whole of chain c
        whole_chain(0);
        event(CH_RECORD, 0, 0);
        for (int c = 1; c < nc; c++) { event(CH_WAIT, c, c - 1); whole_chain(c); event(CH_RECORD, c, c); }
        for (int c = 1; c < nc; c++) event(CH_WAIT, 0, c);
        break;
    default:                                                 // CHAIN_ORDER_BA: chain 0 behind the whole of the others
        event(CH_RECORD, 0, 0);
        for (int c = 1; c < nc; c++) { event(CH_WAIT, c, 0); whole_chain(c); event(CH_RECORD, c, c); }
        for (int c = 1; c < nc; c++) event(CH_WAIT, 0, c);
        whole_chain(0);
        break;
    }
    return SMT_OK;
}

// Chains of a chained call: SMT_CHAINS=<1..3> in the environment (read at every call), 2 otherwise.
static int chain_count()
{
    const char *env = getenv("SMT_CHAINS");
    return env && env[0] >= '1' && env[0] <= '0' + SMT_MAX_CHAINS && env[1] == 0 ? env[0] - '0' : SMT_CHAINS_DEFAULT;
}
// SMT_CHAIN_ORDER=pairs|ab|ba in the environment (read at every call): test hook, the orders of chain_plan.
static int chain_order()
{
    const char *env = getenv("SMT_CHAIN_ORDER");
    if (!env) return CHAIN_ORDER_BESIDE;
    return strcmp(env, "pairs") == 0 ? CHAIN_ORDER_PAIRS : strcmp(env, "ab") == 0 ? CHAIN_ORDER_AB :
           strcmp(env, "ba") == 0 ? CHAIN_ORDER_BA : CHAIN_ORDER_BESIDE;
}

// Which launches of a chained call keep the tapered tail's default rule: SMT_CHAIN_TAPER=all|last|none in the
// environment (read at every call; measurement).  The taper recovers the drain of a launch that runs alone; beside
// another chain's launch there is no such drain and its 1-chunk workgroups only cost.
enum { CHAIN_TAPER_NONE, CHAIN_TAPER_LAST, CHAIN_TAPER_ALL };
static int chain_taper()
{
    const char *env = getenv("SMT_CHAIN_TAPER");
    if (!env) return SMT_CHAIN_TAPER_DEFAULT;
    return strcmp(env, "all") == 0 ? CHAIN_TAPER_ALL : strcmp(env, "last") == 0 ? CHAIN_TAPER_LAST :
           strcmp(env, "none") == 0 ? CHAIN_TAPER_NONE : SMT_CHAIN_TAPER_DEFAULT;
}

// Schedule 3 of adcensus_batch_pairs: issues chain_plan's list.  Events only, no host synchronisation.  Whatever
// happens, every chain's pending conversion is issued and every internal stream that was given work is joined into the
// caller's stream before this returns, ahead of anything else the caller's stream gets.
static int adcensus_batch_chained(smt_adcensus *h, const float *L, const float *R, int n, int views, float *dispL,
                                  float *dispR, bool last_volumes)
{
    const size_t N = (size_t)h->H * h->W;
    const char *fenv = getenv("SMT_CHAIN_FORK");
    unsigned flags = 0;
    if (pair_takes_shared(h, views, dispL, dispR, true)) flags |= CHAIN_SHARED;
    if (last_volumes) flags |= CHAIN_LAST_VOLUMES;
    if (fenv && strcmp(fenv, "start") == 0) flags |= CHAIN_FORK_START;
    if (shared_finish_apart()) flags |= CHAIN_FINISH_APART;
    long count0[SMT_MAX_CHAINS];
    for (int c = 0; c < SMT_MAX_CHAINS; c++) count0[c] = h->chain[c].n_pairs;
    std::vector<ChainOp> ops;
    const int nc = chain_count(), order = chain_order(), taper = chain_taper();
    int rc = chain_plan(n, nc, count0, order, flags, ops);
    if (rc != SMT_OK) return rc;
    const bool concurrent = order == CHAIN_ORDER_BESIDE && std::min(nc, n) >= 2;
    auto internal = [&](int s) { return s == 1 ? h->prep_stream : h->chain2_stream; };
    auto stream = [&](int s) { return s == 0 ? h->stream : internal(s); };
    bool open[SMT_MAX_CHAINS] = {false, false, false};       // internal stream s has work that no join event covers yet
    int last_set = 0;
    auto issue = [&](const ChainOp &o) -> int {
        if (o.stream > 0 && o.kind != CH_RECORD) open[o.stream] = true;
        h->cur = o.chain;
        h->chain_on[o.chain] = o.kind == CH_RECORD || o.kind == CH_WAIT ? h->chain_on[o.chain] : o.stream;
        switch (o.kind) {
        case CH_PREP:
            launch_prep(h, stream(o.stream), L + o.pair * N, R + o.pair * N, h->TS[o.ts_built]);
            return SMT_OK;
        case CH_PAIR: {
            const int b = o.pair;
            if (chain_slot(o.chain, h->chain[o.chain].n_pairs) != o.ts_read) return SMT_ERR_STATE;   // plan and state disagree
            if (b + 1 == n) last_set = o.ts_read;
            h->beside = concurrent && (taper == CHAIN_TAPER_NONE || (taper == CHAIN_TAPER_LAST && b + 1 < n));
            return adcensus_pair(h, L + b * N, R + b * N, views, dispL ? dispL + b * N : nullptr,
                                 dispR ? dispR + b * N : nullptr, false, true,
                                 o.ts_built >= 0 ? L + o.built_for * N : nullptr,
                                 o.ts_built >= 0 ? R + o.built_for * N : nullptr, !(b + 1 == n && last_volumes));
        }
        case CH_CONVERT:
            flush_conversion(h, o.chain);
            return SMT_OK;
        case CH_RECORD:
            SMT_HIP(hipEventRecord(o.ev ? h->join_ev[o.ev] : h->fork_ev, stream(o.stream)));
            if (o.stream > 0) open[o.stream] = false;
            return SMT_OK;
        default:
            SMT_HIP(hipStreamWaitEvent(stream(o.stream), o.ev ? h->join_ev[o.ev] : h->fork_ev, 0));
            return SMT_OK;
        }
    };
    for (size_t k = 0; k < ops.size() && rc == SMT_OK; k++) rc = issue(ops[k]);
    if (rc != SMT_OK) {
        // an error path: what the plan had not issued yet of conversions and joins.  Waiting on a join event a second
        // time is harmless; an event recorded again is waited on again.
        for (int c = 0; c < SMT_MAX_CHAINS; c++) flush_conversion(h, c);
        for (int s = 1; s < SMT_MAX_CHAINS; s++) {
            bool used = open[s];
            for (int c = 0; c < SMT_MAX_CHAINS; c++) used = used || h->chain_on[c] == s;
            if (!used) continue;
            (void)hipEventRecord(h->join_ev[s], internal(s));
            (void)hipStreamWaitEvent(h->stream, h->join_ev[s], 0);
        }
    } else {
        h->T = h->TS[last_set];                              // the deferred volumes come from the last pair's tables
    }
    h->cur = 0;
    h->beside = false;
    for (int c = 0; c < SMT_MAX_CHAINS; c++) h->chain_on[c] = 0;
    if (rc != SMT_OK) return rc;
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// The per-pair loop of a batch (adcensus_internal.h).  Pair b >= 1 follows `sched`; pair 0 is in order, with its tables
// already built when `prepped`; with sched 2 the last pair builds the tables of (nL, nR) inside its launch when they are
// given.  With `maps_ok` and fast_both_views the pairs take the maps-only kernel, all but the last when `last_volumes`
// is set (the last one then leaves its volumes in the handle), every pair when it is clear.
int adcensus_batch_pairs(smt_adcensus *h, const float *L, const float *R, int n, int views, float *dispL,
                         float *dispR, int sched, bool prepped, const float *nL, const float *nR, bool maps_ok,
                         bool last_volumes)
{
    const size_t N = (size_t)h->H * h->W;
    maps_ok = maps_ok && fast_both_views(h, views);
    if (sched == 3) {
        if (maps_ok && n >= 2 && !prepped && !nL && !nR)
            return adcensus_batch_chained(h, L, R, n, views, dispL, dispR, last_volumes);
        sched = 2;                                           // every pair stores the handle's two volumes, or a host-fed chunk
    }
    for (int b = 0; b < n; b++) {
        const bool last = b + 1 == n;
        const float *bl = sched == 2 ? (last ? nL : L + (b + 1) * N) : nullptr;
        const float *br = sched == 2 ? (last ? nR : R + (b + 1) * N) : nullptr;
        int rc = adcensus_pair(h, L + b * N, R + b * N, views, dispL ? dispL + b * N : nullptr,
                               dispR ? dispR + b * N : nullptr, sched == 1 && b > 0, b > 0 ? sched == 2 : prepped,
                               bl, br, maps_ok && (!last || !last_volumes));
        if (rc != SMT_OK) { flush_conversion(h, 0); return rc; }
    }
    // the last shared pair has no next launch; the caller may read or free its maps behind this call
    flush_conversion(h, 0);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

bool adcensus_fused_both_views(const smt_adcensus *h) { return fast_both_views(h, SMT_VIEW_BOTH); }

// The volumes of a batch's deferred last pair, written now: the both-views cost kernel with null maps on the pair's
// tables (h->T, see vol_pending), on the handle's stream behind the batch's launches -- where an eager last pair would
// have stored them -- and waits for it.  The cost kernels do not touch the domain flag (k_prep raises it), so smt_adcensus_status reports
// what it would have.  With timing on, the launch is recorded like a pair whose tables were already built.
static int materialise_volumes(smt_adcensus *h)
{
    flush_conversion(h, 0);                                  // never pending here: no entry point leaves one
    if (!h->vol_pending) return SMT_OK;
    const long slot = h->n_timed % SMT_TIMING_SLOTS;
    hipEvent_t *ev = h->timing ? h->ev + 4 * slot : nullptr;
    if (ev) { (void)hipEventRecord(ev[0], h->stream); (void)hipEventRecord(ev[1], h->stream); h->ev_merged[slot] = true; }
    if (!launch_fast_as((h->D + 63) / 64, h->D % 64 == 0, h, SMT_VIEW_BOTH, nullptr, nullptr))
        return SMT_ERR_STATE;                                // only fast_both_views pairs are deferred
    if (ev) { (void)hipEventRecord(ev[3], h->stream); h->n_timed++; }
    h->vol_pending = false;
    SMT_LAUNCH_CHECK();
    // A caller that synchronised the stream after its batch could read an eager last pair's volumes from anywhere;
    // keep that true.  This happens at most once per handle: after the first lend nothing is deferred.
    SMT_HIP(hipStreamSynchronize(h->stream));
    return SMT_OK;
}

SMT_API int smt_adcensus_compute_batch(smt_adcensus *h, const float *L, const float *R, int pairs,
                                       int views, float *dispL, float *dispR)
{
    if (!h || !L || !R || pairs <= 0 || views < 1 || views > 3) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int sched = pairs > 1 ? batch_schedule(h, views) : 0;
    if (sched == 1) {
        // order the internal stream behind whatever produced the [pairs][H][W] inputs
        SMT_HIP(hipEventRecord(h->in_ready, h->stream));
        SMT_HIP(hipStreamWaitEvent(h->prep_stream, h->in_ready, 0));
    }
    // Only the last pair's volumes stay readable (every pair writes the same two), so pairs 0 .. pairs-2 of the
    // both-views register-window path take the maps-only kernel.  The last pair takes it too while no volume pointer
    // of this handle has been lent (nobody can read them yet): its volumes are then pending, written by
    // smt_adcensus_volume if it is called before the next compute.  SMT_BATCH_VOLUMES in the environment (read at
    // every call): `last` writes the last pair's volumes in the batch itself whatever has been lent, `all` writes
    // every pair's, as the first versions did: same-process A/Bs and tests.
    const char *venv = getenv("SMT_BATCH_VOLUMES");
    const bool all_volumes = venv && strcmp(venv, "all") == 0;
    const bool eager_last = venv && strcmp(venv, "last") == 0;
    const bool defer = !all_volumes && !eager_last && !h->vol_lent && fast_both_views(h, views);
    const int rc = adcensus_batch_pairs(h, L, R, pairs, views, dispL, dispR, sched, false, nullptr, nullptr, !all_volumes, !defer);
    h->vol_pending = defer && rc == SMT_OK;
    return rc;
}

SMT_API int smt_adcensus_volume(smt_adcensus *h, int view, float **vol)
{
    if (!h || !vol || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    // lending is for good: a pointer handed out stays valid until destroy, so nothing is deferred after this call
    h->vol_lent = true;
    const int rc = materialise_volumes(h);
    if (rc != SMT_OK) return rc;
    *vol = h->vol[view == SMT_VIEW_LEFT ? 0 : 1];
    return SMT_OK;
}

SMT_API int smt_adcensus_status(smt_adcensus *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    int f = 0;
    SMT_HIP(hipMemcpyAsync(&f, h->T.flag, 4, hipMemcpyDeviceToHost, h->stream));
    SMT_HIP(hipMemsetAsync(h->T.flag, 0, 4, h->stream));            // read-and-clear
    SMT_HIP(hipStreamSynchronize(h->stream));
    return f ? SMT_ERR_DOMAIN : SMT_OK;
}

// Host-side check of the fused launch's workgroup arithmetic (fused_grid / fused_decode, the functions the kernel runs):
// every cost group and every table group of a launch with `ncost` cost and `nprep` table workgroups is reached exactly
// once.  Needs no GPU.
SMT_API int smt_adcensus_selftest_fused_grid(int ncost, int nprep)
{
    if (ncost <= 0 || (ncost & 7) || nprep <= 0) return SMT_ERR_ARG;
    const FusedGrid f = fused_grid(ncost, nprep);
    if (f.groups < f.cgroups + f.pgroups) return SMT_ERR_STATE;
    unsigned char *seen = new (std::nothrow) unsigned char[(size_t)2 * f.groups]();
    if (!seen) return SMT_ERR_ALLOC;
    int rc = SMT_OK, ntab = 0;
    for (int g = 0; g < f.groups && rc == SMT_OK; g++) {
        int idx = -1;
        const bool table = fused_decode(f, g, idx);
        if (idx < 0 || idx >= f.groups || (!table && idx >= f.cgroups)) { rc = SMT_ERR_STATE; break; }
        unsigned char &cell = seen[(table ? f.groups : 0) + idx];
        if (cell) rc = SMT_ERR_STATE;
        cell = 1;
        ntab += table;
    }
    for (int c = 0; c < f.cgroups && rc == SMT_OK; c++) if (!seen[c]) rc = SMT_ERR_STATE;              // every cost group
    for (int t = 0; t < ntab && rc == SMT_OK; t++) if (!seen[f.groups + t]) rc = SMT_ERR_STATE;         // table groups 0 .. ntab - 1
    if (rc == SMT_OK && ntab < f.pgroups) rc = SMT_ERR_STATE;
    delete[] seen;
    return rc;
}

// Host-side check of the maps-only launch's workgroup arithmetic: with K chunks per cost workgroup (chunk_decode,
// maps_groups) every 64-pixel chunk of an H x (nbx * 64) both-views launch is reached exactly once, and with `nprep`
// table workgroups fused in (fused_grid over maps_groups() cost workgroups) so is every cost and table workgroup.
// Needs no GPU.
SMT_API int smt_adcensus_selftest_maps_grid(int nbx, int H, int K, int nprep)
{
    if (nbx <= 0 || H <= 0 || K < 1 || nprep < 0) return SMT_ERR_ARG;
    const long nb = (long)nbx * H * 2;
    const int ncost = maps_groups(nbx, H, 2, K);
    if (ncost <= 0 || (ncost & 7)) return SMT_ERR_STATE;
    unsigned char *seen = new (std::nothrow) unsigned char[(size_t)nb]();
    if (!seen) return SMT_ERR_ALLOC;
    int rc = SMT_OK;
    for (long b = 0; b < ncost && rc == SMT_OK; b++)
        for (int t = 0; t < K; t++) {
            int view, i, bx;
            if (!chunk_decode(nbx, H, 2, K, b, t, view, i, bx)) {
                // workgroup-uniform early exit: no later t of this workgroup may hold a chunk
                for (int t2 = t + 1; t2 < K && rc == SMT_OK; t2++)
                    if (chunk_decode(nbx, H, 2, K, b, t2, view, i, bx)) rc = SMT_ERR_STATE;
                break;
            }
            if (view < 0 || view > 1 || i < 0 || i >= H || bx < 0 || bx >= nbx) { rc = SMT_ERR_STATE; break; }
            unsigned char &cell = seen[((long)view * H + i) * nbx + bx];
            if (cell) { rc = SMT_ERR_STATE; break; }
            cell = 1;
            // the chunk's XCD is the workgroup's (b % 8): chunks of XCD x are the x-th contiguous eighth
            if ((((long)view * H + i) * nbx + bx) / ((nb + 7) >> 3) != (b & 7)) { rc = SMT_ERR_STATE; break; }
        }
    for (long c = 0; c < nb && rc == SMT_OK; c++) if (!seen[c]) rc = SMT_ERR_STATE;
    delete[] seen;
    if (rc == SMT_OK && nprep > 0) rc = smt_adcensus_selftest_fused_grid(ncost, nprep);
    return rc;
}

// Host-side walk of the shared maps-only form (k_cost_maps_shared's cost, edge and conversion items) over pseudo-random costs with many
// exact ties, through the kernel's own index functions.  The left pass: shared_wg_chunks / shared_run_len give a
// workgroup's sub-runs of at most SH_RUN chunks (checked against chunk_decode); a whole run is published -- the lane ->
// hypothesis split, shared_publishes and shared_ring_slot -- which must not put two columns into one ring slot, then
// flushed once over shared_run_flush_range, shared_complete sending a key to the map or to the key map.  Then the
// edge hypotheses over shared_edge_range and the conversion: as one pass over the pixels, and split into the launch's
// edge items and the next launch's conversion items, which must agree.
// The right view's pseudo-cost of (i, j', d) is the left one of (i, j' + d, d) where the identity holds and a cost of
// its own elsewhere, constant in d from W+3-j' on as the staging clamps make it.  SMT_OK iff every right pixel is
// written exactly once, with the first minimum over all its D hypotheses, every ring ends empty and the key map is
// reset.  Needs no GPU.
SMT_API int smt_adcensus_selftest_shared_keys(int H, int W, int D, int K, unsigned seed)
{
    if (H <= 0 || W <= 0 || D <= 0 || D > 256 || K < 1 || K > 64 || (long)H * W > (1L << 24)) return SMT_ERR_ARG;
    const int C = (D + 63) / 64, nbx = (W + FTJ - 1) / FTJ, idhi = shared_id_hi(W, D);
    const int pubhi = shared_pub_hi(W);
    const bool grouped = shared_ring_grouped(C, D == 64 * C ? D : 0);
    const size_t N = (size_t)H * W;
    // costs: a small palette of floats >= +0 (ties), every cost equal (seed % 3 == 1), or mostly distinct
    static const float pal[] = {0.0f, 0.0f, 0.25f, 0.25f, 1.5f, 0.7265625f, 0.7265625f, 1.9999999f, 0.25f, 1e-30f};
    auto hash_bits = [&](int i, int j, int d, unsigned salt) {
        uint32_t x = (uint32_t)i * 0x9E3779B1u ^ (uint32_t)j * 0x85EBCA77u ^ (uint32_t)d * 0xC2B2AE3Du ^ seed * 0x27D4EB2Fu ^ salt;
        x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
        float f = seed % 3 == 1 ? 0.5f : (seed % 3 == 2 && (x & 3)) ? (float)(x >> 12) * (1.0f / 1048576.0f) : pal[(x >> 4) % 10];
        uint32_t bits;
        memcpy(&bits, &f, 4);
        return bits;
    };
    auto cost_bits = [&](int i, int j, int d) { return hash_bits(i, j, d, 0u); };          // left view
    auto right_bits = [&](int i, int c, int d) {                                           // right view
        if (c >= 3 && c + d <= W - 4) return cost_bits(i, c + d, d);
        return hash_bits(i, c, std::min(d, W + 3 - c), 0x5BD1E995u);
    };
    unsigned long long *keys = new (std::nothrow) unsigned long long[N];
    unsigned *val = new (std::nothrow) unsigned[N]();
    unsigned char *nw = new (std::nothrow) unsigned char[N]();           // writers of each right pixel
    int rc = (keys && val && nw) ? SMT_OK : SMT_ERR_ALLOC;
    for (size_t p = 0; rc == SMT_OK && p < N; p++) keys[p] = SH_NOKEY;
    if (rc == SMT_OK && idhi >= 3) {
        // the taper the launch would take (maps_taper: SMT_MAPS_TAPER's forced counts; no device here, so the default
        // rule is off)
        int n2, n1;
        maps_taper(0, ((long)nbx * H + 7) >> 3, K, n2, n1);
        const int nleft = maps_groups(nbx, H, 1, K, n2, n1);
        unsigned long long ring[SH_RING_N];
        int owner[SH_RING_N];                                             // right column that holds a slot in this run
        for (long b = 0; b < nleft && rc == SMT_OK; b++) {
            for (int e = 0; e < SH_RING_N; e++) ring[e] = SH_NOKEY;
            int view, i, bx, ni, nbxn;
            int left = shared_wg_chunks(nbx, H, K, b, i, bx, n2, n1);
            for (int t = 0; t < K; t++)                                   // the chunks are chunk_decode's
                if (chunk_decode(nbx, H, 1, K, b, t, view, ni, nbxn, n2, n1) != (t < left)) rc = SMT_ERR_STATE;
            // sub-runs of SH_RUN: the publishes of the whole run, then its one flush
            for (int t = 0; left > 0 && rc == SMT_OK;) {
                const int n = shared_run_len(nbx, bx, left);
                if (n < 1 || n > SH_RUN) { rc = SMT_ERR_STATE; break; }
                for (int u = 0; u < n; u++)
                    if (!chunk_decode(nbx, H, 1, K, b, t + u, view, ni, nbxn, n2, n1) || ni != i || nbxn != bx + u) rc = SMT_ERR_STATE;
                const int S = 64 * bx, E = S + 64 * n - 1;
                for (int e = 0; e < SH_RING_N; e++) owner[e] = -1;
                for (int j = S; j <= E && j < W; j++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int k = 0; k < C; k++) {
                            const int dl = lane * C, d = dl + k, tcol = j - dl;
                            if (d >= D || !shared_publishes(j, tcol - k, W, pubhi)) continue;
                            // the kernel's slot: per pixel, or from the base of the pixel's group in its wave's walk
                            const int u = grouped ? ((j - S) % (FPW * n)) % C : 0;
                            const int s = shared_ring_slot(tcol - u, u, k, C);
                            if (s < 0 || s >= SH_RING_N) { rc = SMT_ERR_STATE; continue; }
                            if (owner[s] != -1 && owner[s] != tcol - k) rc = SMT_ERR_STATE;   // two live columns in a slot
                            owner[s] = tcol - k;
                            ring[s] = std::min(ring[s], shared_key(cost_bits(i, j, d), d));
                        }
                int lo, hi;
                shared_run_flush_range(S, E, D, pubhi, lo, hi);
                for (int c = lo; c <= hi; c++) {
                    const int s = c & (SH_RING - 1);
                    unsigned long long k = ring[s];
                    ring[s] = SH_NOKEY;
                    if (s < shared_ring_spill(C, grouped)) { k = std::min(k, ring[SH_RING + s]); ring[SH_RING + s] = SH_NOKEY; }
                    const size_t p = (size_t)i * W + c;
                    if (shared_complete(c, S, E, D, idhi)) {
                        if (k == SH_NOKEY) rc = SMT_ERR_STATE;
                        val[p] = (unsigned)k; nw[p]++;
                    } else if (k != SH_NOKEY) keys[p] = std::min(keys[p], k);
                }
                for (int e = 0; e < SH_RING_N; e++) if (ring[e] != SH_NOKEY) rc = SMT_ERR_STATE;   // free for the next run
                left -= n; t += n; bx += n;
                if (bx == nbx) { bx = 0; i++; }
            }
        }
        // The split finish on copies of the state behind the left pass: the edge items' merges (seed & 4: in front of
        // the publishes' merges instead of behind them -- minima commute) and direct writes, then the conversion over
        // the flat key map.  Its result must be the single pass's below.
        unsigned long long *keys2 = new (std::nothrow) unsigned long long[N];
        unsigned *val2 = new (std::nothrow) unsigned[N];
        unsigned char *nw2 = new (std::nothrow) unsigned char[N];
        if (!keys2 || !val2 || !nw2) rc = SMT_ERR_ALLOC;
        if (rc == SMT_OK) {
            memcpy(val2, val, N * sizeof(unsigned));
            memcpy(nw2, nw, N);
            const bool edges_first = (seed & 4u) != 0;
            for (size_t p = 0; p < N; p++) keys2[p] = edges_first ? SH_NOKEY : keys[p];
            const int nedge = shared_edge_items(H, W, D), ncol = shared_edge_col_items(H, W, D);
            for (int item = 0; item < nedge; item++) {
                if (item < ncol) {
                    for (int it = 0; it < SH_EDGE_PX / 256; it++)
                        for (int tid = 0; tid < 256; tid++) {
                            int i, c;
                            if (!shared_edge_px(item, it, tid, H, W, D, i, c)) continue;
                            const size_t p = (size_t)i * W + c;
                            int lo, hi;
                            shared_edge_range(c, W, D, lo, hi);
                            unsigned long long k = SH_NOKEY;
                            for (int d = lo; d <= hi; d++) k = std::min(k, shared_key(right_bits(i, c, d), d));
                            if (k == SH_NOKEY) rc = SMT_ERR_STATE;                      // an empty edge range
                            if (c > W - 4) { val2[p] = (unsigned)k; nw2[p]++; }
                            else keys2[p] = std::min(keys2[p], k);
                        }
                } else {
                    for (int it = 0; it < SH_EDGE0_PX / 4; it++)
                        for (int wv = 0; wv < 4; wv++) {
                            int i, c;
                            if (!shared_edge0_px(item - ncol, it, wv, H, i, c)) continue;
                            const size_t p = (size_t)i * W + c;
                            int lo, hi;
                            shared_edge_range(c, W, D, lo, hi);
                            unsigned long long k = SH_NOKEY;
                            for (int d = lo; d <= hi; d++) k = std::min(k, shared_key(right_bits(i, c, d), d));
                            val2[p] = (unsigned)k; nw2[p]++;
                        }
                }
            }
            if (edges_first) for (size_t p = 0; p < N; p++) keys2[p] = std::min(keys2[p], keys[p]);
            for (int i = 0; i < H; i++)                                                 // the invariant of the key map
                for (int c = 0; c < W; c++)
                    if ((c < 3 || c > W - 4) && keys2[(size_t)i * W + c] != SH_NOKEY) rc = SMT_ERR_STATE;
            const int nconv = shared_conv_items(H, W);
            for (int item = 0; item < nconv; item++)
                for (int it = 0; it < SH_CONV_PX / 512; it++)
                    for (int tid = 0; tid < 256; tid++) {
                        long p;
                        if (!shared_conv_px(item, it, tid, (long)N, p)) continue;
                        for (long e = p; e < p + 2 && e < (long)N; e++)
                            if (keys2[e] != SH_NOKEY) { val2[e] = (unsigned)keys2[e]; nw2[e]++; keys2[e] = SH_NOKEY; }
                    }
        }
        // the single pass
        for (int i = 0; i < H; i++)
            for (int c = 0; c < W; c++) {
                const size_t p = (size_t)i * W + c;
                if (shared_in_set(c, idhi)) {
                    if (keys[p] != SH_NOKEY) { val[p] = (unsigned)keys[p]; nw[p]++; keys[p] = SH_NOKEY; }
                    continue;
                }
                unsigned long long k = c >= 3 && c <= W - 4 ? keys[p] : SH_NOKEY;
                if (c >= 3 && c <= W - 4) keys[p] = SH_NOKEY;
                int lo, hi;
                shared_edge_range(c, W, D, lo, hi);
                for (int d = lo; d <= hi; d++) k = std::min(k, shared_key(right_bits(i, c, d), d));
                if (k == SH_NOKEY) rc = SMT_ERR_STATE;
                val[p] = (unsigned)k; nw[p]++;
            }
        for (size_t p = 0; p < N && rc == SMT_OK; p++)
            if (val2[p] != val[p] || nw2[p] != nw[p] || keys2[p] != keys[p]) rc = SMT_ERR_STATE;
        delete[] keys2; delete[] val2; delete[] nw2;
    }
    for (int i = 0; i < H && rc == SMT_OK; i++)
        for (int c = 0; c < W && rc == SMT_OK; c++) {
            const size_t p = (size_t)i * W + c;
            if (idhi < 3) { if (nw[p]) rc = SMT_ERR_STATE; continue; }   // the two-view kernel serves this shape
            if (keys[p] != SH_NOKEY) rc = SMT_ERR_STATE;
            float mn = 0.0f;
            int want = 0;
            for (int d = 0; d < D; d++) {
                const uint32_t bits = right_bits(i, c, d);
                float f;
                memcpy(&f, &bits, 4);
                if (d == 0 || f < mn) { mn = f; want = d; }
            }
            if (nw[p] != 1 || val[p] != (unsigned)want) rc = SMT_ERR_STATE;
        }
    delete[] keys; delete[] val; delete[] nw;
    return rc;
}

// Host-side check of a shared launch's auxiliary list (fused_grid / fused_decode over ncost cost workgroups and
// nprep + nconv + nedge auxiliary items, shared_aux_decode): every cost workgroup and every table, conversion and edge
// item is decoded exactly once.  Needs no GPU.
// With a tapered tail (cbody > 0: the cost groups of the body) and a body that takes the auxiliary groups, none of them
// follows cost group cbody, the first tapered one; cbody = 0 must give the plain placement.
static int shared_aux_grid_check(int ncost, int nprep, int nedge, int nconv, int cbody)
{
    if (ncost <= 0 || (ncost & 7) || nprep < 0 || nedge < 0 || nconv < 0 || cbody < 0) return SMT_ERR_ARG;
    const int naux = nprep + nconv + nedge;
    const FusedGrid f = fused_grid(ncost, naux, cbody), f0 = fused_grid(ncost, naux);
    if (8L * f.groups < (long)ncost + naux) return SMT_ERR_STATE;
    if (cbody == 0 && (f.every != f0.every || f.slots != f0.slots || f.groups != f0.groups)) return SMT_ERR_STATE;
    const bool in_body = cbody > 0 && cbody < f.cgroups && f.pgroups > 0 && cbody >= f.pgroups;
    unsigned char *cost = new (std::nothrow) unsigned char[(size_t)ncost]();
    unsigned char *aux = new (std::nothrow) unsigned char[(size_t)naux + 1]();
    int rc = (cost && aux) ? SMT_OK : SMT_ERR_ALLOC;
    bool tapered = false;                                                 // a tapered cost group has been dispatched
    for (long blk = 0; blk < 8L * f.groups && rc == SMT_OK; blk++) {
        int idx = -1;
        const bool table = fused_decode(f, (int)(blk >> 3), idx);
        if (idx < 0) { rc = SMT_ERR_STATE; break; }
        const long b = (long)idx * 8 + (blk & 7);
        if (!table) {
            if (b >= ncost || cost[b]++) rc = SMT_ERR_STATE;
            if (in_body && idx >= cbody) tapered = true;
            continue;
        }
        if (in_body && tapered) rc = SMT_ERR_STATE;
        int item = -1;
        const int kind = shared_aux_decode((int)b, nprep, nconv, nedge, item);
        if (kind == AUX_NONE) { if (b < naux) rc = SMT_ERR_STATE; continue; }
        const int n = kind == AUX_PREP ? nprep : kind == AUX_CONV ? nconv : nedge;
        const int base = kind == AUX_PREP ? 0 : kind == AUX_CONV ? nprep : nprep + nconv;
        if (item < 0 || item >= n || base + item != b || aux[b]++) rc = SMT_ERR_STATE;
    }
    for (int c = 0; c < ncost && rc == SMT_OK; c++) if (cost[c] != 1) rc = SMT_ERR_STATE;
    for (int a = 0; a < naux && rc == SMT_OK; a++) if (aux[a] != 1) rc = SMT_ERR_STATE;
    delete[] cost; delete[] aux;
    return rc;
}
SMT_API int smt_adcensus_selftest_shared_aux_grid(int ncost, int nprep, int nedge, int nconv)
{
    return shared_aux_grid_check(ncost, nprep, nedge, nconv, 0);
}

// Host-side check of the shared launch of an H x W x D pair with K chunks per cost workgroup, through the functions the
// kernel runs: the launch's counts as launch_fast computes them (first: no conversion carried; last: no table tiles)
// pass smt_adcensus_selftest_shared_aux_grid; the conversion items cover each of the H*W keys exactly once; the edge
// items cover each pixel of the columns idhi+1 .. W-1 and 0..2 exactly once and no other; the edge range of every
// column idhi < c <= W-4 is not empty.  Needs no GPU.
SMT_API int smt_adcensus_selftest_shared_aux(int H, int W, int D, int K, int first, int last)
{
    if (H <= 0 || W <= 0 || D <= 0 || D > 256 || K < 1 || K > 64 || (long)H * W > (1L << 24)) return SMT_ERR_ARG;
    const int idhi = shared_id_hi(W, D), nbx = (W + FTJ - 1) / FTJ;
    if (idhi < 3) return SMT_ERR_ARG;                                     // the two-view kernel serves this shape
    int ptx;
    int n2, n1;                                                           // the launch's taper (maps_taper), no device
    maps_taper(0, ((long)nbx * H + 7) >> 3, K, n2, n1);
    const int ncost = maps_groups(nbx, H, 1, K, n2, n1), nprep = last ? 0 : prep_items(H, W, ptx);
    const int nconv = first ? 0 : shared_conv_items(H, W), nedge = shared_edge_items(H, W, D);
    int rc = shared_aux_grid_check(ncost, nprep, nedge, nconv, maps_body_groups(nbx, H, 1, K, n2, n1));
    if (rc != SMT_OK) return rc;
    const long N = (long)H * W;
    unsigned char *seen = new (std::nothrow) unsigned char[(size_t)N]();
    if (!seen) return SMT_ERR_ALLOC;
    for (int item = 0; item < shared_conv_items(H, W); item++)
        for (int it = 0; it < SH_CONV_PX / 512; it++)
            for (int tid = 0; tid < 256; tid++) {
                long p;
                long p0;
                (void)shared_conv_px(item, 0, tid, N, p0);
                const bool in = shared_conv_px(item, it, tid, N, p);
                if (p != p0 + 512L * it) rc = SMT_ERR_STATE;              // the kernel steps one pointer by 512 keys
                if (!in) continue;
                if (p < 0 || (p & 1)) { rc = SMT_ERR_STATE; continue; }
                for (long e = p; e < p + 2 && e < N; e++) if (seen[e]++) rc = SMT_ERR_STATE;
            }
    for (long p = 0; p < N; p++) { if (seen[p] != 1) rc = SMT_ERR_STATE; seen[p] = 0; }
    const int ncol = shared_edge_col_items(H, W, D);
    for (int item = 0; item < nedge; item++)
        for (int it = 0; it < (item < ncol ? SH_EDGE_PX / 256 : SH_EDGE0_PX / 4); it++)
            for (int t = 0; t < (item < ncol ? 256 : 4); t++) {
                int i = -1, c = -1;
                if (!(item < ncol ? shared_edge_px(item, it, t, H, W, D, i, c) : shared_edge0_px(item - ncol, it, t, H, i, c)))
                    continue;
                const bool in = i >= 0 && i < H && (item < ncol ? c > idhi && c < W : c >= 0 && c < 3);
                if (!in || seen[(long)i * W + c]++) rc = SMT_ERR_STATE;
            }
    for (int i = 0; i < H; i++)
        for (int c = 0; c < W; c++) {
            const bool edge = c < 3 || c > idhi;
            if (seen[(long)i * W + c] != (edge ? 1 : 0)) rc = SMT_ERR_STATE;
            int lo, hi;
            shared_edge_range(c, W, D, lo, hi);
            if (c > idhi && c <= W - 4 && (lo > hi || lo < 1 || c + lo != W - 3)) rc = SMT_ERR_STATE;
            if (edge && (lo < 0 || hi > D - 1 || lo > hi)) rc = SMT_ERR_STATE;
        }
    delete[] seen;
    return rc;
}

// Host-side check of the span rule (maps_span, maps_span_groups) over the 8 slices of a launch of nb chunks with K
// chunks per workgroup and tails n2, n1: every chunk 0 .. nb-1 belongs to exactly one group, no group crosses its slice
// or has more than K chunks, no group before the last of a slice is empty, the group count is the companion's, and
// with n1 = n2 = 0 every group is the plain rule's [g K, g K + K).  With tails that fit the slice, the slice's last n1
// groups have 1 chunk and the n2 before them max(1, K / 2).  Needs no GPU.
SMT_API int smt_adcensus_selftest_spans(long nb, int K, int n2, int n1)
{
    if (nb <= 0 || nb > (1L << 28) || K < 1 || K > 64 || n2 < 0 || n1 < 0) return SMT_ERR_ARG;
    const long per = (nb + 7) >> 3, ng = maps_span_groups(per, K, n2, n1);
    unsigned char *seen = new (std::nothrow) unsigned char[(size_t)nb]();
    if (!seen) return SMT_ERR_ALLOC;
    int rc = SMT_OK, e2 = n2, e1 = n1;
    const long body = maps_span_tails(per, K, e2, e1);
    const int K2 = K > 1 ? K >> 1 : 1;
    if (body < 0 || e2 > n2 || e1 > n1 || body + (long)e2 * K2 + e1 != per || ng != (body + K - 1) / K + e2 + e1) rc = SMT_ERR_STATE;
    for (int x = 0; x < 8 && rc == SMT_OK; x++) {
        long expect = 0;                                                  // groups are consecutive in the slice
        for (long g = 0; g < ng + 2 && rc == SMT_OK; g++) {
            long first = -1;
            const int m = maps_span(per, K, n2, n1, g, first);
            if (g >= ng) { if (m != 0) rc = SMT_ERR_STATE; continue; }
            if (m < 1 || m > K || first != expect || first + m > per) { rc = SMT_ERR_STATE; break; }
            if (g >= ng - e1 ? m != 1 : g >= ng - e1 - e2 ? m != K2 : (m != K && g != ng - e1 - e2 - 1)) rc = SMT_ERR_STATE;
            if (n1 == 0 && n2 == 0) {
                const long cl = g * K, lim = per - cl < K ? per - cl : K;      // the plain rule
                if (first != cl || m != lim) rc = SMT_ERR_STATE;
            }
            expect = first + m;
            for (long c = x * per + first; c < x * per + first + m; c++)
                if (c < nb && seen[c]++) rc = SMT_ERR_STATE;
        }
        if (expect != per) rc = SMT_ERR_STATE;
    }
    for (long c = 0; c < nb && rc == SMT_OK; c++) if (seen[c] != 1) rc = SMT_ERR_STATE;
    // the launch's own decode agrees with the span: shared_wg_chunks over a one-chunk-per-row image
    for (long b = 0; b < 8 * ng && rc == SMT_OK && nb <= (1L << 20); b++) {
        long first;
        int i = -1, bx = -1;
        const int m = maps_span(per, K, n2, n1, b >> 3, first), got = shared_wg_chunks(1, (int)nb, K, b, i, bx, n2, n1);
        const long c = (b & 7) * per + first, want = c >= nb ? 0 : (nb - c < m ? nb - c : m);
        if (got != want || (got > 0 && (i != c || bx != 0))) rc = SMT_ERR_STATE;
    }
    delete[] seen;
    return rc;
}

// Host-side check of the rank table (build_rank) against the float sums it stands for: for sigmaC, sigmaS > 0, every
// sum lut[ad] + lut[256 + hd] is finite and >= +0, ranks are dense from 0, and for any two entries rank order equals
// float order (equal ranks exactly when the bit patterns are equal).  Needs no GPU.
// Host-side proof of the chained schedule's order (include/smt.h): chain_plan's list for `pairs` pairs on `chains`
// chains whose counters stand at c0, c1, c2, under `order` and `flags`, with happens-before computed over its
// operations -- program order per stream plus every record -> wait edge, between a start and an end on the caller's
// stream.  Needs no GPU.
SMT_API int smt_adcensus_selftest_chains(int pairs, int chains, long c0, long c1, long c2, int order, unsigned flags)
{
    if (pairs < 1 || pairs > 512) return SMT_ERR_ARG;
    const long count0[SMT_MAX_CHAINS] = {c0, c1, c2};
    std::vector<ChainOp> ops;
    const int prc = chain_plan(pairs, chains, count0, order, flags, ops);
    if (prc != SMT_OK) return prc;
    const int nc = std::min(chains, pairs);
    // node 0: the call's start on the caller's stream; node m + 1: its end there
    const int m = (int)ops.size(), M = m + 2;
    auto stream_of = [&](int k) { return k == 0 || k == M - 1 ? 0 : ops[k - 1].stream; };
    std::vector<std::vector<unsigned char>> before(M, std::vector<unsigned char>(M, 0));   // before[i][j]: j happens before i
    int last_on[SMT_MAX_CHAINS] = {-1, -1, -1}, recorded[SMT_MAX_CHAINS] = {-1, -1, -1};
    auto edge = [&](int from, int to) {
        for (int j = 0; j < M; j++) before[to][j] |= before[from][j];
        before[to][from] = 1;
    };
    for (int k = 0; k < M; k++) {
        const int s = stream_of(k);
        if (s < 0 || s >= SMT_MAX_CHAINS) return SMT_ERR_STATE;
        if (last_on[s] >= 0) edge(last_on[s], k);
        last_on[s] = k;
        if (k == 0 || k == M - 1) continue;
        const ChainOp &o = ops[k - 1];
        if (o.kind == CH_RECORD) recorded[o.ev] = k;
        if (o.kind == CH_WAIT) {
            if (recorded[o.ev] < 0) return SMT_ERR_STATE;    // an event is recorded before anything waits on it
            edge(recorded[o.ev], k);
        }
    }
    auto hb = [&](int a, int b) { return before[b][a] != 0; };
    // nothing starts ahead of the call (the fork) and nothing is left un-joined
    for (int k = 1; k < M - 1; k++)
        if (!hb(0, k) || !hb(k, M - 1)) return SMT_ERR_STATE;
    std::vector<int> launches(pairs, 0), converted(pairs, 0);
    for (int k = 1; k < M - 1; k++) {
        const ChainOp &o = ops[k - 1];
        if (o.kind == CH_PAIR) {
            if (o.pair < 0 || o.pair >= pairs || o.chain != o.pair % nc) return SMT_ERR_STATE;
            if (o.stream != (order == CHAIN_ORDER_PAIRS ? 0 : o.chain)) return SMT_ERR_STATE;
            launches[o.pair]++;
            // the set it reads was built for this pair by a launch before it, and whatever else builds that set does so
            // before that builder or behind this reader
            int builder = -1;
            for (int j = 1; j < M - 1; j++)
                if (ops[j - 1].ts_built == o.ts_read && ops[j - 1].built_for == o.pair && hb(j, k)) builder = builder < 0 ? j : -2;
            if (builder < 0) return SMT_ERR_STATE;
            for (int j = 1; j < M - 1; j++)
                if (j != builder && ops[j - 1].ts_built == o.ts_read && !hb(j, builder) && !hb(k, j)) return SMT_ERR_STATE;
            if (o.key_merged >= 0 && o.key_merged == o.key_conv) return SMT_ERR_STATE;
        }
        if (o.key_conv >= 0) {
            if (o.conv_pair < 0 || o.conv_pair >= pairs) return SMT_ERR_STATE;
            converted[o.conv_pair]++;
        }
    }
    const bool any_shared = (flags & CHAIN_SHARED) != 0;
    for (int b = 0; b < pairs; b++) {
        const bool shared = any_shared && !(b + 1 == pairs && (flags & CHAIN_LAST_VOLUMES));
        if (launches[b] != 1 || converted[b] != (shared ? 1 : 0)) return SMT_ERR_STATE;
    }
    // every key map: merged, converted into the merging pair's map, merged again ..., by operations in a total order
    for (int key = 0; key < 2 * SMT_MAX_CHAINS; key++) {
        int prev = -1, merged_by = -1;                       // the last operation on the key; the pair whose keys it holds
        for (int k = 1; k < M - 1; k++) {
            const ChainOp &o = ops[k - 1];
            if (o.key_conv == key) {
                if (merged_by < 0 || o.conv_pair != merged_by || !hb(prev, k)) return SMT_ERR_STATE;
                prev = k; merged_by = -1;
            }
            if (o.key_merged == key) {
                if (merged_by >= 0 || (prev >= 0 && !hb(prev, k))) return SMT_ERR_STATE;
                prev = k; merged_by = o.pair;
            }
        }
        if (merged_by >= 0) return SMT_ERR_STATE;            // a conversion left pending
    }
    return SMT_OK;
}

SMT_API int smt_adcensus_selftest_cost_rank(float sigmaC, float sigmaS)
{
    if (!(sigmaC > 0.0f) || !(sigmaS > 0.0f)) return SMT_ERR_ARG;
    float lut[320];
    build_lut(sigmaC, sigmaS, lut);
    uint16_t *rank = new (std::nothrow) uint16_t[RANK_N];
    float *sum = new (std::nothrow) float[RANK_N];
    float *uniq = new (std::nothrow) float[RANK_N];
    int rc = (rank && sum && uniq && build_rank(lut, rank)) ? SMT_OK : SMT_ERR_ALLOC;
    int nu = 0;
    if (rc == SMT_OK) {
        for (int e = 0; e < RANK_N; e++) {
            sum[e] = lut[e >> 6] + lut[256 + (e & 63)];
            uint32_t bits;
            memcpy(&bits, &sum[e], 4);
            if (!(sum[e] >= 0.0f && sum[e] < INFINITY) || (bits >> 31)) rc = SMT_ERR_STATE;   // finite, >= +0
            uniq[e] = sum[e];
        }
        // distinct values in float order; the rank of an entry must be the number of distinct values below it
        std::sort(uniq, uniq + RANK_N);
        nu = (int)(std::unique(uniq, uniq + RANK_N) - uniq);
    }
    for (int e = 0; e < RANK_N && rc == SMT_OK; e++) {
        const int below = (int)(std::lower_bound(uniq, uniq + nu, sum[e]) - uniq);
        if (rank[e] != below || uniq[below] != sum[e]) rc = SMT_ERR_STATE;
    }
    // pairwise on a sample of entries: rank order == float order == uint32 bit order
    for (int a = 0; a < RANK_N && rc == SMT_OK; a += 37)
        for (int b = 0; b < RANK_N && rc == SMT_OK; b += 41) {
            uint32_t ba, bb;
            memcpy(&ba, &sum[a], 4); memcpy(&bb, &sum[b], 4);
            if ((rank[a] < rank[b]) != (sum[a] < sum[b]) || (rank[a] == rank[b]) != (ba == bb) || (ba < bb) != (sum[a] < sum[b]))
                rc = SMT_ERR_STATE;
        }
    delete[] rank; delete[] sum; delete[] uniq;
    return rc;
}

SMT_API int smt_adcensus_force_generic(smt_adcensus *h, int on)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->force_generic = on != 0;
    return SMT_OK;
}

SMT_API int smt_adcensus_timing(smt_adcensus *h, int enable)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (enable && !h->ev) {
        h->ev = new (std::nothrow) hipEvent_t[SMT_TIMING_SLOTS * 4];
        h->ev_merged = new (std::nothrow) bool[SMT_TIMING_SLOTS]();
        if (!h->ev || !h->ev_merged) return SMT_ERR_ALLOC;
        for (int k = 0; k < SMT_TIMING_SLOTS * 4; k++) SMT_HIP(hipEventCreate(&h->ev[k]));
    }
    if (enable < 0) return SMT_ERR_ARG;
    h->timing = enable != 0;
    h->timing_stride = enable > 0 ? enable : 1;
    h->n_timed = 0;
    h->n_seen = 0;
    return SMT_OK;
}

SMT_API int smt_adcensus_kernel_times(smt_adcensus *h, float *prep_ms, float *cost_ms, int capacity,
                                      int *count)
{
    if (!h || !count || capacity < 0) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (!h->ev) return SMT_ERR_STATE;
    long n = h->n_timed < SMT_TIMING_SLOTS ? h->n_timed : SMT_TIMING_SLOTS;
    if (n > capacity) n = capacity;
    const long first = h->n_timed - n;
    for (long k = 0; k < n; k++) {
        hipEvent_t *ev = h->ev + 4 * ((first + k) % SMT_TIMING_SLOTS);
        SMT_HIP(hipEventSynchronize(ev[3]));
        float a = 0, b = 0;
        SMT_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));      // table kernels, internal stream
        const long slot = (first + k) % SMT_TIMING_SLOTS;
        SMT_HIP(hipEventElapsedTime(&b, ev[h->ev_merged[slot] ? 1 : 2], ev[3]));   // cost kernel(s), caller's stream
        if (prep_ms) prep_ms[k] = a;
        if (cost_ms) cost_ms[k] = b;
    }
    *count = (int)n;
    return SMT_OK;
}

// Measurement hook (bench.py): see include/smt.h.
namespace {
// everything smt_adcensus_diag_impl acquires, released on every exit path (its SMT_HIP early returns included)
struct DiagResources {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    unsigned long long *stamp = nullptr;
    unsigned long long *hs = nullptr;
    float *ratio = nullptr;
    ~DiagResources()
    {
        for (auto &x : e) if (x) (void)hipEventDestroy(x);
        if (stamp) (void)hipFree(stamp);
        delete[] hs;
        delete[] ratio;
    }
};
}  // namespace

static int smt_adcensus_diag_impl(smt_adcensus *h, int reps, float *sclk_mhz, float *cost_ms, float *store_only_ms, DiagResources &res)
{
    if (h->chain[0].n_pairs == 0) return SMT_ERR_STATE;      // needs the tables of a computed pair
    const int D = h->D, C = D / 64;
    if (D % 64 != 0 || C < 1 || C > 4) return SMT_ERR_ARG;
    const int nbx = (h->W + FTJ - 1) / FTJ;
    const unsigned nblk = (unsigned)(((long)nbx * h->H * 2 + 7) / 8 * 8);
    hipEvent_t (&e)[3] = res.e;
    for (auto &x : e) SMT_HIP(hipEventCreate(&x));
    if (smt_malloc((void **)&res.stamp, (size_t)nblk * 32) != SMT_OK) return SMT_ERR_ALLOC;
    unsigned long long *stamp = res.stamp;
    SMT_HIP(hipMemsetAsync(stamp, 0, (size_t)nblk * 32, h->stream));
    Tables T = h->T;
    T.stamp = stamp;
    SMT_HIP(hipEventRecord(e[0], h->stream));
    for (int r = 0; r < reps; r++) {
        switch (C) {
        case 1: hipLaunchKernelGGL((k_store_only2<1>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, h->vol[0], h->vol[1], nbx); break;
        case 2: hipLaunchKernelGGL((k_store_only2<2>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, h->vol[0], h->vol[1], nbx); break;
        case 3: hipLaunchKernelGGL((k_store_only2<3>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, h->vol[0], h->vol[1], nbx); break;
        default: hipLaunchKernelGGL((k_store_only2<4>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, h->vol[0], h->vol[1], nbx); break;
        }
    }
    SMT_HIP(hipEventRecord(e[1], h->stream));
    // the real kernel with stamps, last, so that the volumes hold the pair's costs again afterwards
    for (int r = 0; r < reps; r++) {
        switch (C) {
        case 1: if (h->plain_stores) hipLaunchKernelGGL((k_cost_fast2<1, true, false>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            else hipLaunchKernelGGL((k_cost_fast2<1, true, true>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            break;
        case 2: if (h->plain_stores) hipLaunchKernelGGL((k_cost_fast2<2, true, false>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            else hipLaunchKernelGGL((k_cost_fast2<2, true, true>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            break;
        case 3: if (h->plain_stores) hipLaunchKernelGGL((k_cost_fast2<3, true, false>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            else hipLaunchKernelGGL((k_cost_fast2<3, true, true>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            break;
        default: if (h->plain_stores) hipLaunchKernelGGL((k_cost_fast2<4, true, false>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            else hipLaunchKernelGGL((k_cost_fast2<4, true, true>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            break;
        }
    }
    SMT_HIP(hipEventRecord(e[2], h->stream));
    SMT_LAUNCH_CHECK();
    h->vol_pending = false;                                  // the stamped launches have just written the pair's volumes
    SMT_HIP(hipEventSynchronize(e[2]));
    float a = 0, b = 0;
    SMT_HIP(hipEventElapsedTime(&a, e[0], e[1]));
    SMT_HIP(hipEventElapsedTime(&b, e[1], e[2]));
    if (store_only_ms) *store_only_ms = a / reps;
    if (cost_ms) *cost_ms = b / reps;
    if (sclk_mhz) {
        // stamps of the last launch: median over workgroups of d(s_memtime) / d(s_memrealtime) * 100 MHz
        unsigned long long *hs = res.hs = new (std::nothrow) unsigned long long[(size_t)nblk * 4];
        float *ratio = res.ratio = new (std::nothrow) float[nblk];
        if (!hs || !ratio) return SMT_ERR_ALLOC;
        SMT_HIP(hipMemcpy(hs, stamp, (size_t)nblk * 32, hipMemcpyDeviceToHost));
        size_t n = 0;
        for (unsigned k = 0; k < nblk; k++) {
            const unsigned long long dt = hs[4 * k + 2] - hs[4 * k], dr = hs[4 * k + 3] - hs[4 * k + 1];
            if (hs[4 * k + 3] != 0 && dr >= 200) ratio[n++] = (float)((double)dt / (double)dr * 100.0);
        }
        if (n) { std::nth_element(ratio, ratio + n / 2, ratio + n); *sclk_mhz = ratio[n / 2]; }
        else *sclk_mhz = 0.0f;
    }
    return SMT_OK;
}

SMT_API int smt_adcensus_diag(smt_adcensus *h, int reps, float *sclk_mhz, float *cost_ms, float *store_only_ms)
{
    if (!h || reps <= 0 || reps > 1000) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    DiagResources res;
    return smt_adcensus_diag_impl(h, reps, sclk_mhz, cost_ms, store_only_ms, res);
}

SMT_API int smt_wta(const float *vol, int H, int W, int D, float *disp, void *stream)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || (size_t)H * W >= ((size_t)1 << 31))
        return SMT_ERR_ARG;                              // pixel indices are int; hypothesis addresses are (size_t)p * D
    const int N = H * W;
    dim3 grid((N + 3) / 4);
    const int C = (D + 63) / 64;
    hipStream_t st = smt_stream(stream);
    const bool full = (D == 64 * C) && C <= 4;
#define SMT_WTA(CC)                                                                                  \
    do {                                                                                             \
        if (full) hipLaunchKernelGGL((k_wta<CC, true>), grid, dim3(NT), 0, st, vol, N, D, disp);     \
        else hipLaunchKernelGGL((k_wta<CC, false>), grid, dim3(NT), 0, st, vol, N, D, disp);         \
    } while (0)
    switch (C) {
    case 1: SMT_WTA(1); break;
    case 2: SMT_WTA(2); break;
    case 3: SMT_WTA(3); break;
    case 4: SMT_WTA(4); break;
    case 5: hipLaunchKernelGGL((k_wta<5, false>), grid, dim3(NT), 0, st, vol, N, D, disp); break;
    case 6: hipLaunchKernelGGL((k_wta<6, false>), grid, dim3(NT), 0, st, vol, N, D, disp); break;
    case 7: hipLaunchKernelGGL((k_wta<7, false>), grid, dim3(NT), 0, st, vol, N, D, disp); break;
    default: hipLaunchKernelGGL((k_wta<8, false>), grid, dim3(NT), 0, st, vol, N, D, disp); break;
    }
#undef SMT_WTA
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}
