// The device code of the AD-Census family: table, cost, maps-only and shared kernels, in one anonymous namespace.
// Included by adcensus.hip alone; the formulation is described there, the index rules live in adcensus_rules.h.
#include "smt_common.h"
#include "adcensus_rules.h"

namespace {

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

struct __attribute__((aligned(16))) Anchor { uint64_t cen, mask; };

// LDS of the maps-only kernel (k_cost_maps2p): its table plus the staged operands, one set shared by both views
// (the volume-writing kernels keep per-instantiation static arrays).  The table workgroups stage their tile in tab.
constexpr int MODE_VOLUME = 0, MODE_MAPS_FLOAT = 1, MODE_MAPS_RANK = 2;         // cost_fast_body's forms
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

// Workgroup -> its one 64-pixel chunk: the K = 1 form of chunk_decode (adcensus_rules.h, where the order is described).
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

}  // namespace
