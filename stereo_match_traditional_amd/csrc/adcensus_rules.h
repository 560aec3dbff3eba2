// What the AD-Census kernels (adcensus_kernels.h), launchers (adcensus.hip) and host selftests (adcensus_selftest.hip)
// must agree on: sizes, index rules, chain_plan, host-built tables, environment readers.  No HIP; internal linkage.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/smt.h"

#ifdef __HIPCC__
#define ADC_HD __host__ __device__
#else
#define ADC_HD
#endif

namespace {

constexpr int TJ = 64;        // k_cost: pixels per workgroup
constexpr int NT = 256;       // threads per workgroup (4 waves)
constexpr int PTW = 64;                                     // k_prep's tile: 64 columns x 32 rows per workgroup
constexpr int PTH = 32;
constexpr int PNT = 256;                                    // each thread does one column of 8 rows
#ifndef SMT_FTJ
#define SMT_FTJ 64
#endif
constexpr int FTJ = SMT_FTJ;      // pixels per workgroup
constexpr int FPW = FTJ / 4;      // consecutive pixels per wave

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
ADC_HD inline int shared_id_hi(int W, int D) { return W - 3 - D; }           // the set is [3, hi]; empty when hi < 3
ADC_HD inline int shared_pub_hi(int W) { return W - 4; }                     // last published right column
ADC_HD inline bool shared_in_set(int c, int hi) { return (unsigned)(c - 3) <= (unsigned)(hi - 3) && hi >= 3; }
// left pixel j publishes a hypothesis to right column c = j - d
ADC_HD inline bool shared_publishes(int j, int c, int W, int pubhi) { return j <= W - 4 && shared_in_set(c, pubhi); }
ADC_HD inline unsigned long long shared_key(unsigned cost_bits, int d) { return ((unsigned long long)cost_bits << 32) | (unsigned)d; }
// A lane publishes its C hypotheses d = dl .. dl+C-1 of left pixel j to the right columns t - k, t = j - dl: ring slot
// base + (C-1-k) with base = (t - (C-1)) mod 512, one address computation per pixel.  A column c with c mod 512 < C-1
// can therefore land in slot c mod 512 or in the spill slot 512 + c mod 512; the flush takes the minimum of the two.
ADC_HD inline int shared_ring_base(int t, int C) { return (int)((unsigned)(t - (C - 1)) & (unsigned)(SH_RING - 1)); }
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
ADC_HD constexpr bool shared_walk_groups(int C, int Dfull) { return C == 3 && Dfull == 192; }
ADC_HD constexpr bool shared_ring_grouped(int C, int Dfull) { return C == 3 && Dfull == 192; }
static_assert(!shared_ring_grouped(3, 192) || shared_walk_groups(3, 192), "");
ADC_HD inline int shared_ring_slot(int t0, int u, int k, int C) { return shared_ring_base(t0, C) + u + (C - 1 - k); }
ADC_HD constexpr int shared_ring_spill(int C, bool grouped) { return grouped ? 2 * (C - 1) : C - 1; }
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
ADC_HD inline long maps_span_tails(long per, int K, int &n2, int &n1)   // -> chunks of the body
{
    const int K2 = K > 1 ? K >> 1 : 1;
    if (n1 < 0) n1 = 0;
    if (n2 < 0) n2 = 0;
    if (n1 > per) n1 = (int)per;
    const long rem = per - n1;
    if ((long)n2 * K2 > rem) n2 = (int)(rem / K2);
    return rem - (long)n2 * K2;
}
ADC_HD inline int maps_span(long per, int K, int n2, int n1, long g, long &first)
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
ADC_HD inline long maps_span_body(long per, int K, int n2, int n1)
{
    return (maps_span_tails(per, K, n2, n1) + K - 1) / K;
}
ADC_HD inline long maps_span_groups(long per, int K, int n2, int n1)
{
    const long nbody = maps_span_body(per, K, n2, n1);               // shrinks n2, n1 by value only: shrink again
    (void)maps_span_tails(per, K, n2, n1);
    return nbody + n2 + n1;
}
ADC_HD inline int shared_wg_chunks(int nbx, int H, int K, long b, int &i, int &bx, int n2 = 0, int n1 = 0)
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
ADC_HD inline int shared_run_len(int nbx, int bx, int left)
{
    const int n = nbx - bx < SH_RUN ? nbx - bx : SH_RUN;
    return n < left ? n : left;
}
ADC_HD inline void shared_run_flush_range(int S, int E, int D, int pubhi, int &lo, int &hi)
{
    lo = S - D + 1 < 3 ? 3 : S - D + 1; hi = E > pubhi ? pubhi : E;
}
// The whole diagonal j' .. j'+D-1 of right column c lies in the run's left columns [S, E] and in the identity set: the
// ring holds its final key, written straight to the map.  Otherwise the key is partial and merged through the handle's
// key map: with the other runs' keys, and past the identity set with the edge hypotheses (never complete).
ADC_HD inline bool shared_complete(int c, int S, int E, int D) { return c >= S && c + D - 1 <= E; }
ADC_HD inline bool shared_complete(int c, int S, int E, int D, int idhi) { return c <= idhi && shared_complete(c, S, E, D); }
// Edge hypotheses of right column c, evaluated by the edge items: d in [lo, hi] (columns 0..2: every d that can win).
ADC_HD inline void shared_edge_range(int c, int W, int D, int &lo, int &hi)
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
ADC_HD inline int shared_conv_items(int H, int W) { return (int)(((long)H * W + SH_CONV_PX - 1) / SH_CONV_PX); }
ADC_HD inline int shared_edge_cols(int W, int D) { return W - 1 - shared_id_hi(W, D); }   // idhi+1 .. W-1
ADC_HD inline int shared_edge_col_items(int H, int W, int D)
{
    return (int)(((long)H * shared_edge_cols(W, D) + SH_EDGE_PX - 1) / SH_EDGE_PX);
}
ADC_HD inline int shared_edge_items(int H, int W, int D)
{
    return shared_edge_col_items(H, W, D) + (3 * H + SH_EDGE0_PX - 1) / SH_EDGE0_PX;
}
constexpr int AUX_PREP = 0, AUX_CONV = 1, AUX_EDGE = 2, AUX_NONE = 3;
ADC_HD inline int shared_aux_decode(int b, int nprep, int nconv, int nedge, int &item)
{
    item = b;
    if (item < nprep) return AUX_PREP;
    item -= nprep;
    if (item < nconv) return AUX_CONV;
    item -= nconv;
    return item < nedge ? AUX_EDGE : AUX_NONE;
}
// Pixel arithmetic of the items, step `it` of thread `tid` (wave `wv`): false past the end of the item's set.
ADC_HD inline bool shared_conv_px(int item, int it, int tid, long N, long &p)    // the keys p and p + 1
{
    p = (long)item * SH_CONV_PX + 2 * ((long)it * 256 + tid);
    return p < N;
}
ADC_HD inline bool shared_edge_px(int item, int it, int tid, int H, int W, int D, int &i, int &c)
{
    const int nc = shared_edge_cols(W, D);
    const long q = (long)item * SH_EDGE_PX + (long)it * 256 + tid;
    if (q >= (long)H * nc) return false;
    i = (int)(q / nc);
    c = shared_id_hi(W, D) + 1 + (int)(q - (long)i * nc);
    return true;
}
ADC_HD inline bool shared_edge0_px(int item, int it, int wv, int H, int &i, int &c)
{
    const int w = item * SH_EDGE0_PX + it * 4 + wv;
    if (w >= 3 * H) return false;
    i = w / 3; c = w - 3 * i;
    return true;
}
constexpr int RANK_N = 256 * 64;

// Workgroup -> 64-pixel chunk.  The chunks of a launch form one linear space (view, row, chunk-in-row)
// and workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md), so XCD x takes the x-th contiguous eighth of
// that space: every XCD then streams its own region of the volumes instead of every eighth 48 KB piece
// of the same region.  A store-only kernel with this mapping writes 10 % faster (6.9 vs 6.25 TB/s,
// same box) than with chunks in dispatch order.  The grid is 1-D, padded to a multiple of 8.
// chunk_decode is the general form: workgroup b takes the K consecutive chunks (b >> 3) * K + t, t = 0 .. K-1, of its
// XCD's eighth (the maps-only kernel, which fills a 32 KB table once per workgroup); K = 1 is chunk_of_block.
// maps_groups() is the number of workgroups that covers a launch.  With a tapered tail (n2, n1: maps_span) the
// workgroup's chunks are the span's, still consecutive; chunk_at is the decode of one of them.
ADC_HD inline bool chunk_at(int nbx, int H, int nviews, long b, long cl, int &view, int &i, int &bx)
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
ADC_HD inline bool chunk_decode(int nbx, int H, int nviews, int K, long b, int t, int &view, int &i, int &bx,
                                             int n2 = 0, int n1 = 0)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    long first;
    if (t >= maps_span(per, K, n2, n1, b >> 3, first)) return false;
    return chunk_at(nbx, H, nviews, b, first + t, view, i, bx);
}
ADC_HD inline int maps_groups(int nbx, int H, int nviews, int K, int n2 = 0, int n1 = 0)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    return (int)(8 * maps_span_groups(per, K, n2, n1));
}
// cost groups in front of the first tapered one (fused_grid's body), 0 without a taper
ADC_HD inline int maps_body_groups(int nbx, int H, int nviews, int K, int n2, int n1)
{
    const long per = ((long)nbx * H * nviews + 7) >> 3;
    (void)maps_span_tails(per, K, n2, n1);
    return n2 + n1 > 0 ? (int)maps_span_body(per, K, n2, n1) : 0;
}

struct FusedGrid { int cgroups, pgroups, every, slots, groups; };
// With a tapered tail (cbody > 0: the cost groups in front of the first tapered one, maps_body_groups) the table groups
// are spread through the body alone, one after every cbody / pgroups cost groups and none in further slots: a table
// tile lasts about as long as a 4-chunk cost workgroup and would undo the taper from inside the tail.  A body with
// fewer groups than there are table groups keeps the placement below.
ADC_HD inline FusedGrid fused_grid(int ncost, int nprep, int cbody = 0)
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
ADC_HD inline bool fused_decode(const FusedGrid &f, int g, int &idx)
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

}  // namespace

// Chains of the chained batch schedule (chain_plan).  Three at the most: a process has four hardware queues here and
// the caller's stream is one of them.
constexpr int SMT_MAX_CHAINS = 3;
constexpr int SMT_CHAINS_DEFAULT = 2;
// The chained schedule is the default of smt_adcensus_compute_batch wherever the fused one would be (batch_schedule).
constexpr bool SMT_CHAINED_DEFAULT = true;
// Table set and key map that chain c's pair number n (the chain's own counter) uses: TS[] / skeys[] index.
static inline int chain_slot(int c, long n) { return 2 * c + (int)(n & 1); }

// fusion tables, the reference's own float expression (AD-Census.h:287-288)
static inline void build_lut(float sigmaC, float sigmaS, float *lut)
{
    for (int k = 0; k < 256; k++) lut[k] = 1.0f - expf(-((float)k / sigmaC));
    for (int k = 0; k < 64; k++) lut[256 + k] = 1.0f - expf(-((float)k / sigmaS));
}

// Rank table of the maps-only kernel: rank[64*ad + hd] = dense rank of the f32 sum lut[ad] + lut[256 + hd] (the one
// IEEE round-to-nearest add the kernels perform) among all 256 x 64 sums.  sigmaC, sigmaS > 0, so every sum is finite
// and >= +0 and the order of the bit patterns as uint32 is the order of the costs: equal bits get an equal rank,
// larger bits a larger one.  At most 16384 ranks, so rank << 16 | d is a WTA key for d < 65536.
static inline bool build_rank(const float *lut, uint16_t *rank)
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

// Table workgroups of one pair: the tiles and the workgroups of the 13 border columns (16 rows each).
static inline int prep_items(int H, int W, int &ptx)
{
    ptx = (W + PTW - 1) / PTW;
    const int pty = (H + PTH - 1) / PTH, eb = (H + PNT / 16 - 1) / (PNT / 16);
    return ptx * (pty + (eb + ptx - 1) / ptx);
}
// Cost workgroups of a launch over `nviews` views, one 64-pixel chunk each: padded to a multiple of 8 (chunk_of_block).
static inline unsigned cost_grid(int nbx, int H, int nviews) { return (unsigned)(((long)nbx * H * nviews + 7) / 8 * 8); }

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
static inline int chain_plan(int n, int nc, const long *count0, int order, unsigned flags, std::vector<ChainOp> &ops)
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

// ---- The environment readers: one per variable, each read at every call (tests set them between calls) ----------------
// SMT_PLACEMENT=0 in the environment turns place_volumes' search off (first allocation is used).
static inline bool placement_off() { const char *env = getenv("SMT_PLACEMENT"); return env && env[0] == '0'; }
// SMT_STORE_MODE=nt / plain in the environment fixes calibrate_store_mode's choice: its first letter, 0 when not set.
static inline char store_mode_env() { const char *env = getenv("SMT_STORE_MODE"); return env ? env[0] : 0; }

// Chunks per workgroup of the maps-only kernel (k_cost_maps2p).  SMT_MAPS_CHUNKS=<1..64> in the environment is a
// tuning hook (read at every call); SMT_MAPS_KERNEL=rank selects the rank-key form in place of the float LUT (A/B,
// at the 4 workgroups per CU its 32 KB table leaves room for, it is the slower one).
static inline int maps_chunks()
{
    const char *env = getenv("SMT_MAPS_CHUNKS");
    const int k = env ? atoi(env) : 0;
    return k >= 1 && k <= 64 ? k : 4;
}
static inline bool maps_kernel_rank() { const char *env = getenv("SMT_MAPS_KERNEL"); return env && env[0] == 'r'; }

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
static inline void maps_taper(int S, long per, int K, int &n2, int &n1)
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
// The shapes the shared form serves: an identity set that is not empty, and D <= 192.  With four hypotheses per lane
// (192 < D <= 256) the lanes' publishes are 32 bytes apart, a 4-way bank conflict, the kernel needs 93 VGPRs and the
// identity set is a smaller part of the row; measured at 1242 x 375 D = 256 it loses 7 % to the two-view kernel
// (DESIGN.md section 4).  SMT_MAPS_SHARED=force in the environment takes it wherever the set is not empty (tests).
static inline bool maps_shared_shape(int W, int D)
{
    const char *env = getenv("SMT_MAPS_SHARED");
    if (shared_id_hi(W, D) < 3 || (env && env[0] == '0' && env[1] == 0)) return false;
    return D <= 192 || (env && env[0] == 'f');
}

// SMT_SHARED_FINISH=apart in the environment (read at every call) converts every shared pair's keys with a launch of
// its own right behind the pair's launch, instead of inside the next pair's: same-process A/Bs and tests.
static inline bool shared_finish_apart()
{
    const char *env = getenv("SMT_SHARED_FINISH");
    return env && strcmp(env, "apart") == 0;
}

// Chains of a chained call: SMT_CHAINS=<1..3> in the environment (read at every call), 2 otherwise.
static inline int chain_count()
{
    const char *env = getenv("SMT_CHAINS");
    return env && env[0] >= '1' && env[0] <= '0' + SMT_MAX_CHAINS && env[1] == 0 ? env[0] - '0' : SMT_CHAINS_DEFAULT;
}
// SMT_CHAIN_ORDER=pairs|ab|ba in the environment (read at every call): test hook, the orders of chain_plan.
static inline int chain_order()
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
static inline int chain_taper()
{
    const char *env = getenv("SMT_CHAIN_TAPER");
    if (!env) return SMT_CHAIN_TAPER_DEFAULT;
    return strcmp(env, "all") == 0 ? CHAIN_TAPER_ALL : strcmp(env, "last") == 0 ? CHAIN_TAPER_LAST :
           strcmp(env, "none") == 0 ? CHAIN_TAPER_NONE : SMT_CHAIN_TAPER_DEFAULT;
}
// SMT_CHAIN_FORK=start in the environment: CHAIN_FORK_START (chain_plan).
static inline bool chain_fork_start() { const char *env = getenv("SMT_CHAIN_FORK"); return env && strcmp(env, "start") == 0; }
// SMT_OVERLAP in the environment, tuning hook: 0 / 1 / 2 / 3 forces batch_schedule's choice; -1: not set to one of them.
static inline int overlap_env()
{
    const char *env = getenv("SMT_OVERLAP");
    return env && env[0] >= '0' && env[0] <= '3' && env[1] == 0 ? env[0] - '0' : -1;
}
// SMT_BATCH_VOLUMES in the environment (smt_adcensus_compute_batch): 'l' for `last`, 'a' for `all`, 0 for neither.
static inline char batch_volumes_env()
{
    const char *env = getenv("SMT_BATCH_VOLUMES");
    return !env ? 0 : strcmp(env, "all") == 0 ? 'a' : strcmp(env, "last") == 0 ? 'l' : 0;
}
