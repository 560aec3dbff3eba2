// The host-only selftests of the AD-Census family (include/smt.h): the rules of adcensus_rules.h walked the way kernels
// and launchers use them.  No HIP: also `g++ -x c++` with tools/adcensus_selftest_main.cpp, as a sanitizer program.
#include "adcensus_rules.h"

#define SMT_API extern "C" __attribute__((visibility("default")))

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

// Host-side check of the rank table (build_rank) against the float sums it stands for: for sigmaC, sigmaS > 0, every
// sum lut[ad] + lut[256 + hd] is finite and >= +0, ranks are dense from 0, and for any two entries rank order equals
// float order (equal ranks exactly when the bit patterns are equal).  Needs no GPU.
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
