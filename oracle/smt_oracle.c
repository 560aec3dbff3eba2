/*
 * smt_oracle.c -- CPU restatement of the reference's per-pixel x per-disparity hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the shipped product path
 * (stereo_match_traditional_amd/, include/, the C-ABI library) may import, link or call
 * this file; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do, and
 * there only as the checker / the timed CPU baseline.
 *
 * PARITY STATUS
 *   - orc_crossagg_* (CBLSM/cross_aggregator.cpp) is PINNED: it is checked bit-for-bit
 *     against the unmodified reference source compiled into oracle/_ref/ (see
 *     oracle/Makefile) and against tests/golden/ fixtures generated from it.
 *   - The AD-CensusV1 stages (orc_ad_*, orc_census_*, orc_fuse, orc_adcensus_view, orc_wta, orc_arms_*,
 *     orc_aggregate_rect orders 0 and 2, orc_scan_*, orc_scanline, orc_lrcheck, orc_lrcheck_variant,
 *     orc_fill_the_hole, orc_remove_speckles, orc_median) and the live CBLSM.h functions (orc_arms_dir without the
 *     stride bug = ArmLength{L,R,Up,Down}, orc_cblsm_ad, orc_aggregate_rect order 1 = costAggregationV5, orc_wta =
 *     ComputeDispOringin, orc_choose_arm_length) are PINNED: AD-CensusV1/{AD-Census.h, CrossArm.cpp,
 *     ScanlineOptimizer.h, PostProcessing.h} and CBLSM/CBLSM.h use cv::Mat only as a pixel container and compile
 *     unmodified against oracle/ref_build/shim/opencv2/opencv.hpp (container only; every OpenCV operation with
 *     arithmetic in it aborts) into oracle/_ref/libadcensus_ref.so and libcblsm_ref.so.  tests/test_ref_pin_cpu.py
 *     checks this file against those builds bit for bit and against tests/golden/ref_pin_hashes.json.
 *   - Still "PARITY UNPINNED": orc_sad*, orc_ncc, orc_asw*, orc_cblsm_cost_aggregation_new (costAggregationNew /
 *     ComputeLocalValue) and orc_bgr2gray.  Their results come out of OpenCV's MatExpr, cv::sum, cv::mean and
 *     cvtColor (OpenCV 3.1.0, AD-CensusV1/AD-CensusV1.vcxproj:135, not in this image), which a container header
 *     must not imitate, and the reference ships no tests, golden vectors or sample outputs.  Those functions are
 *     restated loop-for-loop from the reference text (file:line cited at each function) and cross-checked against
 *     an independently derived closed form (tests/test_cpu_oracle.py).
 *
 * All citations are relative to /root/reference.  Layout conventions follow the
 * reference: images [H][W] row-major, volumes [H][W][D] with d fastest
 * (AD-Census.h:87).  The loops deliberately keep the reference's algorithmic
 * complexity (e.g. the 9x7 census is rebuilt for every (i,j,d)) because this file is
 * also what bench.py times as the CPU baseline ("port").
 *
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off, no -ffast-math).  The same file built with
 * -fopenmp (libsmt_oracle_omp.so) parallelises the AD-Census stage over rows for the all-core CPU
 * baseline; the default build ignores the pragmas (the reference's AD-CensusV1 has no OpenMP).
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORC_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------
 * Synthetic stereo pair generator.  Integer-only, platform independent.
 * ---------------------------------------------------------------------------------- */
static int orc_tri(int x, int p)
{
    /* integer triangle wave in [-p/2, p/2] with period 2p */
    int m = x % (2 * p);
    int v = m < p ? m : 2 * p - m;
    return v - p / 2;
}

ORC_API void orc_synth_pair(int H, int W, int D, uint32_t seed, int noise,
                            uint8_t *L, uint8_t *R)
{
    uint32_t s = seed;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            s = s * 1664525u + 1013904223u;
            int byte = (int)(s >> 24);
            int v;
            if (noise)
                v = byte;
            else
                v = 128 + orc_tri(j, 203) * 70 / 101 + orc_tri(i, 139) * 40 / 69
                    + 25 * (((j / 40) + (i / 30)) & 1) + (byte % 6);
            if (v < 0) v = 0;
            if (v > 255) v = 255;
            R[i * W + j] = (uint8_t)v;
        }
    for (int i = 0; i < H; i++) {
        int g = D / 8 + ((i / 8) % 7) * (D / 16);
        for (int j = 0; j < W; j++) {
            s = s * 1664525u + 1013904223u;
            int byte = (int)(s >> 24);
            L[i * W + j] = (j >= g) ? R[i * W + j - g] : (uint8_t)byte;
        }
    }
}

/* ------------------------------------------------------------------------------------
 * a2  AD_Census::ComputeAD / ComputeADRight            AD-Census.h:75-101, 103-129
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_ad_left(const float *L, const float *R, int H, int W, int D, float *out)
{
#pragma omp parallel for schedule(static)
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            float lv = L[i * W + j];
            float *c = out + ((size_t)i * W + j) * D;
            for (int d = 0; d < D; d++) {
                if (j - d < 0) c[d] = c[d - 1];               /* :88-92 copy previous */
                else c[d] = fabsf(lv - R[i * W + j - d]);     /* :95-96 */
            }
        }
}

ORC_API void orc_ad_right(const float *L, const float *R, int H, int W, int D, float *out)
{
#pragma omp parallel for schedule(static)
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            float rv = R[i * W + j];
            float *c = out + ((size_t)i * W + j) * D;
            for (int d = 0; d < D; d++) {
                if (j + d >= W) c[d] = c[d - 1];              /* :116-120 */
                else c[d] = fabsf(L[i * W + j + d] - rv);     /* :123-124 */
            }
        }
}

/* ------------------------------------------------------------------------------------
 * a3  AD_Census::ComputeCensus9x7 / ...Right           AD-Census.h:142-204, 207-269
 *     63-bit strings rebuilt for every (i,j,d); Kernighan popcount.
 *     Row range [i0,i1) lets bench.py time a bounded band; the window still looks at
 *     rows outside the band (validity is tested against the full image).
 * ---------------------------------------------------------------------------------- */
static int orc_popcount64_loop(uint64_t x)
{
    int n = 0;
    while (x) { n++; x &= x - 1; }                           /* :194-198 */
    return n;
}

ORC_API void orc_census_left(const float *L, const float *R, int H, int W, int D,
                             int i0, int i1, float *out)
{
#pragma omp parallel for schedule(static)      /* only in libsmt_oracle_omp.so (all-core baseline) */
    for (int i = i0; i < i1; i++)
        for (int j = 0; j < W; j++) {
            float lc = L[i * W + j];
            float *c = out + ((size_t)i * W + j) * D;
            for (int d = 0; d < D; d++) {
                uint64_t lb = 0, rb = 0;
                float rc = (j - d < 0) ? R[i * W + 0] : R[i * W + j - d];   /* :159-164 */
                for (int r = -4; r <= 4; r++)
                    for (int k = -3; k <= 3; k++) {
                        lb <<= 1; rb <<= 1;
                        if (i + r < 0 || i + r >= H || j + k < 0 || j + k >= W)
                            continue;                                        /* :173-174 */
                        float lv = L[(i + r) * W + j + k];
                        float rv = (j + k - d < 0) ? R[(i + r) * W + 0]
                                                   : R[(i + r) * W + j + k - d]; /* :177-182 */
                        if (lc > lv) lb += 1;
                        if (rc > rv) rb += 1;
                    }
                c[d] = (float)orc_popcount64_loop(lb ^ rb);
            }
        }
}

ORC_API void orc_census_right(const float *L, const float *R, int H, int W, int D,
                              int i0, int i1, float *out)
{
#pragma omp parallel for schedule(static)
    for (int i = i0; i < i1; i++)
        for (int j = 0; j < W; j++) {
            float rc = R[i * W + j];
            float *c = out + ((size_t)i * W + j) * D;
            for (int d = 0; d < D; d++) {
                uint64_t lb = 0, rb = 0;
                float lc = (j + d >= W) ? L[i * W + W - 1] : L[i * W + j + d]; /* :224-229 */
                for (int r = -4; r <= 4; r++)
                    for (int k = -3; k <= 3; k++) {
                        lb <<= 1; rb <<= 1;
                        if (i + r < 0 || i + r >= H || j + k < 0 || j + k >= W)
                            continue;                                        /* :238-239 */
                        float rv = R[(i + r) * W + j + k];
                        float lv = (j + k + d >= W) ? L[(i + r) * W + 0]     /* :242-243 col 0 (sic) */
                                                    : L[(i + r) * W + j + k + d];
                        if (lc > lv) lb += 1;
                        if (rc > rv) rb += 1;
                    }
                c[d] = (float)orc_popcount64_loop(lb ^ rb);
            }
        }
}

/* ------------------------------------------------------------------------------------
 * a5  AD_Census::ComputeADcensus / ...Right            AD-Census.h:271-294, 296-318
 *     cost = (1 - exp(-(AD/sigmaC))) + (1 - exp(-(census/sigmaS))), all float.
 *     In the reference `exp` on a float argument resolves to the float overload.
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_fuse(const float *ad, const float *census, size_t n, float sigmaC,
                      float sigmaS, float *cost)
{
#pragma omp parallel for schedule(static)
    for (size_t k = 0; k < n; k++) {
        float a = 1.0f - expf(-(ad[k] / sigmaC));
        float c = 1.0f - expf(-(census[k] / sigmaS));
        cost[k] = a + c;
    }
}

/* The two 1-D tables the fusion reduces to for integer-valued images (AD in 0..255,
 * census in 0..63).  Same expression as orc_fuse. */
ORC_API void orc_fuse_luts(float sigmaC, float sigmaS, float *lutA256, float *lutC64)
{
    for (int k = 0; k < 256; k++) lutA256[k] = 1.0f - expf(-((float)k / sigmaC));
    for (int k = 0; k < 64; k++) lutC64[k] = 1.0f - expf(-((float)k / sigmaS));
}

/* Whole a2+a3+a5 stage for one view over a row band, volume written in place at the
 * band's rows.  view: 0 = left (ComputeADcensus), 1 = right (ComputeADcensusRight).
 * ad/census scratch volumes are band-sized to keep memory bounded. */
ORC_API int orc_adcensus_view(const float *L, const float *R, int H, int W, int D,
                              float sigmaC, float sigmaS, int view, int i0, int i1,
                              float *cost)
{
    size_t band = (size_t)(i1 - i0) * W * D;
    float *ad = (float *)calloc(band ? band : 1, sizeof(float));
    float *ce = (float *)calloc(band ? band : 1, sizeof(float));
    if (!ad || !ce) { free(ad); free(ce); return -1; }
    /* AD only needs the band's own rows; run it on a row-offset view. */
    const float *Lb = L + (size_t)i0 * W, *Rb = R + (size_t)i0 * W;
    if (view == 0) orc_ad_left(Lb, Rb, i1 - i0, W, D, ad);
    else orc_ad_right(Lb, Rb, i1 - i0, W, D, ad);
    /* census writes at absolute row offsets -> pass a pointer shifted back by i0 rows */
    float *ce_abs = ce - (size_t)i0 * W * D;
    if (view == 0) orc_census_left(L, R, H, W, D, i0, i1, ce_abs);
    else orc_census_right(L, R, H, W, D, i0, i1, ce_abs);
    orc_fuse(ad, ce, band, sigmaC, sigmaS, cost + (size_t)i0 * W * D);
    free(ad); free(ce);
    return 0;
}

/* ------------------------------------------------------------------------------------
 * a6/a11  WTA: first strict minimum over d.  AD-Census.h:346-380, CrossArm.cpp:33-57,
 *         ScanlineOptimizer.h:40-64, CBLSM.h:383-407 (same rule).
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_wta(const float *vol, int H, int W, int D, float *disp)
{
#pragma omp parallel for schedule(static)
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const float *c = vol + ((size_t)i * W + j) * D;
            float best = c[0], bd = 0;
            for (int d = 1; d < D; d++)
                if (best > c[d]) { bd = (float)d; best = c[d]; }
            disp[i * W + j] = bd;
        }
}

/* ------------------------------------------------------------------------------------
 * a9/a19  Arm lengths.  CrossArm.cpp:147-598 (gray + 3-channel branches),
 *         CBLSM.h:536-966.  One routine, four directions:
 *           dir 0 = left, 1 = right, 2 = top, 3 = bottom.
 *   *tau is the sticky threshold state: the reference's member `_tao`
 *   (CrossArm.h:34) lives across pixels AND across the four calls; CBLSM passes `tao`
 *   by value so it is sticky within one call only -- the caller decides by passing the
 *   same or a fresh *tau.
 *   sec/maxlen = 17/34 hard-coded in CrossArm.cpp:168-172, parameters in CBLSM.h.
 *   right_row_bug: ComputeRightArmLength iterates j < row, tests j+off < row and stores
 *   with stride row (CrossArm.cpp:265, 320, 368); image reads still use the true width.
 * ---------------------------------------------------------------------------------- */
static int orc_pixdiff(const uint8_t *img, int ch, size_t a, size_t b)
{
    int m = 0;
    for (int c = 0; c < ch; c++) {
        int v = abs((int)img[a * ch + c] - (int)img[b * ch + c]);
        if (v > m) m = v;
    }
    return m;
}

ORC_API void orc_arms_dir(const uint8_t *img, int H, int W, int ch, int dir, int *tau,
                          int tau_low, int sec, int maxlen, int right_row_bug, int *out)
{
    int colR = (dir == 1 && right_row_bug) ? H : W;   /* loop bound / store stride */
    for (int i = 0; i < H; i++)
        for (int j = 0; j < colR; j++) {
            int saved = 0, off = 0;
            for (;;) {
                /* `while (j - offset >= 0)` etc. is always true on entry: the body
                 * breaks as soon as the next neighbour is outside (CrossArm.cpp:219). */
                saved = off;
                off++;
                if (off > sec) {                         /* :223-228 flip BEFORE bounds */
                    *tau = tau_low;
                    if (off > maxlen) break;
                }
                int ni = i, nj = j, inside, far_from_border;
                switch (dir) {
                case 0: nj = j - off; inside = nj >= 0;    far_from_border = (j - 1 >= 1); break;
                case 1: nj = j + off; inside = nj < colR;  far_from_border = (j + 1 < colR - 1); break;
                case 2: ni = i - off; inside = ni >= 0;    far_from_border = (i - 1 >= 1); break;
                default: ni = i + off; inside = ni < H;    far_from_border = (i + 1 < H - 1); break;
                }
                if (!inside) break;                      /* :249-253 */
                int diff = orc_pixdiff(img, ch, (size_t)i * W + j, (size_t)ni * W + nj);
                if (diff > *tau) {                       /* :234-247 */
                    if (far_from_border && saved < 1) saved = 1;
                    break;
                }
            }
            out[(size_t)i * colR + j] = saved;           /* :255 / :368 (stride bug) */
        }
}

/* a8+a9: CrossArmAggregation::Initialize + the four Compute*ArmLength calls in the
 * order main.cpp:68-72 makes them.  chain=1: one tau for all four (CrossArm.cpp member
 * `_tao`); chain=0: fresh tau per direction (CBLSM.cpp:64-67, by-value uchar).
 * Outputs are zero-initialised like `new int[col*row]()` (CrossArm.cpp:14-17). */
ORC_API int orc_arms_all(const uint8_t *img, int H, int W, int ch, int tau0, int tau_low,
                         int sec, int maxlen, int chain, int right_row_bug,
                         int *armL, int *armR, int *armT, int *armB)
{
    size_t n = (size_t)H * W;
    if (right_row_bug && H > W) return -1;   /* reference reads outside the image: UB */
    memset(armL, 0, n * sizeof(int)); memset(armR, 0, n * sizeof(int));
    memset(armT, 0, n * sizeof(int)); memset(armB, 0, n * sizeof(int));
    int tau = tau0;
    orc_arms_dir(img, H, W, ch, 0, &tau, tau_low, sec, maxlen, 0, armL);
    if (!chain) tau = tau0;
    orc_arms_dir(img, H, W, ch, 1, &tau, tau_low, sec, maxlen, right_row_bug, armR);
    if (!chain) tau = tau0;
    orc_arms_dir(img, H, W, ch, 2, &tau, tau_low, sec, maxlen, 0, armT);
    if (!chain) tau = tau0;
    orc_arms_dir(img, H, W, ch, 3, &tau, tau_low, sec, maxlen, 0, armB);
    return 0;
}

/* ------------------------------------------------------------------------------------
 * a10/a19  Rectangle-mean aggregation.
 *   order 0: CrossArmAggregation::AggregationVertical CrossArm.cpp:60-102
 *            (columns outer, rows inner);
 *   order 1: costAggregationV5 CBLSM.h:1179-1224 (rows outer, columns inner).
 *   Flat indexing `(i+top)*col + j + left` wraps across row ends exactly as the
 *   reference does.  Reads past the end of the plane are undefined behaviour in the
 *   reference; they are counted in the return value and read as 0.0f here (tests use
 *   sizes where the count is 0).
 * ---------------------------------------------------------------------------------- */
ORC_API long orc_aggregate_rect(const float *vol, int H, int W, int D, const int *armL,
                                const int *armR, const int *armT, const int *armB,
                                int order, float *out)
{
    size_t n = (size_t)H * W;
    long oob = 0;
    /* the d-planes are independent (:66 loops over them); the OpenMP build (fixture generator
     * only) hands them to threads, each with its own plane buffer */
#pragma omp parallel reduction(+ : oob)
    {
    float *plane = (float *)malloc(n * sizeof(float));
#pragma omp for schedule(dynamic, 1)
    for (int d = 0; d < D; d++) {
        for (size_t p = 0; p < n; p++) plane[p] = vol[p * D + d];     /* :68-75 */
        for (int i = 0; i < H; i++)
            for (int j = 0; j < W; j++) {
                int Ll = armL[i * W + j], Rr = armR[i * W + j];
                int up = armT[i * W + j], dn = armB[i * W + j];
                float v = 0; int cnt = 0;
                if (order == 0) {
                    for (int l = -Ll; l <= Rr; l++)
                        for (int t = -up; t <= dn; t++) {
                            long idx = (long)(i + t) * W + j + l;
                            float x = 0.0f;
                            if (idx < 0 || idx >= (long)n) oob++; else x = plane[idx];
                            v = v + x; cnt++;                          /* :92-93 */
                        }
                } else if (order == 1) {
                    for (int t = -up; t <= dn; t++)
                        for (int l = -Ll; l <= Rr; l++) {
                            long idx = (long)(i + t) * W + j + l;
                            float x = 0.0f;
                            if (idx < 0 || idx >= (long)n) oob++; else x = plane[idx];
                            v = v + x; cnt++;                          /* CBLSM.h:1214-1215 */
                        }
                } else {
                    /* order 2: CrossArmAggregation::Aggregation, CrossArm.cpp:104-145 (declared public,
                     * CrossArm.h:19, never called): rows outer, EXCLUSIVE upper bounds (:130-132).  An
                     * empty rectangle divides 0.0f by 0 (:138): NaN under IEEE; counted with the
                     * out-of-plane reads as "reference undefined". */
                    for (int t = -up; t < dn; t++)
                        for (int l = -Ll; l < Rr; l++) {
                            long idx = (long)(i + t) * W + j + l;
                            float x = 0.0f;
                            if (idx < 0 || idx >= (long)n) oob++; else x = plane[idx];
                            v = v + x; cnt++;                          /* :134-135 */
                        }
                    if (cnt == 0) oob++;
                }
                out[((size_t)i * W + j) * D + d] = v / (float)cnt;     /* :96-98 */
            }
    }
    free(plane);
    }
    return oob;
}

/* ------------------------------------------------------------------------------------
 * a13/a14/a15  ScanlineOptimizer                       ScanlineOptimizer.h:104-253
 * ---------------------------------------------------------------------------------- */
static float orc_minf(float a, float b) { return (b < a) ? b : a; }   /* std::min */
static float orc_maxf(float a, float b) { return (a < b) ? b : a; }   /* std::max */

ORC_API void orc_scan_lr(const float *cost, const float *gray, int H, int W, int D,
                         int p1i, int p2i, int is_left, float *agg)
{
    float p1 = (float)p1i, p2Init = (float)p2i;                       /* :132-133 */
    int dir = is_left ? 1 : -1;
#pragma omp parallel
    {
    float *last = (float *)malloc((D + 2) * sizeof(float));
#pragma omp for schedule(static)
    for (int i = 0; i < H; i++) {
        size_t x0 = is_left ? 0 : (size_t)(W - 1);
        const float *ci = cost + ((size_t)i * W + x0) * D;
        float *ai = agg + ((size_t)i * W + x0) * D;
        const float *g = gray + (size_t)i * W + x0;
        float lastgray = *g;
        for (int k = 0; k < D + 2; k++) last[k] = (float)0xffff;      /* :151 */
        memcpy(ai, ci, D * sizeof(float));                            /* :153 */
        memcpy(last + 1, ai, D * sizeof(float));                      /* :155 */
        ci += dir * D; ai += dir * D; g += dir;
        float minLast = (float)0xffff;
        for (int k = 0; k < D + 2; k++) minLast = orc_minf(last[k], minLast); /* :163-166 */
        for (int j = 0; j < W - 1; j++) {
            float minCost = (float)0xffff;
            float gv = *g;
            float p2 = orc_maxf(p1, p2Init / (fabsf(gv - lastgray) + 1)); /* :171 */
            lastgray = gv;                                            /* :172 */
            for (int d = 0; d < D; d++) {
                float c = ci[d];
                float l1 = last[d + 1];
                float l2 = last[d] + p1;
                float l3 = last[d + 2] + p1;
                float l4 = minLast + p2;
                float cs = c + orc_minf(orc_minf(l1, l2), orc_minf(l3, l4)) - minLast; /* :180 */
                ai[d] = cs;
                minCost = orc_minf(minCost, cs);
            }
            minLast = minCost;
            memcpy(last + 1, ai, D * sizeof(float));
            ci += dir * D; ai += dir * D; g += dir;
        }
    }
    free(last);
    }
}

ORC_API void orc_scan_ud(const float *cost, const float *gray, int H, int W, int D,
                         int p1i, int p2i, int is_up, float *agg)
{
    float p1 = (float)p1i, p2Init = (float)p2i;
    int dir = is_up ? 1 : -1;
    ptrdiff_t step = (ptrdiff_t)dir * W * D;
#pragma omp parallel
    {
    float *last = (float *)malloc((D + 2) * sizeof(float));
#pragma omp for schedule(static)
    for (int j = 0; j < W; j++) {
        size_t y0 = is_up ? 0 : (size_t)(H - 1);
        const float *ci = cost + (y0 * W + j) * D;
        float *ai = agg + (y0 * W + j) * D;
        const float *g = gray + y0 * W + j;
        float grayLast = *g;                                          /* :210 never updated */
        for (int k = 0; k < D + 2; k++) last[k] = (float)0xffff;
        memcpy(ai, ci, D * sizeof(float));
        memcpy(last + 1, ai, D * sizeof(float));
        ci += step; ai += step;
        g += dir;                                                     /* :221 +-1 element (sic) */
        float minLast = (float)0xffff;
        for (int k = 0; k < D + 2; k++) minLast = orc_minf(last[k], minLast);
        for (int i = 0; i < H - 1; i++) {
            float gv = *g;
            float p2 = orc_maxf(p1, p2Init / (fabsf(gv - grayLast) + 1)); /* :232 */
            float minCost = (float)0xffff;
            for (int d = 0; d < D; d++) {
                float c = ci[d];
                float l1 = last[d + 1];
                float l2 = last[d + 1] + p1;                          /* :238 d+1 (sic) */
                float l3 = last[d + 2] + p1;
                float l4 = minLast + p2;
                float cs = c + orc_minf(orc_minf(l1, l2), orc_minf(l3, l4)) - minLast;
                ai[d] = cs;
                minCost = orc_minf(minCost, cs);
            }
            minLast = minCost;
            memcpy(last + 1, ai, D * sizeof(float));
            ci += step; ai += step;
            g += dir;                                                 /* :250 */
        }
    }
    free(last);
    }
}

/* ScanLine: four passes then ((left+right)+up)+down.  :104-128 */
ORC_API int orc_scanline(const float *cost, const float *gray, int H, int W, int D,
                         int p1, int p2, float *out)
{
    size_t n = (size_t)H * W * D;
    float *l = (float *)calloc(n, sizeof(float)), *r = (float *)calloc(n, sizeof(float));
    float *u = (float *)calloc(n, sizeof(float)), *dn = (float *)calloc(n, sizeof(float));
    if (!l || !r || !u || !dn) { free(l); free(r); free(u); free(dn); return -1; }
    orc_scan_lr(cost, gray, H, W, D, p1, p2, 1, l);
    orc_scan_lr(cost, gray, H, W, D, p1, p2, 0, r);
    orc_scan_ud(cost, gray, H, W, D, p1, p2, 1, u);
    orc_scan_ud(cost, gray, H, W, D, p1, p2, 0, dn);
    for (size_t k = 0; k < n; k++) out[k] = l[k] + r[k] + u[k] + dn[k];   /* :124 */
    free(l); free(r); free(u); free(dn);
    return 0;
}

/* ------------------------------------------------------------------------------------
 * a17  LeftRightConsistency                            PostProcessing.h:72-135
 *      In place on dL.  cls: 0 = kept, 1 = occlusion, 2 = mismatch (the two reference
 *      vectors are these classes listed in row-major order).
 * ---------------------------------------------------------------------------------- */
/* x86 result of `static_cast<int>(double)` when the value does not fit (undefined in C/C++): cvttsd2si
 * returns INT_MIN. */
static int orc_d2i(double x) { return (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (-2147483647 - 1); }

ORC_API void orc_lrcheck(float *dL, const float *dR, int H, int W, int gate, uint8_t *cls,
                         long *n_occ, long *n_mis)
{
    const float thr = (float)gate;                                    /* :77 */
    long no = 0, nm = 0;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            float *disp = &dL[i * W + j];
            uint8_t c = 0;
            if (*disp == INFINITY) { c = 2; }                          /* :90-93 */
            else {
                int cr = orc_d2i((double)((float)j - *disp) + 0.5);   /* :96 */
                if (cr >= 0 && cr < W) {
                    float dr = dR[i * W + cr];
                    if (fabsf(*disp - dr) > thr) {                     /* :103 */
                        int crl = orc_d2i((double)((float)cr + dr) + 0.5); /* :110 */
                        if (crl > 0 && crl < W) {
                            float dl = dL[i * W + crl];                /* in-place read :112 */
                            c = (dl > *disp) ? 1 : 2;
                        } else c = 2;
                        *disp = INFINITY;                              /* :125 */
                    }
                } else { *disp = INFINITY; c = 2; }                    /* :130-131 */
            }
            cls[i * W + j] = c;
            if (c == 1) no++; else if (c == 2) nm++;
        }
    *n_occ = no; *n_mis = nm;
}

/* LeftAndRightConsistency                                PostProcessing.h:10-70 (no call site)
 *      Out of place: leftDisp is only read, lastDisp written.  cls as orc_lrcheck. */
ORC_API void orc_lrcheck_variant(const float *dL, const float *dR, float *last, int H, int W, float gate,
                                 uint8_t *cls, long *n_occ, long *n_mis)
{
    long no = 0, nm = 0;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            float disp = dL[i * W + j];
            uint8_t c = 0;
            int cr = orc_d2i((double)((float)j - disp) + 0.5);                  /* :24 */
            if (cr >= 0 && cr < W) {
                float dr = dR[i * W + cr];
                if (fabsf(disp - dr) >= gate) {                                /* :32 */
                    int crl = orc_d2i((double)((float)cr + dr) + 0.5);          /* :40 */
                    if (crl > 0 && crl < W) c = (dL[i * W + crl] > disp) ? 1 : 2; /* :41-49 */
                    else c = 2;                                                /* :51-53 */
                    last[i * W + j] = 0;                                       /* :57 */
                } else last[i * W + j] = disp;                                 /* :61 */
            } else { last[i * W + j] = 0; c = 2; }                             /* :64-67 */
            cls[i * W + j] = c;
            if (c == 1) no++; else if (c == 2) nm++;
        }
    *n_occ = no; *n_mis = nm;
}

/* ------------------------------------------------------------------------------------
 * a18  CrossAggregator                                 CBLSM/cross_aggregator.cpp:19-394
 *      PINNED against oracle/_ref (the reference source itself).
 *      arms out: [N][4] = left,right,top,bottom (struct CrossArm, cross_aggregator.h:17)
 * ---------------------------------------------------------------------------------- */
static int orc_coldist(const uint8_t *a, const uint8_t *b)
{
    int d0 = abs((int)a[0] - (int)b[0]), d1 = abs((int)a[1] - (int)b[1]);
    int d2 = abs((int)a[2] - (int)b[2]);
    int m = d0 > d1 ? d0 : d1;
    return m > d2 ? m : d2;                                            /* h:78-80 */
}

static uint8_t orc_ca_arm(const uint8_t *img, int W, int H, int x, int y, int dx, int dy,
                          int L1, int L2, int t1, int t2)
{
    const uint8_t *c0 = img + ((size_t)y * W + x) * 3;
    const uint8_t *prev = c0;
    int lim = L1 < 255 ? L1 : 255;                                     /* :151 MAX_ARM_LENGTH */
    int xn = x + dx, yn = y + dy;
    uint8_t len = 0;
    for (int n = 0; n < lim; n++) {
        if (xn < 0 || xn == W || yn < 0 || yn == H) break;             /* :154-163 */
        const uint8_t *c = img + ((size_t)yn * W + xn) * 3;
        int d1 = orc_coldist(c, c0);
        if (d1 >= t1) break;                                           /* :169-172 */
        if (n > 0 && orc_coldist(c, prev) >= t1) break;                /* :175-180 */
        if (n + 1 > L2 && d1 >= t2) break;                             /* :183-187 */
        len++;
        prev = c; xn += dx; yn += dy;
    }
    return len;
}

ORC_API void orc_crossagg_arms(const uint8_t *bgr, int W, int H, int L1, int L2, int t1,
                               int t2, uint8_t *arms)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            uint8_t *a = arms + ((size_t)y * W + x) * 4;
            a[0] = orc_ca_arm(bgr, W, H, x, y, -1, 0, L1, L2, t1, t2);
            a[1] = orc_ca_arm(bgr, W, H, x, y, +1, 0, L1, L2, t1, t2);
            a[2] = orc_ca_arm(bgr, W, H, x, y, 0, -1, L1, L2, t1, t2);
            a[3] = orc_ca_arm(bgr, W, H, x, y, 0, +1, L1, L2, t1, t2);
        }
}

/* Initialize + SetData + SetParams + Aggregate(iters) + get_cost_ptr.  :19-133 */
ORC_API int orc_crossagg(const uint8_t *bgr, const float *cost_init, int W, int H, int D,
                         int L1, int L2, int t1, int t2, int iters, uint8_t *arms_out,
                         float *cost_out)
{
    size_t n = (size_t)W * H;
    if ((long)n <= 0 || D <= 0) return 1;                              /* :28-31 */
    uint8_t *arms = arms_out;
    uint16_t *cnt[2], *ctmp;
    float *t0 = (float *)malloc(n * sizeof(float)), *t1v = (float *)malloc(n * sizeof(float));
    cnt[0] = (uint16_t *)malloc(n * 2); cnt[1] = (uint16_t *)malloc(n * 2);
    ctmp = (uint16_t *)malloc(n * 2);
    orc_crossagg_arms(bgr, W, H, L1, L2, t1, t2, arms);
    /* ComputeSupPixelCount :271-325 */
    for (int hf = 1; hf >= 0; hf--) {
        int id = hf ? 0 : 1;
        for (int k = 0; k < 2; k++)
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    const uint8_t *a = arms + ((size_t)y * W + x) * 4;
                    int count = 0;
                    int horizontal = (hf && k == 0) || (!hf && k == 1);
                    if (k == 0) {
                        if (horizontal) for (int t = -a[0]; t <= a[1]; t++) count++;
                        else for (int t = -a[2]; t <= a[3]; t++) count++;
                        ctmp[y * W + x] = (uint16_t)count;
                    } else {
                        if (horizontal) for (int t = -a[0]; t <= a[1]; t++) count += ctmp[y * W + x + t];
                        else for (int t = -a[2]; t <= a[3]; t++) count += ctmp[(y + t) * W + x];
                        cnt[id][y * W + x] = (uint16_t)count;
                    }
                }
    }
    memcpy(cost_out, cost_init, n * D * sizeof(float));                 /* :108 */
    int hf = 1;
    for (int it = 0; it < iters; it++) {
        for (int d = 0; d < D; d++) {                                   /* AggregateInArms :327-394 */
            for (size_t p = 0; p < n; p++) t0[p] = cost_out[p * D + d];
            int id = hf ? 0 : 1;
            for (int k = 0; k < 2; k++)
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++) {
                        const uint8_t *a = arms + ((size_t)y * W + x) * 4;
                        const float *src = k == 0 ? t0 : t1v;
                        int horizontal = (hf && k == 0) || (!hf && k == 1);
                        float c = 0.0f;
                        if (horizontal) for (int t = -a[0]; t <= a[1]; t++) c += src[y * W + x + t];
                        else for (int t = -a[2]; t <= a[3]; t++) c += src[(y + t) * W + x];
                        if (k == 0) t1v[y * W + x] = c;
                        else cost_out[((size_t)y * W + x) * D + d] = c / (float)cnt[id][y * W + x];
                    }
        }
        hf = !hf;
    }
    free(t0); free(t1v); free(cnt[0]); free(cnt[1]); free(ctmp);
    return 0;
}

/* ------------------------------------------------------------------------------------
 * a19  CBLSM ComputeAD / ComputeADRight on uchar        CBLSM.h:327-381
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_cblsm_ad(const uint8_t *L, const uint8_t *R, int H, int W, int D, int view,
                          float *out)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            float *c = out + ((size_t)i * W + j) * D;
            for (int d = 0; d < D; d++) {
                if (view == 0) {
                    if (j - d < 0) c[d] = c[d - 1];
                    else c[d] = (float)abs((int)L[i * W + j] - (int)R[i * W + j - d]);
                } else {
                    if (j + d >= W) c[d] = c[d - 1];
                    else c[d] = (float)abs((int)L[i * W + j + d] - (int)R[i * W + j]);
                }
            }
        }
}

/* ------------------------------------------------------------------------------------
 * a20/a21  SAD                                          SAD/Sad.h:15-182
 *   Lp/Rp are the replicate-padded images (pad = winsize+1, SADmain.cpp:47-48),
 *   Hp = H + 2*(winsize+1), Wp likewise.  `cv::abs(a-b)` on 8U Mats is an absdiff in
 *   OpenCV 3.1.0 (MatOp_AddEx::abs), `cv::sum` an exact integer sum.
 * ---------------------------------------------------------------------------------- */
static float orc_sadvalue(const uint8_t *a, const uint8_t *b, int Wp, int side)
{
    int s = 0;
    for (int r = 0; r < side; r++)
        for (int c = 0; c < side; c++) s += abs((int)a[r * Wp + c] - (int)b[r * Wp + c]);
    return (float)s;                                                   /* :17-19 */
}

static float orc_optimal_disparity(const float *sad, int D)            /* :40-85 */
{
    float minv = (float)0xffff, best = (float)0xffff, sec = sad[0];
    for (int i = 1; i < D; i++)
        if (minv > sad[i]) { minv = sad[i]; best = (float)i; }
    for (int i = 0; i < D; i++) {
        if (minv == sad[i]) continue;
        sec = orc_minf(sec, sad[i]);
    }
    if ((double)(sec - minv) <= 0.01) return 0;                        /* :66 */
    if (best == 0 || best == (float)(D - 1)) return 0;                 /* :71 */
    return best;                                                       /* :84 (sub-pixel value discarded) */
}

ORC_API void orc_sad(const uint8_t *Lp, const uint8_t *Rp, int Hp, int Wp, int D,
                     int winsize, int view, int32_t *disp /* [Hp-2w][Wp-2w], pre-zeroed by caller */)
{
    int w = winsize + 1, side = 2 * w + 1;
    int W = Wp - 2 * w;
    float *sad = (float *)malloc(D * sizeof(float));
    if (view == 0) {                                                   /* GetPointDepthLeft :96-139 */
        for (int i = w; i < Hp - w; i++)
            for (int j = w; j < Wp - w; j++) {
                const uint8_t *lw = Lp + (i - w) * Wp + (j - w);
                for (int d = 0; d < D; d++) {
                    if (j - w - d < 0) { sad[d] = sad[d - 1]; continue; }   /* :125-129 */
                    sad[d] = orc_sadvalue(lw, Rp + (i - w) * Wp + (j - w - d), Wp, side);
                }
                disp[(i - w) * W + (j - w)] = (int32_t)orc_optimal_disparity(sad, D);
            }
    } else {                                                           /* GetPointDepthRight :141-182 */
        for (int i = w; i < Hp - w - 1; i++)
            for (int j = w; j < Wp - w - 1; j++) {
                const uint8_t *rw = Rp + (i - w) * Wp + (j - w);
                for (int d = 0; d < D; d++) {
                    if (j + d + w + 1 > Wp) { sad[d] = sad[d - 1]; continue; } /* :167-171 */
                    sad[d] = orc_sadvalue(Lp + (i - w) * Wp + (j - w + d), rw, Wp, side);
                }
                float ms = sad[0]; int idx = 0;                        /* GetMinSadIndex :22-38 */
                for (int k = 1; k < D; k++) if (sad[k] < ms) { ms = sad[k]; idx = k; }
                disp[(i - w) * W + (j - w)] = idx;
            }
    }
    free(sad);
}

/* a22  CrossCheckDiaparity (SAD, int maps)               Sad.h:184-222
 *      Invalid = (int)infinity, undefined in C++; x86 cvttss2si yields INT_MIN, which is
 *      what is written here.  cls: 0 kept, 1 occlusion, 2 mismatch. */
ORC_API void orc_sad_crosscheck(const int32_t *dL, const int32_t *dR, int H, int W,
                                int32_t *out, uint8_t *cls)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            int lv = dL[i * W + j];
            long idx = (long)i * W + j - lv;                           /* :204 flat pointer arithmetic */
            int rv = (idx >= 0 && idx < (long)H * W) ? dR[idx] : 0;
            /* abs(lv - rv) as x86 computes it (signed overflow is undefined in C): the subtraction wraps, and the
             * negation of INT_MIN is INT_MIN, which is not above the threshold */
            int sub = (int)((unsigned)lv - (unsigned)rv);
            int diff = sub < 0 ? (int)(0u - (unsigned)sub) : sub;
            if (diff > 5) {
                cls[i * W + j] = (lv < rv) ? 1 : 2;
                out[i * W + j] = INT32_MIN;
            } else { cls[i * W + j] = 0; out[i * W + j] = lv; }
        }
}

/* ------------------------------------------------------------------------------------
 * a23  NCC                                              NCC/NCC.h:15-95
 * ---------------------------------------------------------------------------------- */
static double orc_ncc_cost(const uint8_t *a, const uint8_t *b, int W, int side)  /* :15-49 */
{
    double lm = 0, rm = 0, ls = 0, rs = 0, num = 0;
    int n = side * side;
    for (int i = 0; i < side; i++)
        for (int j = 0; j < side; j++) { lm += a[j * W + i]; rm += b[j * W + i]; } /* .at(j,i) :29-30 */
    lm /= n; rm /= n;
    for (int i = 0; i < side; i++)
        for (int j = 0; j < side; j++) {
            double x = a[i * W + j] - lm, y = b[i * W + j] - rm;
            ls += x * x;                                               /* pow(.,2) :40-41 */
            rs += y * y;
            num += x * y;
        }
    return num / (sqrt(ls) * sqrt(rs));
}

ORC_API void orc_ncc(const uint8_t *L, const uint8_t *R, int H, int W, int D, int win,
                     int i0, int i1, int32_t *disp /* [H][W] pre-zeroed */, double *cost_out /* nullable [H][W][D] */)
{
    int side = 2 * win + 1;
    double *cost = (double *)malloc(D * sizeof(double));
    if (i0 < win) i0 = win;
    if (i1 > H - win) i1 = H - win;
    for (int i = i0; i < i1; i++)
        for (int j = win; j < W - win; j++) {
            for (int d = 0; d < D; d++) {
                if (j - win - d >= 0)
                    cost[d] = orc_ncc_cost(L + (i - win) * W + (j - win),
                                           R + (i - win) * W + (j - win - d), W, side);
                else cost[d] = 255.0;                                  /* `invalid` 0xff :88 */
            }
            int best = 0; float m = (float)cost[0];                    /* WinTakeAll :53-67 */
            for (int d = 1; d < D; d++)
                if ((double)m < cost[d]) { best = d; m = (float)cost[d]; }
            disp[i * W + j] = best;
            if (cost_out) memcpy(cost_out + ((size_t)i * W + j) * D, cost, D * sizeof(double));
        }
    free(cost);
}

/* ------------------------------------------------------------------------------------
 * a24  ASW                                              ASW/ASW.h:16-47, 193-257, 329-431
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_asw_masks(int winSize, double sigma_s, double sigma_c, double *space /* side*side */,
                           double *color /* 256 */)
{
    int side = 2 * winSize + 3, c = (side - 1) / 2;
    for (int i = 0; i < side; i++) {
        double y = (double)((i - c) * (i - c));
        for (int j = 0; j < side; j++) {
            double x = (double)((j - c) * (j - c));
            space[i * side + j] = exp(-(x + y) / (2 * sigma_s * sigma_s));     /* :30 */
        }
    }
    for (int i = 0; i < 256; i++) color[i] = exp(-(i * i) / (2 * sigma_c * sigma_c)); /* :44 */
}

static float orc_asw_cost(const uint8_t *a, const uint8_t *b, int Wp, int side, int ctr,
                          const double *space, const double *color, int T)    /* :210-257 */
{
    int ca = a[ctr * Wp + ctr], cb = b[ctr * Wp + ctr];
    double sw = 0, sv = 0;
    for (int i = 0; i < side; i++)
        for (int j = 0; j < side; j++) {
            int pa = a[i * Wp + j], pb = b[i * Wp + j];
            double m0 = color[abs(pa - ca)] * space[i * side + j];
            double m1 = color[abs(pb - cb)] * space[i * side + j];
            double m2 = m0 * m1;
            int e = abs(pa - pb); if (e > T) e = T;                    /* :358-366 */
            sw += m2;
            sv += m2 * (double)e;
        }
    return (float)(sv / sw);
}

ORC_API void orc_asw(const uint8_t *Lp, const uint8_t *Rp, int Hp, int Wp, int D, int winSize,
                     const double *space, const double *color, int T, int view, int i0, int i1,
                     float *disp /* [H][W] */, float *cost_out /* nullable [H][W][D] */)
{
    int wins = winSize + 1, side = 2 * wins + 1;
    int W = Wp - 2 * wins, H = Hp - 2 * wins;
    float *cv = (float *)malloc(D * sizeof(float));
    if (i0 < 0) i0 = 0;
    if (i1 > H) i1 = H;
    for (int io = i0; io < i1; io++)
        for (int jo = 0; jo < W; jo++) {
            int i = io + wins, j = jo + wins;
            int undefined_chain = 0;
            for (int d = 0; d < D; d++) {
                if (view == 0) {
                    if (j - wins - d >= 0)
                        cv[d] = orc_asw_cost(Lp + (i - wins) * Wp + (j - wins),
                                             Rp + (i - wins) * Wp + (j - wins - d), Wp, side,
                                             wins, space, color, T);
                    else cv[d] = cv[d - 1];                            /* :371 */
                } else {
                    if (j + wins + d + 1 < Wp - wins)                  /* :401 */
                        cv[d] = orc_asw_cost(Rp + (i - wins) * Wp + (j - wins),
                                             Lp + (i - wins) * Wp + (j - wins + d), Wp, side,
                                             wins, space, color, T);
                    else if (d == 0) { cv[0] = 0.0f; undefined_chain = 1; } /* :424 reads [-1]: UB; all d equal */
                    else cv[d] = cv[d - 1];
                }
            }
            float mv = cv[0], best = 0;                                /* WinTakeAll :193-208 */
            for (int d = 1; d < D; d++) if (mv > cv[d]) { best = (float)d; mv = cv[d]; }
            disp[io * W + jo] = best;
            if (cost_out) {
                float *co = cost_out + ((size_t)io * W + jo) * D;
                for (int d = 0; d < D; d++) co[d] = undefined_chain ? NAN : cv[d];
            }
        }
    free(cv);
}

/* a22  CrossCheckDiaparity (ASW, float maps -> u8)       ASW.h:108-145 */
ORC_API void orc_asw_crosscheck(const float *dL, const float *dR, int H, int W, uint8_t *out)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            int lv = (int)dL[i * W + j];
            long idx = (long)i * W + j - lv;
            float rv = (idx >= 0 && idx < (long)H * W) ? dR[idx] : 0.0f;
            float diff = fabsf((float)lv - rv);
            out[i * W + j] = (diff > 5.0f) ? 0 : (uint8_t)lv;
        }
}

/* ------------------------------------------------------------------------------------
 * 8f n1/n2  staging + MedianFilter
 *   cvtColor(CV_BGR2GRAY): OpenCV 3.1.0 RGB2Gray<uchar> fixed point (third-party, not in this
 *   image; restated from its published source): (1868 B + 9617 G + 4899 R + 8192) >> 14.
 *   MedianFilter: AD-CensusV1/PostProcessing.h:314-344.
 * ---------------------------------------------------------------------------------- */
ORC_API void orc_bgr2gray(const uint8_t *bgr, int n, uint8_t *gray)
{
    for (int p = 0; p < n; p++)
        gray[p] = (uint8_t)((1868 * bgr[3 * p] + 9617 * bgr[3 * p + 1] + 4899 * bgr[3 * p + 2] + (1 << 13)) >> 14);
}

static int orc_cmp_float(const void *a, const void *b)
{
    float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

ORC_API void orc_median(const float *in, float *out, int W, int H, int wnd)
{
    int radius = wnd / 2;                                              /* :317 */
    float *buf = (float *)malloc((size_t)wnd * wnd * sizeof(float));
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            int n = 0;
            for (int r = -radius; r <= radius; r++)
                for (int c = -radius; c <= radius; c++) {
                    int row = i + r, col = j + c;
                    if (row >= 0 && row < H && col >= 0 && col < W) buf[n++] = in[row * W + col];   /* :333-335 */
                }
            qsort(buf, n, sizeof(float), orc_cmp_float);               /* std::sort :339 */
            out[i * W + j] = buf[n / 2];                               /* :341 */
        }
    free(buf);
}

/* RemoveSpeckles                                          PostProcessing.h:250-311
 * PINNED against oracle/_ref (ref_remove_speckles).  invalid_val is an int here as in the reference's signature.
 * The call site's argument `Invalid_Float` (+inf, main.cpp:93) converts to int at run time on x86 as INT_MIN
 * (cvttss2si), the value documented in include/smt.h -- but g++ folds `int(+inf)` at COMPILE time when the constant
 * is written at the call, and does not fold it to INT_MIN.  The reference wrapper therefore takes invalid_val as an
 * int argument and never passes Invalid_Float. */
ORC_API void orc_remove_speckles(float *d, int W, int H, int diff, unsigned min_area, int invalid_val)
{
    size_t n = (size_t)W * H;
    uint8_t *visited = (uint8_t *)calloc(n, 1);
    int *vec = (int *)malloc(n * sizeof(int));
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            if (visited[i * W + j] || d[i * W + j] == invalid_val) continue;      /* :262 float == int */
            size_t sz = 0, cur = 0, next;
            vec[sz++] = i * W + j;
            visited[i * W + j] = 1;
            do {
                next = sz;
                for (size_t k = cur; k < next; k++) {
                    int row = vec[k] / W, col = vec[k] % W;
                    float base = d[row * W + col];
                    for (int r = -1; r <= 1; r++)
                        for (int c = -1; c <= 1; c++) {
                            if (r == 0 && c == 0) continue;
                            int rr = row + r, cc = col + c;
                            if (rr >= 0 && rr < H && cc >= 0 && cc < W) {
                                if (!visited[rr * W + cc] && d[rr * W + cc] != invalid_val &&
                                    fabsf(d[rr * W + cc] - base) <= diff) {           /* :290-292 */
                                    vec[sz++] = rr * W + cc;
                                    visited[rr * W + cc] = 1;
                                }
                            }
                        }
                }
                cur = next;
            } while (next < sz);
            if (sz < min_area)
                for (size_t k = 0; k < sz; k++) d[vec[k]] = (float)invalid_val;     /* :304-308 */
        }
    free(visited); free(vec);
}

/* FillTheHole                                             PostProcessing.h:156-248
 * In place on disp (row*col floats).  The reference swaps the extents (`width = row`, `height =
 * col`, :158-159): the buffer is read as `col` lines of `row` entries.  occ / mis: (first, second)
 * pairs in list order.  Pass 0 fills the occlusion list (second smallest of the first valid values
 * found along 8 rays, :227-233), pass 1 the mismatch list (median, :235-237), pass 2 every entry
 * that still equals 65535 -- and replaces the caller's mismatch list by those (:186), returned in
 * third / *n_third (capacity row*col pairs).  Every write of a pass happens after all its reads
 * (:240-245).  Returns 0, or -1 where the reference itself writes out of bounds: a listed pair
 * outside the buffer, or more third-pass holes than the mismatch list had entries (`fill_disps` is
 * sized before the list is replaced, :180 vs :186). */
static int flt_cmp(const void *a, const void *b)
{
    float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}
ORC_API int orc_fill_the_hole(float *disp, int row, int col, int dispRange, const int *occ, int n_occ,
                              const int *mis, int n_mis, int *third, int *n_third)
{
    const int width = row, height = col;                                      /* :158-159 */
    const float pi = 3.1415926f;
    const float angle1[8] = {pi, 3 * pi / 4, pi / 2, pi / 4, 0, 7 * pi / 4, 3 * pi / 2, 5 * pi / 4};
    const float angle2[8] = {pi, 5 * pi / 4, 3 * pi / 2, 7 * pi / 4, 0, pi / 4, pi / 2, 3 * pi / 4};
    const float *angle = angle1;                                              /* sticky across passes, :166 */
    const int max_search_length = (int)(1.0 * dispRange);                     /* :168 */
    const long n = (long)row * col;
    if (n_third) *n_third = -1;                                               /* -1: list not replaced */
    for (int k = 0; k < 3; k++) {
        const int *trg = (k == 0) ? occ : mis;
        int nt = (k == 0) ? n_occ : n_mis;
        if (nt == 0) continue;                                                /* :174-176 */
        const int cap = nt;                                                   /* fill_disps(trg.size()), :177 */
        int *inv = NULL;
        if (k == 2) {                                                         /* :179-187 */
            inv = (int *)malloc((size_t)n * 2 * sizeof(int));
            int c = 0;
            for (int i = 0; i < height; i++)
                for (int j = 0; j < width; j++)
                    if (disp[i * width + j] == 65535.0f) { inv[2 * c] = i; inv[2 * c + 1] = j; c++; }
            trg = inv; nt = c;
            if (third) { memcpy(third, inv, (size_t)c * 2 * sizeof(int)); }
            if (n_third) *n_third = c;
            if (nt > cap) { free(inv); return -1; }
        }
        float *fill = (float *)calloc((size_t)(cap > 0 ? cap : 1), sizeof(float));
        for (int t = 0; t < nt; t++) {
            const int y = trg[2 * t], x = trg[2 * t + 1];
            const long at = (long)y * width + x;
            if (at < 0 || at >= n) { free(fill); free(inv); return -1; }
            if (y == height / 2) angle = angle2;                              /* :195-197 */
            float got[8]; int ng = 0;
            for (int s = 0; s < 8; s++) {
                const float ang = angle[s];
                const float sina = sinf(ang), cosa = cosf(ang);               /* sin(float) is the float overload, :203-204 */
                for (int m = 1; m < max_search_length; m++) {
                    const long yy = lroundf((float)y + (float)m * sina);      /* float arithmetic, :206-207 */
                    const long xx = lroundf((float)x + (float)m * cosa);
                    if (yy < 0 || yy >= height || xx < 0 || xx >= width) break;
                    const float d = disp[yy * width + xx];
                    if (d != 65535.0f) { got[ng++] = d; break; }
                }
            }
            if (ng == 0) continue;                                            /* fill stays 0, :218-220 */
            qsort(got, (size_t)ng, sizeof(float), flt_cmp);
            if (k == 0) fill[t] = ng > 1 ? got[1] : got[0];
            else fill[t] = got[ng / 2];
        }
        for (int t = 0; t < nt; t++) disp[(long)trg[2 * t] * width + trg[2 * t + 1]] = fill[t];   /* :240-245 */
        free(fill); free(inv);
    }
    return 0;
}

/* chooseArmLengthLeft / Right / Up / Down                  CBLSM.h:65-236
 * dir 0..3; own = ArmLL / ArmLR / ArmLUp / ArmLDown, vert = ArmRUp / ArmRDown (dir 2 / 3). */
ORC_API void orc_choose_arm_length(int dir, const int *own, const int *vert, const int *RL, const int *RR,
                                   int row, int col, int D, int *vol)
{
    for (int i = 0; i < row; ++i)
        for (int j = 0; j < col; ++j)
            for (int d = 0; d < D; d++) {
                int save = 0;
                const size_t p = (size_t)i * col + j;
                if (dir == 0) {
                    int LL = own[p], rl = RL[p], rr = RR[p];
                    if ((j - d < j - rl) || (j + d > j + rr)) { save = 0; }                    /* :76-82 */
                    else
                        for (int a = 1; a <= LL; a++) {
                            if (((j - a - d) >= (j - rl)) && ((j - a - d) <= (j + rr))) save++;  /* :87-88 */
                            else break;
                        }
                } else if (dir == 1) {
                    int LR = own[p], rl = RL[p], rr = RR[p];
                    if ((j - d < j - rl) || (j - d > j + rr)) { save = 0; }                    /* :123-129 */
                    else
                        for (int a = 1; a <= LR; a++) {
                            if ((j + a - d >= j - rl) && (j + a - d < j + rr)) save++;         /* :134-135 */
                            else break;
                        }
                } else if (dir == 2) {
                    int LUp = own[p], RUp = vert[p];
                    for (int up = 1; up <= LUp; up++) {                                        /* :164-185 */
                        int pr = i - up;
                        int pl = RL[(size_t)pr * col + j], prr = RR[(size_t)pr * col + j];
                        if (pr >= (i - RUp)) {
                            if (j - d < 0) break;
                            if (((j - d) < (j + prr)) && ((j - d) > (j - pl))) save++;
                        } else { save = 0; break; }
                    }
                } else {
                    int LDown = own[p], RDown = vert[p];
                    for (int down = 1; down <= LDown; down++) {                                /* :208-229 */
                        int pr = i + down;
                        int pl = RL[(size_t)pr * col + j], prr = RR[(size_t)pr * col + j];
                        if (pr <= i + RDown) {
                            if (j - d < 0) { save = 0; break; }
                            if ((j - d <= j + prr) && (j - d >= j - pl)) save++;
                        } else break;
                    }
                }
                vol[p * D + d] = save;
            }
}

/* CBLSM.h:969-1045 ComputeLocalValue + :1087-1126 costAggregationNew (dead experiments, SURVEY 8f n4;
 * call site commented out, CBLSM.cpp:113-116).  Lp / Rp: images replicate-padded by w = winSize + 1,
 * [Hp][Wp]; arm volumes int32 [H][W][D] with H = Hp - 2w, W = Wp - 2w (`_col_`).  The OpenCV calls are ROI
 * sums of 8-bit pixels (cv::sum -> double, exact); `value` is a float that takes each row's double sum
 * (:1004, :1012, :1022, :1035), the mean divides by a count that is L+R+1 per row although the ROI holds
 * L+R pixels (:1021, :1034 -- "a small error", says the author) and R+1 for a left-clipped row (:1011).
 * Rows or columns that would leave the padded image (impossible with arm volumes from
 * chooseArmLength*) are skipped.  The `#pragma omp parallel for` on the row loop (:982) races on
 * count / value; sequential semantics are the specification.
 * PARITY UNPINNED: both functions take their pixels through ROI by Range and cv::sum, which the container-only
 * header of the reference builds (oracle/ref_build/shim/opencv2/opencv.hpp) declares but does not imitate. */
static float orc_cblsm_local_value(const uint8_t *img, int Hp, int Wp, int i, int j, int Up, int Down, int w,
                                   const int *LArm, const int *RArm, int H, int W, int D, int d)
{
    int count = 0;
    float value = 0;
    const int ptrj = j - w;
    for (int r = -Up; r <= Down; r++) {
        int ptr_i = i - w + r;
        if (ptr_i < 0 || ptr_i >= H || i + r < 0 || i + r >= Hp) continue;
        int L = LArm[((size_t)ptr_i * W + ptrj) * D + d];
        int R = RArm[((size_t)ptr_i * W + ptrj) * D + d];
        int c0, c1;
        if (d > 0) {
            if (j - L - d < 0) {
                if (j + R - d <= 0) { c0 = 0; c1 = 1; count += 1; }                /* :994-997 */
                else { c0 = 0; c1 = j + R - d; count += R + 1; }                   /* :1006-1009 */
            } else { c0 = j - L - d; c1 = j + R - d; count += L + R + 1; }         /* :1018-1021 */
        } else {
            if (L == 0 && R == 0) { c0 = j; c1 = j + 1; }                          /* :1029-1031 */
            else { c0 = j - L; c1 = j + R; }                                       /* :1033-1035 */
            count += L + R + 1;
        }
        if (c0 < 0) c0 = 0;
        if (c1 > Wp) c1 = Wp;
        double sum = 0;
        for (int c = c0; c < c1; c++) sum += img[(size_t)(i + r) * Wp + c];
        value = (float)((double)value + sum);
    }
    return value / count;                                                          /* :1041 */
}

ORC_API void orc_cblsm_cost_aggregation_new(const uint8_t *Lp, const uint8_t *Rp, int Hp, int Wp, int winSize,
                                            const int *armL, const int *armR, const int *armUp, const int *armDown,
                                            int D, float *cost)
{
    const int w = winSize + 1, H = Hp - 2 * w, W = Wp - 2 * w;
    for (int i = w; i < Hp - w; ++i)
        for (int j = w; j < Wp - w; ++j)
            for (int d = 0; d < D; d++) {
                const size_t k = ((size_t)(i - w) * W + (j - w)) * D + d;
                const int Up = armUp[k], Down = armDown[k];
                float lv = orc_cblsm_local_value(Lp, Hp, Wp, i, j, Up, Down, w, armL, armR, H, W, D, 0);   /* :1111 */
                float rv = orc_cblsm_local_value(Rp, Hp, Wp, i, j, Up, Down, w, armL, armR, H, W, D, d);   /* :1113 */
                cost[k] = fabsf(lv - rv);                                                                /* :1114-1118 */
            }
}

/* FNV-1a 64 over raw bytes: fixture hashes */
ORC_API uint64_t orc_fnv1a(const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 1099511628211ull; }
    return h;
}
