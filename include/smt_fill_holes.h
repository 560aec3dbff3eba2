/*
 * smt_fill_holes.h -- SAD/Sad.h's in-place FillHolesInDispMap (Sad.h:317-400, named at SADmain.cpp:79), batched
 * (libsmt_hip.so; plain C99, conventions of smt.h).
 *
 * LeftRightConsistency marks every pixel it rejects +inf.  smt_fill_the_hole[_batch] is PostProcessing.h's FillTheHole
 * as written: it looks for 65535 and never sees those holes.  This is the reference's filler that does: it takes the
 * map as float, the invalid value as a parameter, the true extents, and has no search cap.  It writes into the map it
 * reads, so a pixel sees the fills of the pixels before it in list order; the result below is that raster-order
 * recurrence, exactly.
 *
 * The rule, Sad.h:317-400 read sequentially.  (The `#pragma omp parallel for` on the pass loop is ignored, as in every
 * pinned build of this library: a parallel pass loop has no defined result.)  csrc/fillholes_rule.h holds it as code
 * for the kernel and the host twin.
 *
 * Inputs
 * - M is float32 [H][W], modified in place.
 * - occ and mis are the pixels of class 1 and class 2 of a class map `cls` as smt_lrcheck writes it, in raster order:
 *   the lists LeftRightConsistency and CrossCheckDiaparity produce.  Other class values are not targets.  The function
 *   takes the lists by value, so the caller's lists do not change.
 * - invalid is a float, +inf for the pipeline's maps.
 *
 * Passes
 * - Pass 0 visits occ, pass 1 visits mis, pass 2 visits every pixel with M == invalid at the moment pass 2 starts, in
 *   raster order.
 * - All three always run.  There is no empty() gate as in FillTheHole.
 *
 * One pixel (y, x)
 * - Each of eight directions is walked for n = 1, 2, ...: yy = (int)((float)y + (float)n * sina),
 *   xx = (int)((float)x + (float)n * cosa).  These are float32 operations, each rounded on its own (no fused
 *   multiply-add), with truncation toward zero.
 * - The walk leaves the image (yy < 0 || yy >= H || xx < 0 || xx >= W) and contributes nothing, or it stops at the
 *   first pixel with M != invalid IN THE MAP'S CURRENT STATE and contributes that value.  There is no length cap.
 * - If nothing was collected, the pixel is left as it is.
 * - Otherwise the collected values are sorted ascending.  Pass 0 writes element 1 if there are at least two values,
 *   else element 0.  Passes 1 and 2 write element size / 2.
 *
 * The sixteen constants
 * - pi = 3.1415926f; the angles are pi, 3*pi/4, pi/2, pi/4, 0, 7*pi/4, 3*pi/2, 5*pi/4, evaluated in float32; sina and
 *   cosa are sinf and cosf of them.  csrc/fillholes_rule.h keeps them as hex-float literals (glibc's values; against
 *   MSVC's libm the last ulp is unpinned).
 * - sinf(pi), cosf(pi/2) and cosf(3*pi/2) are small and positive, so the axis rays stay on their row or column.
 * - The diagonal rays are staircases (|sina|, |cosa| about 0.7071): their first step can be a same-row or same-column
 *   neighbour.
 * - A coordinate in (-1, 0) truncates to 0.  A ray at the top or left border therefore visits row or column 0 once more
 *   before it leaves: the pixel itself from (0, x) up-right, (y - 1, 0) from (y, 0) up-left.  A listed pixel that is not
 *   invalid can thus collect itself.
 * - `angle = angle2` after the first target in row H / 2 permutes the same eight directions, and the values are
 *   sorted: it changes nothing.
 *
 * Decided corners
 * - std::sort leaves the order of -0.0f and +0.0f open.  A collected -0.0f counts and is written as +0.0f.
 * - A NaN anywhere in a map, `invalid` being anything else, makes the sort undefined.  That map is not modified and its
 *   status flags carry SMT_FILLHOLES_UB_NAN; the other maps of the call are unaffected.
 * - invalid NaN is SMT_ERR_ARG (no pixel equals it).
 *
 * status is int32 [pairs][4] = {n_occ, n_mis, n_third, flags}: the pixels of class 1, of class 2, and the targets of
 * pass 2 (0 for a map with SMT_FILLHOLES_UB_NAN).  All four words of every pair are written.
 *
 * Extents: 1 <= H, W <= SMT_FILLHOLES_MAX_DIM.  Far beyond it an axis ray drifts off its row and the float32 steps
 * stop being integers; the limit is the size up to which the tests hold the ordering property of the device
 * formulation.
 */
#ifndef SMT_FILL_HOLES_H_
#define SMT_FILL_HOLES_H_

#include "smt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_FILLHOLES_UB_NAN 1          /* status[3]: the map holds a NaN; it was not modified */
#define SMT_FILLHOLES_MAX_DIM 8192

/* FillHolesInDispMap on `pairs` DEVICE maps, in place.  maps: float32 [pairs][H][W], map_stride ELEMENTS apart; cls:
 * uint8 [pairs][H][W] as smt_lrcheck writes it, cls_stride elements apart; a stride of 0 means dense (H*W), otherwise
 * it is >= H*W.  status: DEVICE int32 [pairs][4] or NULL.  Asynchronous on `stream`, never waits on the host.  One
 * launch whatever the data and the pair count (one workgroup per map runs the three passes), no scratch.  Nothing
 * outside the H*W elements of a map and the 4 status words of a pair is written; cls is only read.  pairs == 0 is a
 * no-op.  SMT_ERR_ARG, before any device work: NULL maps or cls, pairs < 0, H or W outside
 * 1..SMT_FILLHOLES_MAX_DIM, a stride below H*W, invalid NaN. */
int smt_fill_holes_batch(float *maps, const uint8_t *cls, int pairs, size_t map_stride, size_t cls_stride, int H, int W,
                         float invalid, int *status, void *stream);

/* The same on HOST buffers, no GPU: plain raster-order loops through the rule header the kernel includes. */
int smt_fill_holes_batch_host(float *maps, const uint8_t *cls, int pairs, size_t map_stride, size_t cls_stride, int H,
                              int W, float invalid, int *status);

/* TEST HOOKS into the rule header, host side: for the library's own tests, not a stable interface; they may change or
 * go in any release.  smt_fill_holes_constants: out[0..7] = sina, out[8..15] = cosa of rays
 * 0..7.  smt_fill_holes_probe: the pixel (yy, xx) that ray `ray` (0..7) of pixel (y, x) visits at step n >= 1. */
void smt_fill_holes_constants(float *out16);
int smt_fill_holes_probe(int y, int x, int ray, int n, int *yy, int *xx);
/* Every pixel that ray `ray` of pixel (y, x) visits before it leaves an H x W image, in order, into yy[] and xx[]
 * (room for `cap` each) -> their number, or SMT_ERR_ARG (a bad argument, or more than cap). */
int smt_fill_holes_walk(int H, int W, int y, int x, int ray, int *yy, int *xx, int cap);
/* The first `passes` (0..3) passes of the host twin on one dense HOST map; a map with a NaN is left alone. */
int smt_fill_holes_host_passes(float *map, const uint8_t *cls, int H, int W, float invalid, int passes);

/* smt_pipeline_run_batch with this filler and the median behind the LR check: per pair, on the caller's stream, at
 * the place the tail runs, LR check, smt_fill_holes_batch on dispL with the pair's cls, then MedianFilter (window
 * median_wnd, 1..7) into lastDisp.  There is no RemoveSpeckles stage: its (float)INT_MIN marks are != invalid and so
 * are not holes to this filler (Sad.h's own float RemoveSpeckles is not built).  status: int32 [pairs][4] or NULL.
 * lastDisp: float32 [pairs][H][W], not dispL; NULL skips the median (dispL is then the only product of the tail).
 * The same results under every SMT_PIPE_SCHEDULE.  Everything else as smt_pipeline_run_batch, whose behaviour, like
 * that of _post and _refined, does not change. */
int smt_pipeline_run_batch_filled(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                                  float *dispR, uint8_t *cls, int *counts, int median_wnd, float invalid,
                                  float *lastDisp, int *status);

#ifdef __cplusplus
}
#endif

#endif /* SMT_FILL_HOLES_H_ */
