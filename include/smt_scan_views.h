/*
 * smt_scan_views.h -- the scanline optimiser on both views (libsmt_hip.so; plain C99, conventions of smt.h).
 *
 * AD-CensusV1/main.cpp runs ScanlineOptimizer on the left aggregated volume only (:86-89) and then cross-checks that map
 * against the plain WTA of the aggregated right volume (:84, :92).  ScanlineOptimizer::ScanLine(vol, gray) does not know
 * which view it is given: the entry points below run it on two volumes at once, run it without storing the sum, and let
 * the pipeline give the right view the treatment the left one gets.  Nothing in smt.h changes its results or its code;
 * every default is the reference's flow.  DESIGN.md section 5.18.
 */
#ifndef SMT_SCAN_VIEWS_H_
#define SMT_SCAN_VIEWS_H_

#include "smt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ScanLine (+ WTA) on two volumes of the handle's shape: per view exactly what smt_scanline_run(h, vin, gray, vout, disp)
 * writes, bit for bit, under the handle's quirks and sub-pixel switch.  The views share the grid of each pass (left /
 * right, up, down), so both views' scanlines are resident together: three launches when both views ask for a map, four
 * when one asks for none (the last pass then runs per view).  That pays while one view leaves the device partly idle;
 * where one view's left / right launch already has more than a wave per SIMD (H > 512 on the MI355X) the call issues the
 * single-view launches view after view instead -- the same results (csrc/scanline.hip has the measurements).
 *   vin*, vout*  float32 [H][W][D];  gray*  float32 [H][W];  disp*  float32 [H][W]
 * Per view vout may be NULL when disp is not: that view runs the maps-only last pass, which reads the sum of the first
 * three passes from scratch the handle owns and stores the map only (8 bytes per hypothesis instead of 12).  Both NULL
 * for a view is SMT_ERR_ARG; so is a vout that is one of the inputs or the other vout, and dispL == dispR.  vinL == vinR
 * is allowed.
 * Scratch: a handle holds up to four [H][W][D] float volumes -- per view the right path and, for a view without vout, the
 * running sum -- each allocated by the first call that needs it (smt_scanline_run needs one, smt_scanline_run_map two)
 * and kept until smt_scanline_destroy.
 * Asynchronous on the handle's stream only. */
int smt_scanline_run_pair(smt_scanline *h, const float *vinL, const float *grayL, float *voutL, float *dispL,
                          const float *vinR, const float *grayR, float *voutR, float *dispR);

/* One view, maps only: disp is what smt_scanline_run writes, no volume is returned.  Two scratch volumes.  SMT_ERR_ARG
 * for a NULL argument.  Asynchronous on the handle's stream only. */
int smt_scanline_run_map(smt_scanline *h, const float *vol_in, const float *gray, float *disp);

/* Which views the pipeline's scanline optimiser runs on, between runs.
 *   SMT_VIEW_LEFT   the default: smt_pipeline_run_batch and _post as smt.h describes them, bit for bit, launching the
 *                   same kernels.
 *   SMT_VIEW_BOTH   dispR becomes the WTA of the right view's scanline sum: ScanLine on the aggregated right volume
 *                   guided by the float right image (main.cpp's rightptr) with the same p1 and p2, refined when
 *                   smt_pipeline_set_subpixel is on.  LeftRightConsistency and, under _post, RemoveSpeckles and
 *                   MedianFilter then run on those maps, unchanged.  SMT_QUIRK_FIX_SCAN_VERTICAL acts on both views.
 *                   dispL before the LR check, the left view's volumes and smt_pipeline_volumes are as under LEFT.
 *   anything else (SMT_VIEW_RIGHT alone included) is SMT_ERR_ARG.
 * Results are identical under every SMT_PIPE_SCHEDULE.  Under schedule 0 each pair runs one smt_scanline_run_pair on the
 * caller's stream; under 1 and 2 the right view's scan follows the right view's aggregation on the handle's side stream,
 * on a second scanline handle, beside the next pair's AD-Census and left aggregation (csrc/pipeline.hip).
 * Memory: the first BOTH run -- not create, not this call -- allocates three more [H][W][D] float volumes,
 * 12 * H * W * D bytes (the right view's sum, its right path and its maps-only running sum), and under schedule 1 a
 * second float right image, 4 * H * W bytes.  They are kept until smt_pipeline_destroy. */
int smt_pipeline_set_scan_views(smt_pipeline *h, int views);

/* Lends the right view's scanline sum, float32 [H][W][D], of the last pair of the last SMT_VIEW_BOTH call (valid until the
 * next BOTH call or destroy; order reads after the call on the handle's stream).  Pairs 0 .. n-2 of a call run the
 * maps-only last pass for the right view and store no sum; the left view stores every pair's, as smt_pipeline_volumes
 * promises.  SMT_ERR_STATE before a BOTH call has run, SMT_ERR_ARG for a NULL argument. */
int smt_pipeline_scan_right_volume(smt_pipeline *h, float **sum);

#ifdef __cplusplus
}
#endif

#endif /* SMT_SCAN_VIEWS_H_ */
