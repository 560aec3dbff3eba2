/*
 * smt_bilateral.h -- the reference's bilateral image filter, batched (libsmt_hip.so; plain C99, conventions of smt.h).
 *
 * ASW/BiliteralFilter.h:49-142, bilateralfiter(src, dst, wsize, spaceSigma, colorSigma), is the plain bilateral filter
 * that ASW/TeddyBilateral.cpp was written to run on the Teddy pair before matching.  These entry points are that
 * function: 1 or 3 channels, each channel on its own, replicate padding, the space mask and the colour table of
 * :12-43 (the formulas of ASW.h:16-47).  bilateralfiterWight (:145-242, which does not compile) and ASW.h's
 * bilateralfiter (:260-327, no defined result) stay out.
 *
 * The rule (csrc/bilateral_rule.h), float64 with one rounding per operation, no contraction:
 *   h = wsize_h, w = wsize_w, hh = (h - 1) / 2, ww = (w - 1) / 2 (integer division: an even size acts as the odd size
 *   below it).  space is an h x w table with row stride w of which rows 0..2hh and columns 0..2ww are used; color has
 *   256 entries.  For a pixel, a channel and the taps t = (r, c), r = -hh..hh outer, c = -ww..ww inner, q_t the source
 *   sample at the clamped position (copyMakeBorder BORDER_REPLICATE, :63):
 *     pass 1   wt[t] = color[|q_t - centre|] * space[t];   S = S + wt[t], from 0.0                          (:71-97)
 *     norm     SMT_BILATERAL_NORM_RECIPROCAL  wn[t] = wt[t] * (1.0 / S)     what OpenCV 3.1's Mat / double evaluates
 *              SMT_BILATERAL_NORM_DIVIDE      wn[t] = wt[t] / S                                             (:100-106)
 *     pass 2   acc = acc + (double)q_t * wn[t], from 0.0, the same order                                    (:109-122)
 *     output   acc < 0 -> 0, acc > 255 -> 255, truncation toward zero; a NaN acc gives 0 (the x86 value of the
 *              reference's undefined cast; reachable only with caller tables whose weights sum to 0 or overflow)
 * The normalisation is an OpenCV MatExpr: which of the two forms it is cannot be settled without OpenCV, so that step
 * is parity unpinned; both forms are here.  The sums' order is observable: a flat 255 comes out as 254 at 23 x 23.
 *
 * Limits (SMT_ERR_ARG outside): channels 1 or 3; 1 <= wsize_h, wsize_w <= 64; dst != src; images >= 0, H, W > 0.
 */
#ifndef SMT_BILATERAL_H_
#define SMT_BILATERAL_H_

#include "smt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_BILATERAL_NORM_RECIPROCAL 0
#define SMT_BILATERAL_NORM_DIVIDE 1

#define SMT_BILATERAL_FORM_DIRECT 1
#define SMT_BILATERAL_FORM_STAGED 2

/* getGausssianMask (:12-31) and getColorMask (:36-43) on the host with libm: space_host float64 [wsize_h][wsize_w],
 * color_host float64 [256]. */
int smt_bilateral_masks(int wsize_h, int wsize_w, double sigma_space, double sigma_color, double *space_host,
                        double *color_host);

/* bilateralfiter on `images` dense images.  src, dst: DEVICE uint8 [images][H][W][channels]; space, color: DEVICE
 * float64 tables, all wsize_h * wsize_w and 256 entries may be read; norm: SMT_BILATERAL_NORM_*; acc: NULL, or DEVICE
 * float64 [images][H][W][channels], the unclamped sums of pass 2 (a diagnostic output like the matchers' cost
 * volumes).  images == 0 is a no-op.  One launch, asynchronous on `stream`, no host wait, no scratch. */
int smt_bilateral_filter_batch(const uint8_t *src, int images, int H, int W, int channels, int wsize_h, int wsize_w,
                               const double *space, const double *color, int norm, uint8_t *dst, double *acc,
                               void *stream);

/* The same on HOST buffers, no GPU: direct loops through the rule header the kernels include. */
int smt_bilateral_filter_host(const uint8_t *src, int images, int H, int W, int channels, int wsize_h, int wsize_w,
                              const double *space, const double *color, int norm, uint8_t *dst, double *acc);

/* Test hooks.  impl 0 = the measured default, SMT_BILATERAL_FORM_DIRECT = one thread per
 * pixel from global memory, SMT_BILATERAL_FORM_STAGED = the LDS-staged tile kernel.  last_form: what the last
 * smt_bilateral_filter_batch launched (0: none yet). */
int smt_bilateral_set_impl(int impl);
int smt_bilateral_last_form(void);

#ifdef __cplusplus
}
#endif

#endif /* SMT_BILATERAL_H_ */
