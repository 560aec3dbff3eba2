/*
 * smt_sad_subpixel.h -- sub-pixel disparities of the SAD family (libsmt_hip.so; plain C99, conventions of smt.h).
 *
 * SAD/Sad.h:76-81 is where the reference fits the parabola through the winner and its two neighbours: OptimalDisparity
 * computes final_disp and returns best_disp.  These entry points return it.  The integer entry points of smt.h (smt_sad,
 * smt_sad_both, smt_sad_flow_run_batch) keep their code and their results.
 *
 * The rule (csrc/sad_subpixel_rule.h), float32 with one rounding per operation, min_den from
 * smt_subpixel_params (NULL = the default 1, the literal of Sad.h:80; non-finite or <= 0 gives SMT_ERR_ARG):
 *   left view   r = the integer smt_sad returns for the pixel (OptimalDisparity, Sad.h:40-85, on the `sad` row with its
 *               chain entries sad[d] = sad[d-1] for d > x).  r == 0 -> 0.0f (the uniqueness test :66, both ends :71,
 *               D <= 2); r == 65535 -> 65535.0f (no entry with d >= 1 below 0xffff); otherwise
 *                 s = (sad[r-1] + sad[r+1]) - 2 sad[r];  den = min_den < s ? s : min_den;
 *                 result = r + (sad[r-1] - sad[r+1]) / (2 den).
 *               sad[0] takes no part in the minimum search (:46), so sad[r-1] may lie below the minimum and the offset
 *               is then not bounded by 1/2: that is what :76-81 compute.
 *   right view  w = the integer smt_sad returns (GetMinSadIndex, :22-38, on the row c(d) for d <= dmax = min(D-1, W-1-x')
 *               and c(dmax) beyond, :167-171); w == 0 or w == D - 1 keeps w, otherwise the same formula on row[w-1],
 *               row[w], row[w+1] (row[w+1] == row[w] when w == dmax < D - 1).  The last row and column are 0.0f.
 * Every cost is an integer below 2^24: the sums are exact, only the division and the final add round, and the maps equal
 * a NumPy restatement bit for bit (tests/sad_subpixel_cases.py).
 *
 * Every entry writes the integer winner maps too when given a buffer for them: exactly smt_sad's maps.
 */
#ifndef SMT_SAD_SUBPIXEL_H_
#define SMT_SAD_SUBPIXEL_H_

#include "smt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One view.  Lp, Rp, H, W, D, winsize, view as smt_sad, and smt_sad's argument checks plus min_den.  disp float32 [H][W];
 * winner int32 [H][W] or NULL: exactly smt_sad's map.  Runs the formulation smt_sad_set_impl selects (the neighbours
 * come from the registers of the wave that holds the row).  Asynchronous on `stream`. */
int smt_sad_subpixel(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize, int view,
                     const smt_subpixel_params *params, float *disp, int32_t *winner, void *stream);

/* Both views from one evaluation of the hypotheses, as smt_sad_both: the same three forms behind the same hooks
 * (smt_sad_both_set_impl, _set_dispatch, _set_band; smt_sad_both_last_form reports what ran).  dispL, dispR float32
 * [H][W]; winL, winR int32 [H][W] or NULL: exactly smt_sad_both's maps; costL float32 [H][W][D] or NULL as smt_sad_both's.
 * The left view is refined inside the box kernel.  The right view's neighbours are costs of other left pixels: under
 * impl 2 a second launch recomputes the two neighbour window sums of every right pixel from the images (work grows with
 * the window), under impl 1 they are gathered from the left volume (work grows with D).  By default (dispatch 0, impl 2)
 * a measured rule chooses between the two -- the volume where side^2 > 9 D - 200 and it fits 2 GiB (DESIGN.md section
 * 5.17) --; smt_sad_both_set_dispatch(1) obeys impl to the letter.  Scratch arena: 4 * H * W bytes, 4 * H * W * D where
 * the volume form runs without costL.  Asynchronous on `stream`. */
int smt_sad_both_subpixel(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize,
                          const smt_subpixel_params *params, float *dispL, float *dispR, int32_t *winL, int32_t *winR,
                          float *costL, void *stream);

/* The same maps on host buffers, no GPU: direct loops over the windows through the same rule header.  Lp, Rp uint8
 * [H+2w][W+2w] as smt_sad; any of the four outputs may be NULL. */
int smt_sad_subpixel_host(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize,
                          const smt_subpixel_params *params, float *dispL, float *dispR, int32_t *winL, int32_t *winR);

/* smt_sad_flow_run_batch with sub-pixel maps, on the same handle: pad (SADmain.cpp:47-48), both views through
 * smt_sad_both_subpixel (:66-67), CrossCheckDiaparity (:68) decided on the integer winners -- its index j - leftvalue
 * and its abs are integer -- so cls uint8 [pairs][H][W] is exactly what smt_sad_flow_run_batch writes.  dispL, dispR,
 * lastdisp float32 [pairs][H][W]; lastdisp is dispL where the check accepts and +inf (Invalid_Float, Sad.h:13) where it
 * rejects.  Any output may be NULL.  The first such call on a handle allocates the handle's float maps; a warm call
 * allocates nothing beyond the scratch arena.  Asynchronous on the handle's stream. */
int smt_sad_flow_run_batch_subpixel(smt_sad_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                    const smt_subpixel_params *params, float *dispL, float *dispR, float *lastdisp,
                                    uint8_t *cls);

#ifdef __cplusplus
}
#endif

#endif /* SMT_SAD_SUBPIXEL_H_ */
