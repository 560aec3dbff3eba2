/*
 * smt_refine.h -- AD-Census iterative region voting and outlier interpolation, batched (libsmt_hip.so; plain C99,
 * conventions of smt.h).
 *
 * After LeftRightConsistency every rejected pixel of the pipeline's left map is +inf, after RemoveSpeckles every
 * removed pixel is (float)INT_MIN.  The reference stops there; the AD-Census method goes on with iterative region
 * voting over the cross-based support region and interpolation of the remaining outliers, and the reference tree
 * carries that step's parameters (CBLSM/adcensus_types.h:58-59, 72: irv_ts = 20, irv_th = 0.4f, do_filling).
 * **Parity unpinned: no reference code.**  The rule below is the library's definition (csrc/refine_rule.h holds it as
 * code for the kernels and the host twins).  Every output is an integer or a copy of an
 * input float, so there is no tolerance anywhere.
 *
 * The rule.  Maps are float32 [H][W].  D is the disparity range, 1 <= D <= SMT_MAX_DISPARITY.
 *
 * Reliable
 * - A value v is reliable iff v >= 0.0f && v < (float)D.
 * - This is false for NaN, +-inf and (float)INT_MIN.  It is true for -0.0f.
 * - Its bin is min(D-1, (int)(v + 0.5f)).
 * - Every other pixel is an outlier.
 *
 * Region of p = (i, j)
 * - It is built from four int32 [H][W] arm maps aL, aR, aT, aB, read at flat index r*W + c.
 * - Every length is clamped into 0..255.  A clamp sets flag SMT_REFINE_ARM_CLAMPED in that map's status word.
 *   (The flag is set when any of the 4*H*W lengths of that map's arm maps lies outside 0..255, whether or not an
 *   outlier's region reads it.)
 * - The rows are r = max(0, i - aT[p]) .. min(H-1, i + aB[p]).
 * - In row r, with q = (r, j), the columns are max(0, j - aL[q]) .. min(W-1, j + aR[q]).
 * - A region therefore has at most 511 x 511 pixels, fewer than 2^18.
 *
 * One voting iteration
 * - It reads map M and writes map M'.  No pixel of M' depends on another pixel of M'.
 * - A reliable pixel is copied bit for bit.
 * - An outlier p counts the reliable pixels of its region in M, per bin.
 *   - S is their number.
 *   - d* is the smallest bin with the largest count h.
 * - M'(p) = (float)d* iff S > irv_ts and (double)h > (double)irv_th * (double)S.  Both products are exact in double
 *   at these sizes.
 * - Otherwise M'(p) = M(p), bit for bit.
 * - irv_iters iterations run, default 5.  Values from 0 to 16 are accepted.
 *
 * Interpolation
 * - It runs after the voting.  It is evaluated on the map as it stands when the voting ends, for every pixel at once.
 * - A pixel filled by interpolation is never a candidate for another pixel.
 * - Each remaining outlier p casts 16 rays.  The steps (dy, dx) are, in this order:
 *   - (0,1), (1,2), (1,1), (2,1)
 *   - (1,0), (2,-1), (1,-1), (1,-2)
 *   - (0,-1), (-1,-2), (-1,-1), (-2,-1)
 *   - (-1,0), (-2,1), (-1,1), (-1,2)
 * - Ray n probes p + k*step_n for k = 1, 2, ...
 *   - It continues while the probe is inside the image.
 *   - It stops at k <= search when search > 0.  search = 0, the default, goes to the border.
 *   - Its candidate is the first reliable pixel it meets.
 * - The winner depends on the class map cls, as smt_lrcheck writes it:
 *   - Class 1 (occlusion) takes the candidate with the smallest value.  Ties go to the lower ray index.
 *   - Every other class takes the candidate with the smallest |gray(p) - gray(q)| on the uint8 left image.  Ties go
 *     to the lower ray index.
 * - The winner's float is copied bit for bit.
 * - A pixel with no candidate stays as it was.
 *
 * Optional outputs per map
 * - state uint8 [H][W]:
 *   - 0 means reliable on entry.
 *   - k means filled by voting iteration k (1..16).
 *   - 254 means filled by interpolation.
 *   - 255 means still an outlier.
 * - status int32 [4]: {outliers on entry, filled by voting, filled by interpolation, flags}.
 *
 * Batch conventions as smt_median_filter_batch: `pairs` maps, every stride in ELEMENTS, 0 = dense (H*W), otherwise
 * >= H*W; nothing outside the H*W elements of a map, a state map or the 4 status words of a pair is written.  All
 * device entries are asynchronous on `stream`, never wait on the host, and enqueue a fixed number of launches whatever
 * the data and the pair count: one opening launch, irv_iters voting launches, one interpolation launch (plus one
 * memset when status != NULL).  Scratch comes from the library's arena: one float map per pair (pairs*H*W*4 bytes)
 * and, for the direct voting form, at most 32768 * D counters.
 * SMT_ERR_ARG, before any device work: NULL required pointers, pairs < 0, non-positive sizes, H*W >= 2^31, D outside
 * 1..SMT_MAX_DISPARITY, irv_iters outside 0..16, search < 0, strides below H*W.  pairs == 0 is a no-op for the
 * stateless entries.  params == NULL: the defaults.
 */
#ifndef SMT_REFINE_H_
#define SMT_REFINE_H_

#include "smt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_REFINE_ARM_CLAMPED 1        /* status[3]: an arm length outside 0..255 was clamped */

#define SMT_REFINE_STATE_INTERPOLATED 254
#define SMT_REFINE_STATE_OUTLIER 255

#define SMT_REFINE_FORM_DIRECT 1        /* one thread per pixel, its counters in global scratch */
#define SMT_REFINE_FORM_WAVE 2          /* one wave per outlier, its counters in LDS */

typedef struct smt_refine_params {
    int irv_ts;       /* 20   (adcensus_types.h:58, 72) */
    float irv_th;     /* 0.4f (adcensus_types.h:59, 72) */
    int irv_iters;    /* 5, 0..16 */
    int search;       /* 0 = to the border; > 0: at most that many probes per ray */
} smt_refine_params;

void smt_refine_default_params(smt_refine_params *p);

/* irv_iters voting iterations on `pairs` DEVICE maps, in place.  armL, armR, armT, armB: DEVICE int32 [pairs][H][W],
 * arm_stride elements apart (the same for all four).  state (uint8 [pairs][H][W], state_stride apart) and status
 * (int32 [pairs][4], dense) may be NULL.  status[2] is 0. */
int smt_region_vote_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT,
                          const int *armB, size_t arm_stride, int H, int W, int D, const smt_refine_params *params,
                          uint8_t *state, size_t state_stride, int *status, void *stream);

/* The interpolation alone on `pairs` DEVICE maps, in place.  cls: uint8 [pairs][H][W] as smt_lrcheck writes it; gray:
 * the uint8 left images [pairs][H][W].  Only params->search is used.  status[1] and status[3] are 0. */
int smt_interpolate_outliers_batch(float *maps, int pairs, size_t map_stride, const uint8_t *cls, size_t cls_stride,
                                   const uint8_t *gray, size_t gray_stride, int H, int W, int D,
                                   const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status,
                                   void *stream);

/* Voting, then interpolation. */
int smt_refine_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT,
                     const int *armB, size_t arm_stride, const uint8_t *cls, size_t cls_stride, const uint8_t *gray,
                     size_t gray_stride, int H, int W, int D, const smt_refine_params *params, uint8_t *state,
                     size_t state_stride, int *status, void *stream);

/* The same three on HOST buffers, no GPU: plain loops through the rule header the kernels include. */
int smt_region_vote_batch_host(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR,
                               const int *armT, const int *armB, size_t arm_stride, int H, int W, int D,
                               const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status);
int smt_interpolate_outliers_batch_host(float *maps, int pairs, size_t map_stride, const uint8_t *cls, size_t cls_stride,
                                        const uint8_t *gray, size_t gray_stride, int H, int W, int D,
                                        const smt_refine_params *params, uint8_t *state, size_t state_stride,
                                        int *status);
int smt_refine_batch_host(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT,
                          const int *armB, size_t arm_stride, const uint8_t *cls, size_t cls_stride, const uint8_t *gray,
                          size_t gray_stride, int H, int W, int D, const smt_refine_params *params, uint8_t *state,
                          size_t state_stride, int *status);

/* Test hooks.  impl 0 = the default, SMT_REFINE_FORM_DIRECT, SMT_REFINE_FORM_WAVE: the voting
 * formulation; identical bits.  last_form: what the last voting launch was (0: none yet). */
int smt_refine_set_impl(int impl);
int smt_refine_last_form(void);

/* smt_pipeline_run_batch_post with the refinement between RemoveSpeckles and MedianFilter: per pair, on the caller's
 * stream, at the place the tail runs, LR check, RemoveSpeckles, refine (smt_refine_batch on dispL with the pair's cls
 * and left image), then MedianFilter into lastDisp.  The arms are those of the pair's LEFT image, recomputed by a
 * crossarm handle of the tail's own (the pipeline's tao and quirk bits; created by the first refined call): two more
 * launches per pair.  refine == NULL: the defaults.  state: uint8 [pairs][H][W] dense or NULL; status: int32
 * [pairs][4] or NULL.  Everything else as smt_pipeline_run_batch_post, whose behaviour does not change. */
int smt_pipeline_run_batch_refined(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                                   float *dispR, uint8_t *cls, int *counts, const smt_post_params *post,
                                   const smt_refine_params *refine, float *lastDisp, uint8_t *state, int *status);

#ifdef __cplusplus
}
#endif

#endif /* SMT_REFINE_H_ */
