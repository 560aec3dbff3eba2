// The north-star pipeline of AD-CensusV1/main.cpp:57-92 as one batched entry point ("batch
// variants taking a pair count and strides"; BASELINE.json configs[2] sharded like configs[4]):
//   uchar gray pair -> float copies (:46-55) -> AD_Census both views + WTA (:57-61) -> CrossArmAggregation on
//   the left and on the right image (:67-84) -> ScanlineOptimizer on the LEFT aggregated volume guided by the
//   float left image (:86-89, enabled) -> LeftRightConsistency (:92).
// Nothing here computes: it sequences the library's own entry points and owns the three [H][W][D] volumes
// between the stages, so a batch of pairs reuses them (9.6 GB at 1920x1080x192 whatever the batch size).
// Pairs are independent, which makes this the sharding unit for the pair axis.
// Schedules.  SMT_PIPE_SCHEDULE=2: three streams and double-buffered front-end state, so that kernels with
// different bottlenecks run side by side (tools/overlap_probe.py: the scanline passes are HBM / latency bound with
// 2 160 waves in flight, the aggregation is vector-issue bound; side by side they take 8.75 ms where one after the
// other takes 9.65 at 1920x1080 D=192; a high-priority stream or raised wave priority for the scanline, or compute
// units masked out of the aggregation's stream, all measured worse or equal):
//   front  F : u8 -> f32, AD-Census of pair b into table / volume / float-image set b & 1   (store bound)
//   main   M : arms + aggregation of the left view, LR check of pair b - 1, scanline of pair b
//   side   S : arms + aggregation of the right view (its own crossarm handle), beside the scanline of the same pair
// Event edges for pair b, set s = b & 1:
//   M: in      --> F                       the caller's inputs are ordered before everything
//   M: scan(b-2) done, S: right(b-2) done --> F     set s is free again (float images, cost volumes)
//   F: front(b) --> M                      arms(left), aggregate(left) --ev_left--> S: arms(right), aggregate(right)
//   S: right(b-1) --> M                    LR check of pair b - 1, issued after aggregate(left, b): the right view of
//                                          b - 1 has had that whole aggregation to finish, M never waits for it
//   after the loop: S: right(last) --> M: LR check(last).  Every call leaves all its work ordered on the caller's stream.
// SMT_PIPE_SCHEDULE=1 (the default) is the two-stream form: both views' arms beside the AD-Census of the same pair and
// the right view's aggregation (its own crossarm handle) beside the left view's scanline, nothing else double-buffered; SMT_PIPE_SCHEDULE=0 runs everything on the caller's stream.
// Measured at 1920x1080 D=192, 8 pairs per call, ms per pair: 10.7 (0), 9.66-9.76 (1), 9.61-9.66 (2) -- the third
// stream buys 1 % for a second AD-Census handle (3.3 GB) and a second crossarm handle, hence the default.
// smt_pipeline_run_batch_post adds main.cpp:93-94 (RemoveSpeckles, MedianFilter) per pair, on M right after that
// pair's LR check in every schedule: the tail is a few launches on one map, M already holds the map, and on S it would
// sit in front of the right view's aggregation that the next LR check waits for.  Its scratch (one pair's speckle
// forest and counts, an error word) is the handle's, allocated by the first _post call; tails follow each other on M,
// so one set serves every pair.
// smt_pipeline_run_batch_refined (include/smt_refine.h) puts region voting and outlier interpolation between :93 and
// :94 of the same tail: the arms of the pair's left image, recomputed on M by a third crossarm handle (caT), then
// smt_refine_batch on the pair's map.  The other two entry points launch what they launched.
// smt_pipeline_run_batch_filled (include/smt_fill_holes.h) has another tail at the same place: Sad.h's FillHolesInDispMap
// on the pair's map with the pair's class map (one launch), then the median.  It needs none of the tail's scratch.
#include "smt_common.h"
#include "../../include/smt_scan_views.h"
#include "../../include/smt_refine.h"
#include "../../include/smt_fill_holes.h"
#include <initializer_list>
#include <limits.h>
#include <new>
#include <stdlib.h>

struct smt_pipeline {
    int device;
    int H, W, D;
    smt_pipeline_params P;
    int sched;               // 0, 1, 2: see above
    int last_set;            // set of the last pair run (smt_pipeline_volumes)
    hipStream_t stream;      // M: the caller's stream
    hipStream_t side, front; // S, F
    hipEvent_t ev_in, ev_left, ev_front[2], ev_scan[2], ev_right[2];
    smt_adcensus *adc[2];
    smt_crossarm *caL, *caR;
    smt_scanline *so;
    float *Lf[2], *Rf[2];    // float copies of the pair in flight, per set
    float *agg[2], *sovol;   // aggregated left / right, scanline sum
    void *tail;              // speckle scratch of one pair (smt_speckle_scratch_bytes), first _post call
    int *tail_err;           // nonzero when a speckle kernel hit a loop cap; read and cleared by smt_pipeline_status
    // smt_pipeline_set_scan_views(SMT_VIEW_BOTH), all allocated by the first BOTH run (see "Both views" below)
    int scan_views;          // SMT_VIEW_LEFT (the default) or SMT_VIEW_BOTH
    unsigned quirks;         // what smt_pipeline_set_quirks / _set_subpixel were given, for soR
    float sub_min_den;
    smt_scanline *soR;       // schedules 1, 2: the right view's scanline handle, on S
    float *sovolR;           // the right view's scanline sum (the last pair's)
    bool sovolR_valid;
    hipEvent_t ev_aggR, ev_scanR[2];
    // smt_pipeline_run_batch_refined: the tail's own crossarm handle, on M, created by the first refined call.  A pair's
    // tail cannot read caL's maps: under schedules 0 to 2 and SMT_VIEW_BOTH they hold another image's arms by then.
    smt_crossarm *caT;
};

// main.cpp:93-94 on one pair, or nothing (post == NULL: smt_pipeline_run_batch)
struct pipe_tail {
    const smt_post_params *post;
    float *last;             // lastDisp [pairs][H][W], may be NULL
    // smt_pipeline_run_batch_refined: region voting and interpolation between :93 and :94, or nothing (refine == NULL)
    const smt_refine_params *refine;
    const uint8_t *grayL;    // the call's left images: the arms and the interpolation read pair b's
    uint8_t *state;          // [pairs][H][W], may be NULL
    int *status;             // [pairs][4], may be NULL
    // smt_pipeline_run_batch_filled: FillHolesInDispMap and the median instead of :93-94 (post == NULL), or nothing (0)
    int fill_wnd;            // the median's window, 1..7
    float fill_invalid;
};

SMT_API void smt_pipeline_default_params(smt_pipeline_params *p)
{
    if (!p) return;
    p->sigmaC = 10.0f; p->sigmaS = 30.0f;                 // main.cpp:25-26
    p->tao = 30; p->p1 = 10; p->p2 = 150; p->gate = 2;    // main.cpp:27-30
}

SMT_API void smt_post_default_params(smt_post_params *p)
{
    if (!p) return;
    p->speckle_diff = 1; p->speckle_min_area = 30;         // main.cpp:93
    p->speckle_invalid = INT_MIN;                          // int(Invalid_Float = +inf): x86's integer indefinite
    p->median_wnd = 3;                                     // main.cpp:94
}

SMT_API int smt_pipeline_destroy(smt_pipeline *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < 2; k++) {
        if (h->adc[k]) smt_adcensus_destroy(h->adc[k]);
        if (h->ev_front[k]) (void)hipEventDestroy(h->ev_front[k]);
        if (h->ev_scan[k]) (void)hipEventDestroy(h->ev_scan[k]);
        if (h->ev_right[k]) (void)hipEventDestroy(h->ev_right[k]);
        (void)hipFree(h->Lf[k]); (void)hipFree(h->Rf[k]);
        (void)hipFree(h->agg[k]);
    }
    if (h->caL) smt_crossarm_destroy(h->caL);
    if (h->caR) smt_crossarm_destroy(h->caR);
    if (h->caT) smt_crossarm_destroy(h->caT);
    if (h->so) smt_scanline_destroy(h->so);
    if (h->soR) smt_scanline_destroy(h->soR);
    (void)hipFree(h->sovolR);
    for (hipEvent_t e : {h->ev_aggR, h->ev_scanR[0], h->ev_scanR[1]})
        if (e) (void)hipEventDestroy(e);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_left) (void)hipEventDestroy(h->ev_left);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->front) (void)hipStreamDestroy(h->front);
    (void)hipFree(h->sovol);
    (void)hipFree(h->tail); (void)hipFree(h->tail_err);
    delete h;
    return SMT_OK;
}

static int pipeline_apply_streams(smt_pipeline *h)
{
    void *m = (void *)h->stream;
    int rc = smt_crossarm_set_stream(h->caL, m);
    if (rc == SMT_OK) rc = smt_scanline_set_stream(h->so, m);
    if (rc == SMT_OK && h->caR) rc = smt_crossarm_set_stream(h->caR, (void *)h->side);
    if (rc == SMT_OK && h->caT) rc = smt_crossarm_set_stream(h->caT, m);
    if (rc == SMT_OK && h->soR) rc = smt_scanline_set_stream(h->soR, (void *)h->side);
    for (int k = 0; k < 2 && rc == SMT_OK; k++)
        if (h->adc[k]) rc = smt_adcensus_set_stream(h->adc[k], h->sched == 2 ? (void *)h->front : m);
    return rc;
}

SMT_API int smt_pipeline_create(int H, int W, int D, const smt_pipeline_params *p, smt_pipeline **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    smt_pipeline *h = new (std::nothrow) smt_pipeline();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D;
    h->scan_views = SMT_VIEW_LEFT;
    if (p) h->P = *p; else smt_pipeline_default_params(&h->P);
    {
        const char *e = getenv("SMT_PIPE_SCHEDULE");
        h->sched = (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ? e[0] - '0' : 1;
    }
    const int nset = h->sched == 2 ? 2 : 1;
    const size_t N = (size_t)H * W, V = N * D;
    smt_crossarm_params cp;
    smt_crossarm_default_params(&cp);
    cp.tau = h->P.tao;
    int rc = SMT_OK;
    for (int k = 0; k < nset && rc == SMT_OK; k++) {
        rc = smt_adcensus_create(H, W, D, h->P.sigmaC, h->P.sigmaS, &h->adc[k]);
        if (rc == SMT_OK) rc = smt_malloc((void **)&h->Lf[k], N * 4);
        if (rc == SMT_OK) rc = smt_malloc((void **)&h->Rf[k], N * 4);
    }
    if (rc == SMT_OK) rc = smt_crossarm_create(H, W, D, &cp, &h->caL);
    if (rc == SMT_OK && h->sched >= 1) rc = smt_crossarm_create(H, W, D, &cp, &h->caR);
    if (rc == SMT_OK) rc = smt_scanline_create(H, W, D, h->P.p1, h->P.p2, &h->so);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->agg[0], V * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->agg[1], V * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->sovol, V * 4);
    if (rc == SMT_OK && hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess) rc = SMT_ERR_HIP;
    if (rc == SMT_OK && hipStreamCreateWithFlags(&h->front, hipStreamNonBlocking) != hipSuccess) rc = SMT_ERR_HIP;
    hipEvent_t *evs[] = {&h->ev_in, &h->ev_left, &h->ev_front[0], &h->ev_front[1], &h->ev_scan[0], &h->ev_scan[1],
                         &h->ev_right[0], &h->ev_right[1]};
    for (hipEvent_t *e : evs)
        if (rc == SMT_OK && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) rc = SMT_ERR_HIP;
    if (rc == SMT_OK) rc = pipeline_apply_streams(h);
    if (rc != SMT_OK) { smt_pipeline_destroy(h); return rc; }
    *out = h;
    return SMT_OK;
}

SMT_API int smt_pipeline_create_on(int device, int H, int W, int D, const smt_pipeline_params *p, smt_pipeline **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return smt_pipeline_create(H, W, D, p, out);
}

SMT_API int smt_pipeline_set_stream(smt_pipeline *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->stream = smt_stream(s);
    return pipeline_apply_streams(h);
}

SMT_API int smt_pipeline_set_quirks(smt_pipeline *h, unsigned quirks)
{
    if (!h || (quirks & ~SMT_QUIRK_FIX_ALL)) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    // every stage takes the flags it knows; handles a schedule does not use do not exist
    int rc = smt_crossarm_set_quirks_internal(h->caL, quirks);
    if (rc == SMT_OK && h->caR) rc = smt_crossarm_set_quirks_internal(h->caR, quirks);
    if (rc == SMT_OK && h->caT) rc = smt_crossarm_set_quirks_internal(h->caT, quirks);
    if (rc == SMT_OK) rc = smt_scanline_set_quirks(h->so, quirks);
    if (rc == SMT_OK && h->soR) rc = smt_scanline_set_quirks(h->soR, quirks);
    for (int k = 0; k < 2 && rc == SMT_OK; k++)
        if (h->adc[k]) rc = smt_adcensus_set_quirks(h->adc[k], quirks);
    if (rc == SMT_OK) h->quirks = quirks;
    return rc;
}

SMT_API int smt_pipeline_set_subpixel(smt_pipeline *h, const smt_subpixel_params *p)
{
    if (!h || (p && !spx_min_den_ok(p->min_den))) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    // the maps a run writes: dispL by the scanline handle, dispR by the right view's aggregation -- caR's where the
    // schedule has one, else caL's, whose left-view call asks for no map
    int rc = smt_scanline_set_subpixel(h->so, p);
    if (rc == SMT_OK) rc = smt_crossarm_set_subpixel(h->caL, p);
    if (rc == SMT_OK && h->caR) rc = smt_crossarm_set_subpixel(h->caR, p);
    if (rc == SMT_OK && h->soR) rc = smt_scanline_set_subpixel(h->soR, p);
    if (rc == SMT_OK) h->sub_min_den = p ? p->min_den : 0.0f;
    return rc;
}

#define PIPE_HIP(call) do { if (rc == SMT_OK && (call) != hipSuccess) rc = SMT_ERR_HIP; } while (0)

// main.cpp:93-94 for pair b, on M after its LR check
static int pipeline_tail(smt_pipeline *h, const pipe_tail &t, float *dl, const uint8_t *cls, int b)
{
    const int H = h->H, W = h->W;
    if (t.fill_wnd) {
        int rc = smt_fill_holes_batch(dl, cls, 1, 0, 0, H, W, t.fill_invalid, t.status ? t.status + 4 * b : nullptr,
                                      (void *)h->stream);
        if (rc == SMT_OK && t.last) rc = smt_median_filter(dl, t.last + (size_t)b * H * W, W, H, t.fill_wnd, (void *)h->stream);
        return rc;
    }
    if (!t.post) return SMT_OK;
    const smt_post_params &q = *t.post;
    int rc = smt_speckle_enqueue(dl, 1, 0, W, H, q.speckle_diff, q.speckle_min_area, q.speckle_invalid, h->tail,
                                 h->tail_err, h->stream);                                       // :93
    if (rc == SMT_OK && t.refine) {
        // the arms of this pair's left image (two launches), then voting and interpolation in place on dl
        const size_t N = (size_t)H * W;
        const uint8_t *L8 = t.grayL + b * N;
        int *arm[4] = {nullptr, nullptr, nullptr, nullptr};
        rc = smt_crossarm_arms(h->caT, L8, 1);
        if (rc == SMT_OK) rc = smt_crossarm_arm_maps(h->caT, &arm[0], &arm[1], &arm[2], &arm[3]);
        if (rc == SMT_OK)
            rc = smt_refine_batch(dl, 1, 0, arm[0], arm[1], arm[2], arm[3], 0, cls, 0, L8, 0, H, W, h->D, t.refine,
                                  t.state ? t.state + b * N : nullptr, 0, t.status ? t.status + 4 * b : nullptr,
                                  (void *)h->stream);
    }
    if (rc == SMT_OK && t.last) rc = smt_median_filter(dl, t.last + (size_t)b * H * W, W, H, q.median_wnd, (void *)h->stream);   // :94
    return rc;
}

// schedules 0 and 1: one set of front-end state, the left view's handle does both views
static int pipeline_run_simple(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                               float *dispR, uint8_t *cls, int *counts, const pipe_tail &tail)
{
    const int H = h->H, W = h->W;
    const size_t N = (size_t)H * W;
    void *st = (void *)h->stream;
    const bool two = h->sched == 1;
    if (two) {
        int rc = SMT_OK;
        PIPE_HIP(hipEventRecord(h->ev_in, h->stream));
        PIPE_HIP(hipStreamWaitEvent(h->side, h->ev_in, 0));                            // the caller's inputs, for the side stream
        if (rc != SMT_OK) return rc;
    }
    for (int b = 0; b < pairs; b++) {
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        float *dl = dispL + b * N, *dr = dispR + b * N;
        int rc = SMT_OK;
        if (two) {
            // both views' arms need only the images: on the side stream (the right view has its own handle), beside
            // this pair's AD-Census
            rc = smt_crossarm_set_stream(h->caL, (void *)h->side);
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                   // :67-72
            PIPE_HIP(hipEventRecord(h->ev_front[0], h->side));
            const int rc2 = smt_crossarm_set_stream(h->caL, st);
            if (rc == SMT_OK) rc = rc2;
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                   // :77-81 (its own Initialize: threshold reset)
        }
        if (rc == SMT_OK) rc = smt_u8_to_f32(L8, H, W, h->Lf[0], st);                   // main.cpp:46-55
        if (rc == SMT_OK) rc = smt_u8_to_f32(R8, H, W, h->Rf[0], st);
        if (rc == SMT_OK) rc = smt_adcensus_compute(h->adc[0], h->Lf[0], h->Rf[0], SMT_VIEW_BOTH, nullptr, nullptr);   // :57-61 (its WTA maps are overwritten at :75, :84)
        float *vol[2] = {nullptr, nullptr};
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[0], SMT_VIEW_LEFT, &vol[0]);
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[0], SMT_VIEW_RIGHT, &vol[1]);
        if (two) PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_front[0], 0));
        else if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                  // :67-72
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[0], h->agg[0], 0, nullptr);  // :73 (its WTA :75 is overwritten by :89)
        if (two) {
            PIPE_HIP(hipEventRecord(h->ev_left, h->stream));
            PIPE_HIP(hipStreamWaitEvent(h->side, h->ev_left, 0));
            if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caR, vol[1], h->agg[1], 0, dr);   // :82-84, beside the scanline
            PIPE_HIP(hipEventRecord(h->ev_right[0], h->side));
        } else {
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, R8, 1);                   // :77-81 (Initialize again: threshold reset)
            if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[1], h->agg[1], 0, dr);   // :82-84
        }
        if (rc == SMT_OK) rc = smt_scanline_run(h->so, h->agg[0], h->Lf[0], h->sovol, dl);     // :86-89
        if (two) PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_right[0], 0));
        if (rc == SMT_OK) rc = smt_lrcheck(dl, dr, H, W, h->P.gate, cls + b * N, counts ? counts + 2 * b : nullptr, st);   // :92
        if (rc == SMT_OK) rc = pipeline_tail(h, tail, dl, cls + b * N, b);                                   // :93-94
        if (rc != SMT_OK) { (void)hipStreamSynchronize(h->side); return rc; }
    }
    h->last_set = 0;
    return SMT_OK;
}

// ---- Both views (smt_pipeline_set_scan_views(SMT_VIEW_BOTH), include/smt_scan_views.h) -------------------------------
// dispR is the WTA of ScanLine(aggregated right volume, float right image); the right view's aggregation writes no map.
// The functions above are the LEFT flow and stay as they are; these are their BOTH twins.  A scanline pass is HBM and
// latency bound and belongs beside an aggregation (vector-issue bound, see the header of this file), so under schedules
// 1 and 2 the right view's scan goes on S behind the right view's aggregation, on a scanline handle of its own (soR),
// and runs beside the next pair's front end and left aggregation on M; M's LR check of pair b - 1 moves behind the
// scanline of pair b, which gives S that whole scan on top of the aggregation to finish.  Pairs before the last run
// the maps-only last pass (smt_scanline_run_map); the last pair stores its sum in sovolR (smt_pipeline_scan_right_volume).
// Edges on top of the LEFT flow's:
//   S: scan(right, b) --ev_scanR / ev_right[s]--> M: LR check of pair b     (not only aggregate(right, b))
//   schedule 1: S: aggregate(right, b) --ev_aggR--> M: AD-Census of pair b + 1; the one AD-Census set does not wait for
//               the scan.  The float right image does: it guides scan(right, b), so pairs alternate between Rf[0] and
//               Rf[1], and Rf[s] is rewritten by pair b + 2 on M behind the LR check of pair b.  S issues the arms of
//               pair b + 1 (which M's left aggregation waits for) BEFORE scan(right, b), else the scan would sit in
//               front of them and the aggregation beside it could not start.
//   schedule 2: ev_right[s] is recorded behind scan(right, b), so F's wait for set s covers Rf[s] too
//   agg[1]: aggregate(right, b) follows scan(right, b - 1) on S in every schedule
//   M: scan(left, b) --ev_scan[s]--> S: scan(right, b)     two scans side by side share HBM and gain nothing; measured,
//               DESIGN.md section 5.18, where the whole flow's figures are: under schedules 1 and 2 it is still dearer per
//               pair than a scan appended to the caller's stream
// Schedule 0: one smt_scanline_run_pair per pair on the caller's stream, both views in the same three launches.
static int pipeline_both_prepare(smt_pipeline *h)
{
    int rc = SMT_OK;
    if (!h->sovolR) rc = smt_malloc((void **)&h->sovolR, (size_t)h->H * h->W * h->D * 4);
    for (hipEvent_t *e : {&h->ev_aggR, &h->ev_scanR[0], &h->ev_scanR[1]})
        if (rc == SMT_OK && !*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) rc = SMT_ERR_HIP;
    if (rc == SMT_OK && h->sched >= 1 && !h->soR) {
        rc = smt_scanline_create(h->H, h->W, h->D, h->P.p1, h->P.p2, &h->soR);
        if (rc == SMT_OK) rc = smt_scanline_set_stream(h->soR, (void *)h->side);
        if (rc == SMT_OK) rc = smt_scanline_set_quirks(h->soR, h->quirks);
        smt_subpixel_params sp{h->sub_min_den};
        if (rc == SMT_OK) rc = smt_scanline_set_subpixel(h->soR, h->sub_min_den > 0.0f ? &sp : nullptr);
    }
    if (rc == SMT_OK && h->sched == 1 && !h->Rf[1]) rc = smt_malloc((void **)&h->Rf[1], (size_t)h->H * h->W * 4);
    return rc;
}

// S: the right view's scan of the pair whose float right image is Rf[s], into dr
static int pipeline_scan_right(smt_pipeline *h, int s, bool store, float *dr, hipEvent_t done)
{
    // not before M has finished the left view's scan of the same pair: two scans side by side share HBM and gain
    // nothing, so this one starts when M turns to the next pair's front end and left aggregation
    if (hipStreamWaitEvent(h->side, h->ev_scan[s], 0) != hipSuccess) return SMT_ERR_HIP;
    int rc = store ? smt_scanline_run(h->soR, h->agg[1], h->Rf[s], h->sovolR, dr)
                   : smt_scanline_run_map(h->soR, h->agg[1], h->Rf[s], dr);
    PIPE_HIP(hipEventRecord(done, h->side));
    return rc;
}

static int pipeline_run_simple_both(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                                    float *dispR, uint8_t *cls, int *counts, const pipe_tail &tail)
{
    const int H = h->H, W = h->W;
    const size_t N = (size_t)H * W;
    void *st = (void *)h->stream;
    const bool two = h->sched == 1;
    int rc = SMT_OK;
    if (two) {
        PIPE_HIP(hipEventRecord(h->ev_in, h->stream));
        PIPE_HIP(hipStreamWaitEvent(h->side, h->ev_in, 0));
    }
    for (int b = 0; b < pairs && rc == SMT_OK; b++) {
        const int s = two ? (b & 1) : 0;
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        float *dl = dispL + b * N, *dr = dispR + b * N;
        if (two) {
            rc = smt_crossarm_set_stream(h->caL, (void *)h->side);
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                   // :67-72
            PIPE_HIP(hipEventRecord(h->ev_front[0], h->side));
            const int rc2 = smt_crossarm_set_stream(h->caL, st);
            if (rc == SMT_OK) rc = rc2;
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                   // :77-81
            if (rc == SMT_OK && b >= 1)                                                 // beside this pair's AD-Census and left aggregation
                rc = pipeline_scan_right(h, s ^ 1, false, dr - N, h->ev_scanR[s ^ 1]);
        }
        if (rc == SMT_OK) rc = smt_u8_to_f32(L8, H, W, h->Lf[0], st);                   // main.cpp:46-55
        if (rc == SMT_OK) rc = smt_u8_to_f32(R8, H, W, h->Rf[s], st);
        if (two && b >= 1) PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_aggR, 0));    // aggregate(right, b - 1) read the volumes
        if (rc == SMT_OK) rc = smt_adcensus_compute(h->adc[0], h->Lf[0], h->Rf[s], SMT_VIEW_BOTH, nullptr, nullptr);   // :57-61
        float *vol[2] = {nullptr, nullptr};
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[0], SMT_VIEW_LEFT, &vol[0]);
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[0], SMT_VIEW_RIGHT, &vol[1]);
        if (two) PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_front[0], 0));
        else if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                  // :67-72
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[0], h->agg[0], 0, nullptr);  // :73
        if (two) {
            PIPE_HIP(hipEventRecord(h->ev_left, h->stream));
            PIPE_HIP(hipStreamWaitEvent(h->side, h->ev_left, 0));
            if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caR, vol[1], h->agg[1], 0, nullptr);   // :82-83, beside the scanline
            PIPE_HIP(hipEventRecord(h->ev_aggR, h->side));
            if (rc == SMT_OK) rc = smt_scanline_run(h->so, h->agg[0], h->Lf[0], h->sovol, dl);     // :86-89
            PIPE_HIP(hipEventRecord(h->ev_scan[s], h->stream));
            if (b >= 1) {                                                                           // :92 of pair b - 1
                PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_scanR[s ^ 1], 0));
                if (rc == SMT_OK)
                    rc = smt_lrcheck(dl - N, dr - N, H, W, h->P.gate, cls + (b - 1) * N, counts ? counts + 2 * (b - 1) : nullptr, st);
                if (rc == SMT_OK) rc = pipeline_tail(h, tail, dl - N, cls + (b - 1) * N, b - 1);
            }
        } else {
            if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, R8, 1);                   // :77-81
            if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[1], h->agg[1], 0, nullptr);   // :82-83
            if (rc == SMT_OK)                                                           // :86-89 on both views
                rc = smt_scanline_run_pair(h->so, h->agg[0], h->Lf[0], h->sovol, dl, h->agg[1], h->Rf[0],
                                           b == pairs - 1 ? h->sovolR : nullptr, dr);
            if (rc == SMT_OK) rc = smt_lrcheck(dl, dr, H, W, h->P.gate, cls + b * N, counts ? counts + 2 * b : nullptr, st);   // :92
            if (rc == SMT_OK) rc = pipeline_tail(h, tail, dl, cls + b * N, b);                       // :93-94
        }
    }
    if (two && rc == SMT_OK) {
        const int b = pairs - 1, s = b & 1;
        rc = pipeline_scan_right(h, s, true, dispR + b * N, h->ev_scanR[s]);
        PIPE_HIP(hipStreamWaitEvent(h->stream, h->ev_scanR[s], 0));
        if (rc == SMT_OK)
            rc = smt_lrcheck(dispL + b * N, dispR + b * N, H, W, h->P.gate, cls + b * N, counts ? counts + 2 * b : nullptr, st);
        if (rc == SMT_OK) rc = pipeline_tail(h, tail, dispL + b * N, cls + b * N, b);
    }
    if (rc != SMT_OK) { (void)hipStreamSynchronize(h->side); return rc; }
    h->last_set = 0;
    return SMT_OK;
}

static int pipeline_run_both(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                             float *dispR, uint8_t *cls, int *counts, const pipe_tail &tail)
{
    int rc = pipeline_both_prepare(h);
    if (rc != SMT_OK) return rc;
    h->sovolR_valid = false;
    if (h->sched != 2) {
        rc = pipeline_run_simple_both(h, grayL, grayR, pairs, dispL, dispR, cls, counts, tail);
        h->sovolR_valid = rc == SMT_OK;
        return rc;
    }
    const int H = h->H, W = h->W;
    const size_t N = (size_t)H * W;
    hipStream_t M = h->stream, S = h->side, F = h->front;
    PIPE_HIP(hipEventRecord(h->ev_in, M));
    PIPE_HIP(hipStreamWaitEvent(F, h->ev_in, 0));
    for (int b = 0; b < pairs && rc == SMT_OK; b++) {
        const int s = b & 1;
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        float *dl = dispL + b * N, *dr = dispR + b * N;
        // F: front end of pair b into set s
        if (b >= 2) {
            PIPE_HIP(hipStreamWaitEvent(F, h->ev_scan[s], 0));     // scanline(left, b-2) read Lf[s]; aggregate(left, b-2) read the volumes
            PIPE_HIP(hipStreamWaitEvent(F, h->ev_right[s], 0));    // scan(right, b-2) read Rf[s]; aggregate(right, b-2) read the volumes
        }
        if (rc == SMT_OK) rc = smt_u8_to_f32(L8, H, W, h->Lf[s], (void *)F);                   // main.cpp:46-55
        if (rc == SMT_OK) rc = smt_u8_to_f32(R8, H, W, h->Rf[s], (void *)F);
        if (rc == SMT_OK) rc = smt_adcensus_compute(h->adc[s], h->Lf[s], h->Rf[s], SMT_VIEW_BOTH, nullptr, nullptr);   // :57-61
        PIPE_HIP(hipEventRecord(h->ev_front[s], F));
        float *vol[2] = {nullptr, nullptr};
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[s], SMT_VIEW_LEFT, &vol[0]);
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[s], SMT_VIEW_RIGHT, &vol[1]);
        // M: left view
        PIPE_HIP(hipStreamWaitEvent(M, h->ev_front[s], 0));
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                               // :67-72
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[0], h->agg[0], 0, nullptr);  // :73
        PIPE_HIP(hipEventRecord(h->ev_left, M));
        if (rc == SMT_OK) rc = smt_scanline_run(h->so, h->agg[0], h->Lf[s], h->sovol, dl);     // :86-89
        PIPE_HIP(hipEventRecord(h->ev_scan[s], M));
        if (b >= 1) {                                                                           // :92 of pair b - 1
            PIPE_HIP(hipStreamWaitEvent(M, h->ev_right[s ^ 1], 0));
            if (rc == SMT_OK)
                rc = smt_lrcheck(dl - N, dr - N, H, W, h->P.gate, cls + (b - 1) * N, counts ? counts + 2 * (b - 1) : nullptr, (void *)M);
            if (rc == SMT_OK) rc = pipeline_tail(h, tail, dl - N, cls + (b - 1) * N, b - 1);                     // :93-94 of pair b - 1
        }
        // S: right view: aggregation beside the left view's scanline, scan beside the next pair's left aggregation
        PIPE_HIP(hipStreamWaitEvent(S, h->ev_left, 0));
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                               // :77-81
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caR, vol[1], h->agg[1], 0, nullptr);  // :82-83
        if (rc == SMT_OK) rc = pipeline_scan_right(h, s, b == pairs - 1, dr, h->ev_right[s]);
    }
    if (rc == SMT_OK) {
        const int b = pairs - 1, s = b & 1;
        PIPE_HIP(hipStreamWaitEvent(M, h->ev_right[s], 0));
        if (rc == SMT_OK)
            rc = smt_lrcheck(dispL + b * N, dispR + b * N, H, W, h->P.gate, cls + b * N, counts ? counts + 2 * b : nullptr, (void *)M);
        if (rc == SMT_OK) rc = pipeline_tail(h, tail, dispL + b * N, cls + b * N, b);
        h->last_set = s;
    }
    if (rc != SMT_OK) { (void)hipStreamSynchronize(S); (void)hipStreamSynchronize(F); }
    h->sovolR_valid = rc == SMT_OK;
    return rc;
}

SMT_API int smt_pipeline_set_scan_views(smt_pipeline *h, int views)
{
    if (!h || (views != SMT_VIEW_LEFT && views != SMT_VIEW_BOTH)) return SMT_ERR_ARG;
    h->scan_views = views;
    return SMT_OK;
}

SMT_API int smt_pipeline_scan_right_volume(smt_pipeline *h, float **sum)
{
    if (!h || !sum) return SMT_ERR_ARG;
    if (!h->sovolR_valid) return SMT_ERR_STATE;
    *sum = h->sovolR;
    return SMT_OK;
}

static int pipeline_run(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                        float *dispR, uint8_t *cls, int *counts, const pipe_tail &tail)
{
    if (h->scan_views == SMT_VIEW_BOTH) return pipeline_run_both(h, grayL, grayR, pairs, dispL, dispR, cls, counts, tail);
    if (h->sched != 2) return pipeline_run_simple(h, grayL, grayR, pairs, dispL, dispR, cls, counts, tail);
    const int H = h->H, W = h->W;
    const size_t N = (size_t)H * W;
    hipStream_t M = h->stream, S = h->side, F = h->front;
    int rc = SMT_OK;
    PIPE_HIP(hipEventRecord(h->ev_in, M));
    PIPE_HIP(hipStreamWaitEvent(F, h->ev_in, 0));
    for (int b = 0; b < pairs && rc == SMT_OK; b++) {
        const int s = b & 1;
        const uint8_t *L8 = grayL + b * N, *R8 = grayR + b * N;
        float *dl = dispL + b * N, *dr = dispR + b * N;
        // F: front end of pair b into set s
        if (b >= 2) {
            PIPE_HIP(hipStreamWaitEvent(F, h->ev_scan[s], 0));     // scanline(b-2) read Lf[s]; aggregate(left, b-2) read the volumes
            PIPE_HIP(hipStreamWaitEvent(F, h->ev_right[s], 0));    // aggregate(right, b-2) read the volumes
        }
        if (rc == SMT_OK) rc = smt_u8_to_f32(L8, H, W, h->Lf[s], (void *)F);                   // main.cpp:46-55
        if (rc == SMT_OK) rc = smt_u8_to_f32(R8, H, W, h->Rf[s], (void *)F);
        if (rc == SMT_OK) rc = smt_adcensus_compute(h->adc[s], h->Lf[s], h->Rf[s], SMT_VIEW_BOTH, nullptr, nullptr);   // :57-61
        PIPE_HIP(hipEventRecord(h->ev_front[s], F));
        float *vol[2] = {nullptr, nullptr};
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[s], SMT_VIEW_LEFT, &vol[0]);
        if (rc == SMT_OK) rc = smt_adcensus_volume(h->adc[s], SMT_VIEW_RIGHT, &vol[1]);
        // M: left view
        PIPE_HIP(hipStreamWaitEvent(M, h->ev_front[s], 0));
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caL, L8, 1);                               // :67-72
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caL, vol[0], h->agg[0], 0, nullptr);  // :73 (its WTA :75 is overwritten by :89)
        PIPE_HIP(hipEventRecord(h->ev_left, M));
        if (b >= 1) {                                                                           // :92 of pair b - 1
            PIPE_HIP(hipStreamWaitEvent(M, h->ev_right[s ^ 1], 0));
            if (rc == SMT_OK)
                rc = smt_lrcheck(dl - N, dr - N, H, W, h->P.gate, cls + (b - 1) * N, counts ? counts + 2 * (b - 1) : nullptr, (void *)M);
            if (rc == SMT_OK) rc = pipeline_tail(h, tail, dl - N, cls + (b - 1) * N, b - 1);                     // :93-94 of pair b - 1
        }
        if (rc == SMT_OK) rc = smt_scanline_run(h->so, h->agg[0], h->Lf[s], h->sovol, dl);     // :86-89
        PIPE_HIP(hipEventRecord(h->ev_scan[s], M));
        // S: right view, beside the scanline passes
        PIPE_HIP(hipStreamWaitEvent(S, h->ev_left, 0));
        if (rc == SMT_OK) rc = smt_crossarm_arms(h->caR, R8, 1);                               // :77-81
        if (rc == SMT_OK) rc = smt_crossarm_aggregate(h->caR, vol[1], h->agg[1], 0, dr);       // :82-84
        PIPE_HIP(hipEventRecord(h->ev_right[s], S));
    }
    if (rc == SMT_OK) {
        const int b = pairs - 1, s = b & 1;
        PIPE_HIP(hipStreamWaitEvent(M, h->ev_right[s], 0));
        if (rc == SMT_OK)
            rc = smt_lrcheck(dispL + b * N, dispR + b * N, H, W, h->P.gate, cls + b * N, counts ? counts + 2 * b : nullptr, (void *)M);
        if (rc == SMT_OK) rc = pipeline_tail(h, tail, dispL + b * N, cls + b * N, b);
        h->last_set = s;
    }
    if (rc != SMT_OK) { (void)hipStreamSynchronize(S); (void)hipStreamSynchronize(F); }
    return rc;
}

SMT_API int smt_pipeline_run_batch(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                   float *dispL, float *dispR, uint8_t *cls, int *counts)
{
    if (!h || !grayL || !grayR || pairs <= 0 || !dispL || !dispR || !cls) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    return pipeline_run(h, grayL, grayR, pairs, dispL, dispR, cls, counts, pipe_tail{nullptr, nullptr});
}

// the tail's scratch, allocated by the first call that has a tail
static int pipeline_tail_prepare(smt_pipeline *h)
{
    if (h->tail) return SMT_OK;
    int rc = smt_malloc(&h->tail, smt_speckle_scratch_bytes(1, h->W, h->H));
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->tail_err, 4);
    if (rc == SMT_OK && hipMemsetAsync(h->tail_err, 0, 4, h->stream) != hipSuccess) rc = SMT_ERR_HIP;
    if (rc != SMT_OK) { (void)hipFree(h->tail); (void)hipFree(h->tail_err); h->tail = nullptr; h->tail_err = nullptr; }
    return rc;
}

SMT_API int smt_pipeline_run_batch_post(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                        float *dispL, float *dispR, uint8_t *cls, int *counts,
                                        const smt_post_params *post, float *lastDisp)
{
    if (!h || !grayL || !grayR || pairs <= 0 || !dispL || !dispR || !cls || !post) return SMT_ERR_ARG;
    if (post->median_wnd < 1 || post->median_wnd > 7 || lastDisp == dispL) return SMT_ERR_ARG;
    if ((long long)h->H * h->W >= (1ll << 31)) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int rc = pipeline_tail_prepare(h);
    if (rc != SMT_OK) return rc;
    return pipeline_run(h, grayL, grayR, pairs, dispL, dispR, cls, counts, pipe_tail{post, lastDisp});
}

SMT_API int smt_pipeline_run_batch_refined(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                           float *dispL, float *dispR, uint8_t *cls, int *counts,
                                           const smt_post_params *post, const smt_refine_params *refine, float *lastDisp,
                                           uint8_t *state, int *status)
{
    if (!h || !grayL || !grayR || pairs <= 0 || !dispL || !dispR || !cls || !post) return SMT_ERR_ARG;
    if (post->median_wnd < 1 || post->median_wnd > 7 || lastDisp == dispL) return SMT_ERR_ARG;
    if ((long long)h->H * h->W >= (1ll << 31)) return SMT_ERR_ARG;
    smt_refine_params rp;
    if (refine) rp = *refine; else smt_refine_default_params(&rp);
    if (rp.irv_iters < 0 || rp.irv_iters > 16 || rp.search < 0) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    int rc = pipeline_tail_prepare(h);
    if (rc == SMT_OK && !h->caT) {
        smt_crossarm_params cp;
        smt_crossarm_default_params(&cp);
        cp.tau = h->P.tao;
        rc = smt_crossarm_create(h->H, h->W, h->D, &cp, &h->caT);
        if (rc == SMT_OK) rc = smt_crossarm_set_quirks_internal(h->caT, h->quirks);
        if (rc == SMT_OK) rc = smt_crossarm_set_stream(h->caT, (void *)h->stream);
        if (rc != SMT_OK && h->caT) { smt_crossarm_destroy(h->caT); h->caT = nullptr; }
    }
    if (rc != SMT_OK) return rc;
    return pipeline_run(h, grayL, grayR, pairs, dispL, dispR, cls, counts, pipe_tail{post, lastDisp, &rp, grayL, state, status});
}

SMT_API int smt_pipeline_run_batch_filled(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                          float *dispL, float *dispR, uint8_t *cls, int *counts, int median_wnd,
                                          float invalid, float *lastDisp, int *status)
{
    if (!h || !grayL || !grayR || pairs <= 0 || !dispL || !dispR || !cls) return SMT_ERR_ARG;
    if (median_wnd < 1 || median_wnd > 7 || lastDisp == dispL || invalid != invalid) return SMT_ERR_ARG;
    if (h->H > SMT_FILLHOLES_MAX_DIM || h->W > SMT_FILLHOLES_MAX_DIM) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    return pipeline_run(h, grayL, grayR, pairs, dispL, dispR, cls, counts,
                        pipe_tail{nullptr, lastDisp, nullptr, nullptr, nullptr, status, median_wnd, invalid});
}

SMT_API int smt_pipeline_volumes(smt_pipeline *h, float **cost_left, float **cost_right, float **agg_left, float **agg_right,
                                 float **scanline_sum)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    int rc = SMT_OK;
    smt_adcensus *a = h->adc[h->last_set];
    if (cost_left) rc = smt_adcensus_volume(a, SMT_VIEW_LEFT, cost_left);
    if (rc == SMT_OK && cost_right) rc = smt_adcensus_volume(a, SMT_VIEW_RIGHT, cost_right);
    if (agg_left) *agg_left = h->agg[0];
    if (agg_right) *agg_right = h->agg[1];
    if (scanline_sum) *scanline_sum = h->sovol;
    return rc;
}

SMT_API int smt_pipeline_status(smt_pipeline *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipStreamSynchronize(h->stream);               // everything of the last call is ordered on the caller's stream
    int rc = SMT_OK;
    for (int k = 0; k < 2; k++)
        if (h->adc[k]) { const int a = smt_adcensus_status(h->adc[k]); if (rc == SMT_OK) rc = a; }
    { const int c = smt_crossarm_status(h->caL); if (rc == SMT_OK) rc = c; }
    if (h->caR) { const int c = smt_crossarm_status(h->caR); if (rc == SMT_OK) rc = c; }
    if (h->tail_err) {                                   // a speckle kernel of a _post call hit a loop cap
        int e = 0;
        if (hipMemcpy(&e, h->tail_err, 4, hipMemcpyDeviceToHost) != hipSuccess) e = 1;
        if (e) { (void)hipMemset(h->tail_err, 0, 4); if (rc == SMT_OK) rc = SMT_ERR_STATE; }
    }
    return rc;
}
