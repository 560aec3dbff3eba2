// smt_asw_flow_*: the active lines of ASW/ASWeight.cpp for a batch of gray pairs, on the device.
//   :54-55  copyMakeBorder(gray, winSize + 1, BORDER_REPLICATE) of both images     smt_pad_replicate
//   :60-61  AdaptiveSupportWeight, AdaptiveSupportWeightRight                      smt_asw_both (one pass over the hypotheses)
//   :66     CrossCheckDiaparity                                                    smt_asw_crosscheck
//   :67-78  normalize, convertTo, filterSpeckles, medianBlur, FillImageNew         smt_asw_flow_run_batch_post (asw_tail.hip)
// smt_asw_flow_run_batch stops at :66; smt_asw_flow_run_batch_post reaches the end of the file.
// The handle owns the two masks (smt_asw_masks on the host, uploaded once), the padded images and one pair of maps, so
// a warm call allocates nothing beyond the scratch arena of smt_asw.
#include "smt_common.h"
#include <new>
#include <vector>

struct smt_asw_flow {
    int device;
    int H, W, D;
    smt_asw_params P;
    hipStream_t stream;
    double *space, *color;    // (2 winSize + 3)^2 and 256 doubles
    uint8_t *padL, *padR;     // [H + 2 wins][W + 2 wins]
    float *mapL, *mapR;       // maps of the current pair where the caller passes no buffer
    int *post_err;            // loop-cap flag of run_batch_post's speckle kernels (smt_asw_flow_status)
};

SMT_API void smt_asw_default_params(smt_asw_params *p)
{
    if (!p) return;
    p->winSize = 11; p->T = 40; p->sigma_space = 50.0; p->sigma_color = 30.0;      // ASWeight.cpp:43-47
}

SMT_API int smt_asw_flow_destroy(smt_asw_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->space); (void)hipFree(h->color);
    (void)hipFree(h->padL); (void)hipFree(h->padR);
    (void)hipFree(h->mapL); (void)hipFree(h->mapR);
    (void)hipFree(h->post_err);
    delete h;
    return SMT_OK;
}

static int asw_flow_create(int H, int W, int D, const smt_asw_params *p, smt_asw_flow **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    if ((long long)H * W > (1ll << 28)) return SMT_ERR_ARG;               // pixel indices are int
    smt_asw_params P;
    if (p) P = *p; else smt_asw_default_params(&P);
    if (P.winSize < 1 || P.winSize > 30 || !(P.sigma_space > 0.0) || !(P.sigma_color > 0.0)) return SMT_ERR_ARG;
    smt_asw_flow *h = new (std::nothrow) smt_asw_flow();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->P = P;
    const int side = 2 * P.winSize + 3, wins = P.winSize + 1;
    const size_t np = (size_t)(H + 2 * wins) * (W + 2 * wins), N = (size_t)H * W;
    std::vector<double> sp((size_t)side * side), cm(256);
    int rc = smt_asw_masks(P.winSize, P.sigma_space, P.sigma_color, sp.data(), cm.data());
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->space, sp.size() * 8);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->color, cm.size() * 8);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->padL, np);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->padR, np);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->mapL, N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->mapR, N * 4);
    if (rc == SMT_OK) rc = smt_malloc((void **)&h->post_err, 4);
    if (rc == SMT_OK && hipMemset(h->post_err, 0, 4) != hipSuccess) rc = SMT_ERR_HIP;
    if (rc == SMT_OK && (hipMemcpy(h->space, sp.data(), sp.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
                         hipMemcpy(h->color, cm.data(), cm.size() * 8, hipMemcpyHostToDevice) != hipSuccess))
        rc = SMT_ERR_HIP;
    if (rc != SMT_OK) { smt_asw_flow_destroy(h); return rc; }
    *out = h;
    return SMT_OK;
}

SMT_API int smt_asw_flow_create_on(int device, int H, int W, int D, const smt_asw_params *p, smt_asw_flow **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return asw_flow_create(H, W, D, p, out);
}

SMT_API int smt_asw_flow_set_stream(smt_asw_flow *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_asw_flow_run_batch(smt_asw_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                   float *dispL, float *dispR, uint8_t *lastDisp)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int H = h->H, W = h->W, wins = h->P.winSize + 1;
    const size_t N = (size_t)H * W;
    void *st = (void *)h->stream;
    for (int b = 0; b < pairs; b++) {
        float *dl = dispL ? dispL + b * N : h->mapL, *dr = dispR ? dispR + b * N : h->mapR;
        int rc = smt_pad_replicate(grayL + b * N, H, W, wins, h->padL, st);                          // ASWeight.cpp:54
        if (rc == SMT_OK) rc = smt_pad_replicate(grayR + b * N, H, W, wins, h->padR, st);            // :55
        if (rc == SMT_OK) rc = smt_asw_both(h->padL, h->padR, H, W, h->D, h->P.winSize, h->space, h->color, h->P.T,
                                            dl, dr, nullptr, nullptr, st);                           // :60-61
        if (rc == SMT_OK && lastDisp) rc = smt_asw_crosscheck(dl, dr, H, W, lastDisp + b * N, st);   // :66
        if (rc != SMT_OK) return rc;
    }
    return SMT_OK;
}

// run_batch for all pairs, then the file's tail: :67-68 + :70-71 per requested view, :69 + :72-78 once over the batch
SMT_API int smt_asw_flow_run_batch_post(smt_asw_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                                        float *dispR, uint8_t *lastDisp, uint8_t *dispL8, uint8_t *dispR8,
                                        const smt_asw_post_params *post, uint8_t *after_median, uint8_t *after_fill,
                                        int *fill_counts)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!grayL || !grayR || !lastDisp || (dispL8 && !dispL) || (dispR8 && !dispR)) return SMT_ERR_ARG;
    if (h->W > 65535 || (long long)h->H * h->W >= (1ll << 28)) return SMT_ERR_ARG;
    if (post && ((post->median_first != 3 && post->median_first != 5) || (post->median_last != 3 && post->median_last != 5) ||
                 (post->fix & ~(unsigned)SMT_ASW_FIX_FILL_ROW_END)))
        return SMT_ERR_ARG;
    int rc = smt_asw_flow_run_batch(h, grayL, grayR, pairs, dispL, dispR, lastDisp);
    if (rc != SMT_OK) return rc;
    smt_dev_guard dev_guard(h->device);
    void *st = (void *)h->stream;
    if (dispL8) rc = smt_minmax_normalize_f32_u8_batch(dispL, dispL8, pairs, 0, h->H, h->W, st);             // :67, :70
    if (rc == SMT_OK && dispR8) rc = smt_minmax_normalize_f32_u8_batch(dispR, dispR8, pairs, 0, h->H, h->W, st);   // :68, :71
    if (rc != SMT_OK) return rc;
    return smt_asw_tail_batch(lastDisp, pairs, 0, h->H, h->W, post, after_median, after_fill, fill_counts, h->post_err, st);
}

SMT_API int smt_asw_flow_status(smt_asw_flow *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return SMT_ERR_HIP;
    int e = 0;
    if (hipMemcpy(&e, h->post_err, 4, hipMemcpyDeviceToHost) != hipSuccess) e = 1;
    if (e) { (void)hipMemset(h->post_err, 0, 4); return SMT_ERR_STATE; }
    return SMT_OK;
}
