// Host-only contract stub of the entries of include/smt.h that host/smt_host.hpp calls.  No HIP.
//
// It computes nothing and is not an oracle.  "Device" memory is malloc'ed with the exact byte count, so under
// AddressSanitizer a mirror that sizes a device buffer wrongly, or copies more than a buffer holds, faults here.  Every
// compute entry (1) rejects what smt.h says it rejects, (2) reads every byte of every input extent the header grants
// it, (3) fills every output extent with stub_pattern(entry, k).  Extents come from the comments of smt.h alone.
#include "smt_contract_stub.hpp"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>

#include "../../include/smt.h"

namespace {

std::vector<StubCall> g_log;
std::map<std::string, int> g_fail;
std::map<std::string, int> g_flag;
int g_handles = 0, g_allocs = 0, g_streams = 0;
volatile unsigned g_sink = 0;

// returns true when the call has to fail with *rc
bool enter(const char *entry, std::initializer_list<long long> args, int *rc)
{
    g_log.push_back(StubCall{entry, std::vector<long long>(args)});
    auto it = g_fail.find(entry);
    if (it == g_fail.end()) return false;
    *rc = it->second;
    g_fail.erase(it);
    return true;
}
bool flagged(const char *entry)
{
    auto it = g_flag.find(entry);
    if (it == g_flag.end()) return false;
    g_flag.erase(it);
    return true;
}
#define ENTER(...)                                      \
    do {                                                \
        int rc_ = 0;                                    \
        if (enter(__func__, {__VA_ARGS__}, &rc_)) return rc_; \
    } while (0)

void rd(const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    unsigned s = 0;
    for (size_t i = 0; i < bytes; i++) s += b[i];
    g_sink = g_sink + s;
}
void wr(void *p, size_t bytes, const char *entry, int k) { if (bytes) memset(p, stub_pattern(entry, k), bytes); }
void wr_opt(void *p, size_t bytes, const char *entry, int k) { if (p) wr(p, bytes, entry, k); }
void wr_cls(uint8_t *cls, size_t n) { for (size_t i = 0; i < n; i++) cls[i] = (uint8_t)(i % 3); }

struct Handle {
    int H = 0, W = 0, D = 0, aux = 0;
    void *own[4] = {nullptr, nullptr, nullptr, nullptr};   // buffers the library lends
};
Handle *new_handle(int H, int W, int D, int aux = 0)
{
    Handle *h = new Handle;
    h->H = H; h->W = W; h->D = D; h->aux = aux;
    g_handles++;
    return h;
}
int del_handle(void *p)
{
    if (!p) return SMT_ERR_ARG;
    Handle *h = static_cast<Handle *>(p);
    for (void *q : h->own) free(q);
    delete h;
    g_handles--;
    return SMT_OK;
}
size_t px(const Handle *h) { return (size_t)h->H * h->W; }
size_t padded(int H, int W, int win) { const int w = win + 1; return (size_t)(H + 2 * w) * (W + 2 * w); }
bool bad_size(int H, int W) { return H <= 0 || W <= 0; }
bool bad_D(int D) { return D < 1 || D > SMT_MAX_DISPARITY; }
bool bad_quirks(unsigned q) { return (q & ~SMT_QUIRK_FIX_ALL) != 0; }
bool bad_sub(const smt_subpixel_params *p) { return p && !(p->min_den > 0.0f && p->min_den < 3.0e38f); }

}  // namespace

const std::vector<StubCall> &stub_log() { return g_log; }
void stub_log_clear() { g_log.clear(); }
void stub_fail(const char *entry, int rc) { g_fail[entry] = rc; }
void stub_flag(const char *entry) { g_flag[entry] = 1; }
unsigned char stub_pattern(const char *entry, int k)
{
    unsigned h = 2166136261u;
    for (const char *c = entry; *c; c++) h = (h ^ (unsigned char)*c) * 16777619u;
    return (unsigned char)(1 + (h + 41u * (unsigned)k) % 200u);
}
int stub_live_handles() { return g_handles; }
int stub_live_allocs() { return g_allocs; }
int stub_live_streams() { return g_streams; }

extern "C" {

const char *smt_strerror(int status)
{
    switch (status) {
    case SMT_OK: return "ok";
    case SMT_ERR_ARG: return "bad argument";
    case SMT_ERR_HIP: return "HIP error";
    case SMT_ERR_ALLOC: return "allocation failed";
    case SMT_ERR_DOMAIN: return "domain";
    case SMT_ERR_REF_UB: return "reference UB";
    case SMT_ERR_STATE: return "state";
    }
    return "unknown";
}
int smt_device_count(int *count) { ENTER(); if (!count) return SMT_ERR_ARG; *count = 2; return SMT_OK; }
int smt_set_device(int device) { ENTER(device); return device < 0 || device >= 2 ? SMT_ERR_ARG : SMT_OK; }

// ---- plumbing
int smt_malloc(void **dptr, size_t bytes)
{
    ENTER((long long)bytes);
    if (!dptr) return SMT_ERR_ARG;
    if (bytes > ((size_t)1 << 30)) return SMT_ERR_ALLOC;
    *dptr = malloc(bytes);          // exact: the redzone starts right behind the last byte asked for
    if (!*dptr) return SMT_ERR_ALLOC;
    memset(*dptr, 0xCD, bytes);
    g_allocs++;
    return SMT_OK;
}
int smt_free(void *dptr) { ENTER(); if (dptr) { free(dptr); g_allocs--; } return SMT_OK; }
int smt_memcpy_h2d(void *d, const void *s, size_t n, void *) { ENTER((long long)n); if (n) memcpy(d, s, n); return SMT_OK; }
int smt_memcpy_d2h(void *d, const void *s, size_t n, void *) { ENTER((long long)n); if (n) memcpy(d, s, n); return SMT_OK; }
int smt_memset(void *d, int b, size_t n, void *) { ENTER(b, (long long)n); if (n) memset(d, b, n); return SMT_OK; }
int smt_stream_create(void **stream)
{
    ENTER();
    if (!stream) return SMT_ERR_ARG;
    *stream = malloc(1);
    g_streams++;
    return SMT_OK;
}
int smt_stream_destroy(void *stream) { ENTER(); if (stream) { free(stream); g_streams--; } return SMT_OK; }
int smt_stream_sync(void *) { ENTER(); return SMT_OK; }

// ---- AD-Census
static int adc_create(int H, int W, int D, smt_adcensus **out)
{
    if (!out || bad_size(H, W) || bad_D(D)) return SMT_ERR_ARG;
    Handle *h = new_handle(H, W, D);
    for (int v = 0; v < 2; v++) {
        h->own[v] = malloc(px(h) * D * sizeof(float));
        memset(h->own[v], 0xCD, px(h) * D * sizeof(float));
    }
    *out = reinterpret_cast<smt_adcensus *>(h);
    return SMT_OK;
}
int smt_adcensus_create(int H, int W, int D, float, float, smt_adcensus **out) { ENTER(H, W, D); return adc_create(H, W, D, out); }
int smt_adcensus_create_on(int device, int H, int W, int D, float, float, smt_adcensus **out)
{
    ENTER(device, H, W, D);
    if (device < 0 || device >= 2) return SMT_ERR_ARG;
    return adc_create(H, W, D, out);
}
int smt_adcensus_destroy(smt_adcensus *h) { ENTER(); return del_handle(h); }
int smt_adcensus_set_stream(smt_adcensus *h, void *) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }
int smt_adcensus_set_quirks(smt_adcensus *h, unsigned quirks) { ENTER(quirks); return !h || bad_quirks(quirks) ? SMT_ERR_ARG : SMT_OK; }
int smt_adcensus_compute(smt_adcensus *hh, const float *L, const float *R, int views, float *dispL, float *dispR)
{
    ENTER(views);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || views < 1 || views > 3) return SMT_ERR_ARG;
    rd(L, px(h) * 4); rd(R, px(h) * 4);
    if (views & SMT_VIEW_LEFT) wr(h->own[0], px(h) * h->D * 4, __func__, 2);
    if (views & SMT_VIEW_RIGHT) wr(h->own[1], px(h) * h->D * 4, __func__, 3);
    wr_opt(dispL, px(h) * 4, __func__, 0); wr_opt(dispR, px(h) * 4, __func__, 1);
    return SMT_OK;
}
int smt_adcensus_compute_batch(smt_adcensus *hh, const float *L, const float *R, int pairs, int views, float *dispL, float *dispR)
{
    ENTER(pairs, views);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || pairs < 0 || views < 1 || views > 3) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs * 4;
    rd(L, n); rd(R, n);
    wr_opt(dispL, n, __func__, 0); wr_opt(dispR, n, __func__, 1);
    return SMT_OK;
}
int smt_adcensus_volume(smt_adcensus *hh, int view, float **vol)
{
    ENTER(view);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !vol || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    *vol = static_cast<float *>(h->own[view == SMT_VIEW_LEFT ? 0 : 1]);
    return SMT_OK;
}
int smt_adcensus_status(smt_adcensus *h) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }

int smt_wta(const float *vol, int H, int W, int D, float *disp, void *)
{
    ENTER(H, W, D);
    if (!vol || !disp || bad_size(H, W) || bad_D(D)) return SMT_ERR_ARG;
    rd(vol, (size_t)H * W * D * 4);
    wr(disp, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}
int smt_wta_subpixel(const float *vol, int H, int W, int D, const smt_subpixel_params *p, float *disp, void *)
{
    ENTER(H, W, D, p ? (long long)(p->min_den * 1000.0f) : -1);
    if (!vol || !disp || bad_size(H, W) || bad_D(D) || bad_sub(p)) return SMT_ERR_ARG;
    rd(vol, (size_t)H * W * D * 4);
    wr(disp, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}

// ---- cross-arm aggregation
void smt_crossarm_default_params(smt_crossarm_params *p) { *p = smt_crossarm_params{30, 6, 17, 34, 1, 0}; }
void smt_crossarm_cblsm_params(smt_crossarm_params *p) { *p = smt_crossarm_params{25, 6, 17, 34, 0, SMT_QUIRK_FIX_RIGHT_ARM_STRIDE}; }
int smt_crossarm_create(int H, int W, int D, const smt_crossarm_params *p, smt_crossarm **out)
{
    ENTER(H, W, D, p ? p->tau : -1, p ? p->max_length : -1, p ? p->sec_length : -1, p ? (long long)p->quirks : -1);
    if (!out || bad_size(H, W) || bad_D(D) || (p && bad_quirks(p->quirks))) return SMT_ERR_ARG;
    Handle *h = new_handle(H, W, D);
    for (int d = 0; d < 4; d++) h->own[d] = calloc(px(h), sizeof(int));
    *out = reinterpret_cast<smt_crossarm *>(h);
    return SMT_OK;
}
int smt_crossarm_destroy(smt_crossarm *h) { ENTER(); return del_handle(h); }
int smt_crossarm_set_subpixel(smt_crossarm *h, const smt_subpixel_params *p)
{
    ENTER(p ? (long long)(p->min_den * 1000.0f) : -1);
    return !h || bad_sub(p) ? SMT_ERR_ARG : SMT_OK;
}
int smt_crossarm_arms(smt_crossarm *hh, const uint8_t *img, int channels)
{
    ENTER(channels);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !img || (channels != 1 && channels != 3)) return SMT_ERR_ARG;
    rd(img, px(h) * channels);
    for (int d = 0; d < 4; d++) wr(h->own[d], px(h) * 4, __func__, d);
    h->aux = 1;
    return SMT_OK;
}
int smt_crossarm_reset(smt_crossarm *hh)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h) return SMT_ERR_ARG;
    for (int d = 0; d < 4; d++) memset(h->own[d], 0, px(h) * 4);
    return SMT_OK;
}
int smt_crossarm_arm_dir(smt_crossarm *hh, const uint8_t *img, int channels, int dir)
{
    ENTER(channels, dir);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !img || (channels != 1 && channels != 3) || dir < 0 || dir > 3) return SMT_ERR_ARG;
    rd(img, px(h) * channels);
    wr(h->own[dir], px(h) * 4, __func__, dir);
    h->aux = 1;
    return SMT_OK;
}
int smt_crossarm_arm_maps(smt_crossarm *hh, int **l, int **r, int **t, int **b)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h) return SMT_ERR_ARG;
    int **o[4] = {l, r, t, b};
    for (int d = 0; d < 4; d++) if (o[d]) *o[d] = static_cast<int *>(h->own[d]);
    return SMT_OK;
}
int smt_crossarm_load_arm_maps(smt_crossarm *hh, const int *l, const int *r, const int *t, const int *b)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !l || !r || !t || !b) return SMT_ERR_ARG;
    const int *in[4] = {l, r, t, b};
    for (int d = 0; d < 4; d++) memcpy(h->own[d], in[d], px(h) * 4);
    h->aux = 1;
    return SMT_OK;
}
int smt_crossarm_aggregate(smt_crossarm *hh, const float *in, float *out, int order, float *disp)
{
    ENTER(order, disp != nullptr);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !in || !out || in == out || order < 0 || order > 2) return SMT_ERR_ARG;
    if (!h->aux) return SMT_ERR_STATE;                 // aggregate before arms
    rd(in, px(h) * h->D * 4);
    for (int d = 0; d < 4; d++) rd(h->own[d], px(h) * 4);
    wr(out, px(h) * h->D * 4, __func__, 0);
    wr_opt(disp, px(h) * 4, __func__, 1);
    return SMT_OK;
}
int smt_crossarm_status(smt_crossarm *h) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }

int smt_cblsm_ad(const uint8_t *L, const uint8_t *R, int H, int W, int D, int view, float *vol, void *)
{
    ENTER(H, W, D, view);
    if (!L || !R || !vol || bad_size(H, W) || D < 1 || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    rd(L, (size_t)H * W); rd(R, (size_t)H * W);
    wr(vol, (size_t)H * W * D * 4, __func__, 0);
    return SMT_OK;
}
int smt_cblsm_choose_arm_length(int dir, const int *own, const int *vert, const int *RL, const int *RR, int H, int W, int D,
                                int *arm_volume, void *)
{
    ENTER(dir, H, W, D, vert != nullptr);
    if (dir < 0 || dir > 3 || !own || !RL || !RR || !arm_volume || bad_size(H, W) || D < 1 || (dir >= 2 && !vert)) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W * 4;
    rd(own, n); rd(RL, n); rd(RR, n);
    if (dir >= 2) rd(vert, n);
    wr(arm_volume, n * D, __func__, dir);
    return SMT_OK;
}
int smt_cblsm_cost_aggregation_v4(const float *in, const int *aL, const int *aR, const int *aU, const int *aD, int H, int W, int D,
                                  float *out, float *disp, int *ub_flag, void *)
{
    ENTER(H, W, D, disp != nullptr, ub_flag != nullptr);
    if (!in || !out || in == out || !aL || !aR || !aU || !aD || bad_size(H, W) || D < 1 || (disp && D > SMT_MAX_DISPARITY)) return SMT_ERR_ARG;
    const size_t V = (size_t)H * W * D * 4;
    rd(in, V); rd(aL, V); rd(aR, V); rd(aU, V); rd(aD, V);
    wr(out, V, __func__, 0);
    wr_opt(disp, (size_t)H * W * 4, __func__, 1);
    if (ub_flag) { rd(ub_flag, 4); if (flagged(__func__)) *ub_flag |= 1; }
    return SMT_OK;
}

// ---- scanline
int smt_scanline_create(int H, int W, int D, int p1, int p2, smt_scanline **out)
{
    ENTER(H, W, D, p1, p2);
    if (!out || bad_size(H, W) || bad_D(D)) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_scanline *>(new_handle(H, W, D));
    return SMT_OK;
}
int smt_scanline_destroy(smt_scanline *h) { ENTER(); return del_handle(h); }
int smt_scanline_set_quirks(smt_scanline *h, unsigned quirks) { ENTER(quirks); return !h || bad_quirks(quirks) ? SMT_ERR_ARG : SMT_OK; }
int smt_scanline_set_subpixel(smt_scanline *h, const smt_subpixel_params *p)
{
    ENTER(p ? (long long)(p->min_den * 1000.0f) : -1);
    return !h || bad_sub(p) ? SMT_ERR_ARG : SMT_OK;
}
int smt_scanline_run(smt_scanline *hh, const float *in, const float *gray, float *out, float *disp)
{
    ENTER(disp != nullptr);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !in || !gray || !out || in == out) return SMT_ERR_ARG;
    rd(in, px(h) * h->D * 4); rd(gray, px(h) * 4);
    wr(out, px(h) * h->D * 4, __func__, 0);
    wr_opt(disp, px(h) * 4, __func__, 1);
    return SMT_OK;
}

// ---- the pipeline
int smt_pipeline_create(int H, int W, int D, const smt_pipeline_params *p, smt_pipeline **out)
{
    ENTER(H, W, D, p != nullptr);
    if (!out || bad_size(H, W) || bad_D(D)) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_pipeline *>(new_handle(H, W, D));
    return SMT_OK;
}
int smt_pipeline_destroy(smt_pipeline *h) { ENTER(); return del_handle(h); }
int smt_pipeline_set_quirks(smt_pipeline *h, unsigned quirks) { ENTER(quirks); return !h || bad_quirks(quirks) ? SMT_ERR_ARG : SMT_OK; }
int smt_pipeline_set_subpixel(smt_pipeline *h, const smt_subpixel_params *p)
{
    ENTER(p ? (long long)(p->min_den * 1000.0f) : -1);
    return !h || bad_sub(p) ? SMT_ERR_ARG : SMT_OK;
}
int smt_pipeline_run_batch(smt_pipeline *hh, const uint8_t *L, const uint8_t *R, int pairs, float *dispL, float *dispR, uint8_t *cls,
                           int *counts)
{
    ENTER(pairs, counts != nullptr);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || !dispL || !dispR || !cls || pairs <= 0) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr(dispL, n * 4, __func__, 0); wr(dispR, n * 4, __func__, 1); wr(cls, n, __func__, 2);
    wr_opt(counts, (size_t)pairs * 8, __func__, 3);
    return SMT_OK;
}
int smt_pipeline_status(smt_pipeline *h) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }

// ---- the CBLSM flow and the window cost volumes
int smt_cblsm_flow_create_on(int device, int H, int W, int D, const smt_cblsm_params *, smt_cblsm_flow **out)
{
    ENTER(device, H, W, D);
    if (!out || bad_size(H, W) || bad_D(D)) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_cblsm_flow *>(new_handle(H, W, D));
    return SMT_OK;
}
int smt_cblsm_flow_destroy(smt_cblsm_flow *h) { ENTER(); return del_handle(h); }
static int cblsm_flow_run(const char *entry, smt_cblsm_flow *hh, const uint8_t *L, const uint8_t *R, int pairs, float *dl, float *dr)
{
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || !dl || !dr || pairs < 0) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr(dl, n * 4, entry, 0); wr(dr, n * 4, entry, 1);
    return SMT_OK;
}
int smt_cblsm_flow_run_batch(smt_cblsm_flow *h, const uint8_t *L, const uint8_t *R, int pairs, float *dl, float *dr)
{
    ENTER(pairs);
    return cblsm_flow_run(__func__, h, L, R, pairs, dl, dr);
}
int smt_cblsm_flow_run_batch_window(smt_cblsm_flow *h, const uint8_t *L, const uint8_t *R, int pairs, int winSize, float *dl, float *dr)
{
    ENTER(pairs, winSize);
    if (winSize < 0 || winSize > 89) return SMT_ERR_ARG;
    if (h && reinterpret_cast<Handle *>(h)->W <= winSize + 1) return SMT_ERR_REF_UB;
    return cblsm_flow_run(__func__, h, L, R, pairs, dl, dr);
}
int smt_cblsm_flow_status(smt_cblsm_flow *h) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }
int smt_cblsm_window_cost_batch(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D, int winSize,
                                int form, float *vol, size_t vol_stride, void *)
{
    ENTER(pairs, (long long)img_stride, H, W, D, winSize, form, (long long)vol_stride);
    if (!Lp || !Rp || !vol || bad_size(H, W) || pairs < 0 || pairs > 65535 || bad_D(D) || winSize < 0 || winSize > 89 || form < 1 ||
        form > 3)
        return SMT_ERR_ARG;
    const size_t img = padded(H, W, winSize) * (form == SMT_CBLSM_COST_V4 ? 3 : 1), v = (size_t)H * W * D;
    if ((img_stride && img_stride < img) || (vol_stride && vol_stride < v)) return SMT_ERR_ARG;
    if (form == SMT_CBLSM_COST_RIGHT && W <= winSize + 1) return SMT_ERR_REF_UB;
    for (int b = 0; b < pairs; b++) {
        rd(Lp + b * (img_stride ? img_stride : img), img); rd(Rp + b * (img_stride ? img_stride : img), img);
        wr(vol + b * (vol_stride ? vol_stride : v), v * 4, __func__, 0);
    }
    return SMT_OK;
}

// ---- LR checks and hole filling
int smt_lrcheck(float *dispL, const float *dispR, int H, int W, int gate, uint8_t *cls, int *counts, void *)
{
    ENTER(H, W, gate, counts != nullptr);
    if (!dispL || !dispR || !cls || bad_size(H, W)) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    rd(dispL, n * 4); rd(dispR, n * 4);
    wr(dispL, n * 4, __func__, 0); wr_cls(cls, n); wr_opt(counts, 8, __func__, 2);
    return SMT_OK;
}
int smt_lrcheck_variant(const float *dispL, const float *dispR, float *last, int H, int W, float gate, uint8_t *cls, int *counts, void *)
{
    ENTER(H, W, (long long)(gate * 1000.0f), counts != nullptr);
    if (!dispL || !dispR || !last || !cls || bad_size(H, W)) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    rd(dispL, n * 4); rd(dispR, n * 4);
    wr(last, n * 4, __func__, 0); wr_cls(cls, n); wr_opt(counts, 8, __func__, 2);
    return SMT_OK;
}
// a host helper of the real library too: the expansion itself is its contract
int smt_lrcheck_lists(const uint8_t *cls, int H, int W, int *occ, int *n_occ, int *mis, int *n_mis)
{
    ENTER(H, W);
    if (!cls || !occ || !mis || !n_occ || !n_mis || bad_size(H, W)) return SMT_ERR_ARG;
    int no = 0, nm = 0;
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            const uint8_t c = cls[(size_t)i * W + j];
            if (c == 1) { occ[2 * no] = i; occ[2 * no + 1] = j; no++; }
            else if (c == 2) { mis[2 * nm] = i; mis[2 * nm + 1] = j; nm++; }
        }
    // "room for H*W pairs": the rest of both lists belongs to the entry as well
    for (size_t k = 2 * (size_t)no; k < 2 * (size_t)H * W; k++) occ[k] = -1;
    for (size_t k = 2 * (size_t)nm; k < 2 * (size_t)H * W; k++) mis[k] = -1;
    *n_occ = no; *n_mis = nm;
    return SMT_OK;
}
int smt_fill_the_hole(float *disp, int row, int col, int dispRange, const int *occ, int n_occ, const int *mis, int n_mis, int *third,
                      int *n_third, void *)
{
    ENTER(row, col, dispRange, n_occ, n_mis, third != nullptr, n_third != nullptr);
    if (!disp || bad_size(row, col) || dispRange < 0 || n_occ < 0 || n_mis < 0 || (n_occ && !occ) || (n_mis && !mis)) return SMT_ERR_ARG;
    const size_t n = (size_t)row * col;
    rd(disp, n * 4);
    if (n_occ) rd(occ, (size_t)n_occ * 8);
    if (n_mis) rd(mis, (size_t)n_mis * 8);
    wr(disp, n * 4, __func__, 0);
    // the third pass runs only when the mismatch list is not empty (:174): one entry then, else "not replaced"
    if (third) { wr(third, n * 8, __func__, 1); if (n_mis) { third[0] = row - 1; third[1] = col - 1; } }
    if (n_third) *n_third = n_mis ? 1 : -1;
    return SMT_OK;
}
int smt_fill_the_hole_batch(float *disp, const uint8_t *cls, int pairs, size_t ds, size_t cs, int row, int col, int dispRange, int *status,
                            void *)
{
    ENTER(pairs, (long long)ds, (long long)cs, row, col, dispRange, status != nullptr);
    const size_t n = (size_t)row * col;
    if (!disp || !cls || bad_size(row, col) || dispRange < 0 || pairs < 0 || (ds && ds < n) || (cs && cs < n)) return SMT_ERR_ARG;
    for (int b = 0; b < pairs; b++) {
        rd(disp + b * (ds ? ds : n), n * 4); rd(cls + b * (cs ? cs : n), n);
        wr(disp + b * (ds ? ds : n), n * 4, __func__, 0);
    }
    wr_opt(status, (size_t)pairs * 16, __func__, 1);
    return SMT_OK;
}

// ---- CrossAggregator
int smt_crossagg_create(int W, int H, int D, smt_crossagg **out)
{
    ENTER(W, H, D);
    if (!out || (long long)W * H <= 0 || W <= 0 || D < 1 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    Handle *h = new_handle(H, W, D);
    h->own[0] = calloc(px(h) * D, sizeof(float));
    h->own[1] = calloc(px(h), 4);
    *out = reinterpret_cast<smt_crossagg *>(h);
    return SMT_OK;
}
int smt_crossagg_destroy(smt_crossagg *h) { ENTER(); return del_handle(h); }
int smt_crossagg_set_params(smt_crossagg *h, int L1, int L2, int t1, int t2) { ENTER(L1, L2, t1, t2); return !h || L1 < 0 ? SMT_ERR_ARG : SMT_OK; }
int smt_crossagg_aggregate(smt_crossagg *hh, const uint8_t *img, const float *cost, int num_iters)
{
    ENTER(num_iters);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !img || !cost || num_iters < 0) return SMT_ERR_ARG;
    rd(img, px(h) * 3); rd(cost, px(h) * h->D * 4);
    wr(h->own[0], px(h) * h->D * 4, __func__, 0); wr(h->own[1], px(h) * 4, __func__, 1);
    return SMT_OK;
}
int smt_crossagg_cost(smt_crossagg *h, float **cost)
{
    ENTER();
    if (!h || !cost) return SMT_ERR_ARG;
    *cost = static_cast<float *>(reinterpret_cast<Handle *>(h)->own[0]);
    return SMT_OK;
}
int smt_crossagg_arms(smt_crossagg *h, uint8_t **arms)
{
    ENTER();
    if (!h || !arms) return SMT_ERR_ARG;
    *arms = static_cast<uint8_t *>(reinterpret_cast<Handle *>(h)->own[1]);
    return SMT_OK;
}

// ---- window matchers
int smt_sad(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize, int view, int32_t *disp, void *)
{
    ENTER(H, W, D, winsize, view);
    if (!Lp || !Rp || !disp || bad_size(H, W) || bad_D(D) || winsize < 0 || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT))
        return SMT_ERR_ARG;
    rd(Lp, padded(H, W, winsize)); rd(Rp, padded(H, W, winsize));
    wr(disp, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}
int smt_sad_both(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize, int32_t *dl, int32_t *dr, float *costL, void *)
{
    ENTER(H, W, D, winsize, costL != nullptr);
    if (!Lp || !Rp || !dl || !dr || bad_size(H, W) || bad_D(D) || winsize < 0) return SMT_ERR_ARG;
    rd(Lp, padded(H, W, winsize)); rd(Rp, padded(H, W, winsize));
    wr(dl, (size_t)H * W * 4, __func__, 0); wr(dr, (size_t)H * W * 4, __func__, 1);
    wr_opt(costL, (size_t)H * W * D * 4, __func__, 2);
    return SMT_OK;
}
void smt_sad_default_params(smt_sad_params *p) { p->winsize = 3; }
int smt_sad_flow_create_on(int device, int H, int W, int D, const smt_sad_params *p, smt_sad_flow **out)
{
    ENTER(device, H, W, D, p ? p->winsize : -1);
    if (!out || bad_size(H, W) || bad_D(D) || (p && p->winsize < 0)) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_sad_flow *>(new_handle(H, W, D));
    return SMT_OK;
}
int smt_sad_flow_destroy(smt_sad_flow *h) { ENTER(); return del_handle(h); }
int smt_sad_flow_run_batch(smt_sad_flow *hh, const uint8_t *L, const uint8_t *R, int pairs, int32_t *dl, int32_t *dr, int32_t *last,
                           uint8_t *cls)
{
    ENTER(pairs);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || pairs < 0) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr_opt(dl, n * 4, __func__, 0); wr_opt(dr, n * 4, __func__, 1); wr_opt(last, n * 4, __func__, 2); wr_opt(cls, n, __func__, 3);
    return SMT_OK;
}

int smt_ncc(const uint8_t *L, const uint8_t *R, int H, int W, int D, int winSize, int32_t *disp, double *cost, void *)
{
    ENTER(H, W, D, winSize, cost != nullptr);
    if (!L || !R || !disp || bad_size(H, W) || bad_D(D) || winSize < 0) return SMT_ERR_ARG;
    rd(L, (size_t)H * W); rd(R, (size_t)H * W);
    wr(disp, (size_t)H * W * 4, __func__, 0);
    wr_opt(cost, (size_t)H * W * D * 8, __func__, 1);
    return SMT_OK;
}
void smt_ncc_default_params(smt_ncc_params *p) { p->winSize = 10; }
int smt_ncc_flow_create_on(int device, int H, int W, int D, const smt_ncc_params *p, smt_ncc_flow **out)
{
    ENTER(device, H, W, D, p ? p->winSize : -1);
    if (!out || bad_size(H, W) || bad_D(D) || (p && p->winSize < 0)) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_ncc_flow *>(new_handle(H, W, D));
    return SMT_OK;
}
int smt_ncc_flow_destroy(smt_ncc_flow *h) { ENTER(); return del_handle(h); }
int smt_ncc_flow_set_form(smt_ncc_flow *h, int form) { ENTER(form); return !h || form < 0 || form > 3 ? SMT_ERR_ARG : SMT_OK; }
int smt_ncc_flow_run_batch(smt_ncc_flow *hh, const uint8_t *L, const uint8_t *R, int pairs, int32_t *disp, double *cost)
{
    ENTER(pairs, cost != nullptr);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || !disp || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr(disp, n * 4, __func__, 0); wr_opt(cost, n * h->D * 8, __func__, 1);
    return SMT_OK;
}
int smt_lrncc_flow_run_batch(smt_ncc_flow *hh, const uint8_t *L, const uint8_t *R, int pairs, int32_t *dl, int32_t *dr, int32_t *last,
                             uint8_t *cls)
{
    ENTER(pairs);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr_opt(dl, n * 4, __func__, 0); wr_opt(dr, n * 4, __func__, 1); wr_opt(last, n * 4, __func__, 2); wr_opt(cls, n, __func__, 3);
    return SMT_OK;
}
static int whole_bad(int H, int W, const smt_whole_ncc_params *p)
{
    const int k = p ? p->kernel_size : 5, O = p ? p->max_offset : 79;
    if (H < 2 || W < 2 || k < 1 || O < 1 || O > SMT_MAX_DISPARITY || H > 65535) return SMT_ERR_ARG;
    if (O > W) return SMT_ERR_REF_UB;
    return SMT_OK;
}
int smt_whole_ncc(const uint8_t *L, const uint8_t *R, int H, int W, const smt_whole_ncc_params *p, int view, uint8_t *depth, int32_t *offset,
                  double *cost, void *)
{
    ENTER(H, W, p ? p->kernel_size : -1, p ? p->max_offset : -1, p ? p->add_constant : -1, view, offset != nullptr, cost != nullptr);
    if (!L || !R || !depth || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    if (const int rc = whole_bad(H, W, p)) return rc;
    rd(L, (size_t)H * W); rd(R, (size_t)H * W);
    wr(depth, (size_t)H * W, __func__, 0);
    wr_opt(offset, (size_t)H * W * 4, __func__, 1);
    wr_opt(cost, (size_t)H * W * (p ? p->max_offset : 79) * 8, __func__, 2);
    return SMT_OK;
}
int smt_bgr_to_grey_batch(const uint8_t *bgr, int n, int H, int W, uint8_t *grey, void *)
{
    ENTER(n, H, W);
    if (!bgr || !grey || n < 0 || bad_size(H, W)) return SMT_ERR_ARG;
    rd(bgr, (size_t)n * H * W * 3);
    wr(grey, (size_t)n * H * W, __func__, 0);
    return SMT_OK;
}
int smt_whole_ncc_flow_create_on(int device, int H, int W, const smt_whole_ncc_params *p, smt_whole_ncc_flow **out)
{
    ENTER(device, H, W, p ? p->kernel_size : -1, p ? p->max_offset : -1, p ? p->add_constant : -1);
    if (!out) return SMT_ERR_ARG;
    if (const int rc = whole_bad(H, W, p)) return rc;
    *out = reinterpret_cast<smt_whole_ncc_flow *>(new_handle(H, W, p ? p->max_offset : 79));
    return SMT_OK;
}
int smt_whole_ncc_flow_destroy(smt_whole_ncc_flow *h) { ENTER(); return del_handle(h); }
int smt_whole_ncc_flow_set_form(smt_whole_ncc_flow *h, int form) { ENTER(form); return !h || form < 0 || form > 2 ? SMT_ERR_ARG : SMT_OK; }
int smt_whole_ncc_flow_run_batch(smt_whole_ncc_flow *hh, const uint8_t *L, const uint8_t *R, int pairs, uint8_t *dL, uint8_t *dR, int32_t *oL,
                                 int32_t *oR, int32_t *last, uint8_t *cls)
{
    ENTER(pairs);
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || pairs < 0 || pairs > 32767) return SMT_ERR_ARG;
    const size_t n = px(h) * (size_t)pairs;
    rd(L, n); rd(R, n);
    wr_opt(dL, n, __func__, 0); wr_opt(dR, n, __func__, 1); wr_opt(oL, n * 4, __func__, 2); wr_opt(oR, n * 4, __func__, 3);
    wr_opt(last, n * 4, __func__, 4); wr_opt(cls, n, __func__, 5);
    return SMT_OK;
}

int smt_asw_masks(int winSize, double, double, double *space, double *color)
{
    ENTER(winSize);
    if (winSize < 0 || winSize > 30 || !space || !color) return SMT_ERR_ARG;
    const size_t side = 2 * (size_t)winSize + 3;
    wr(space, side * side * 8, __func__, 0); wr(color, 256 * 8, __func__, 1);
    return SMT_OK;
}
static int asw_bad(const void *Lp, const void *Rp, int H, int W, int D, int winSize, const void *sp, const void *cm)
{
    return !Lp || !Rp || !sp || !cm || bad_size(H, W) || bad_D(D) || winSize < 0 || winSize > 30;
}
static void asw_read(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int winSize, const double *sp, const double *cm)
{
    const size_t side = 2 * (size_t)winSize + 3;
    rd(Lp, padded(H, W, winSize)); rd(Rp, padded(H, W, winSize)); rd(sp, side * side * 8); rd(cm, 256 * 8);
}
int smt_asw(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winSize, const double *sp, const double *cm, int T, int view,
            float *disp, float *cost, void *)
{
    ENTER(H, W, D, winSize, T, view, cost != nullptr);
    if (asw_bad(Lp, Rp, H, W, D, winSize, sp, cm) || !disp || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    asw_read(Lp, Rp, H, W, winSize, sp, cm);
    wr(disp, (size_t)H * W * 4, __func__, 0); wr_opt(cost, (size_t)H * W * D * 4, __func__, 1);
    return SMT_OK;
}
int smt_asw_both(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winSize, const double *sp, const double *cm, int T, float *dl,
                 float *dr, float *cl, float *cr, void *)
{
    ENTER(H, W, D, winSize, T, cl != nullptr, cr != nullptr);
    if (asw_bad(Lp, Rp, H, W, D, winSize, sp, cm) || !dl || !dr) return SMT_ERR_ARG;
    asw_read(Lp, Rp, H, W, winSize, sp, cm);
    wr(dl, (size_t)H * W * 4, __func__, 0); wr(dr, (size_t)H * W * 4, __func__, 1);
    wr_opt(cl, (size_t)H * W * D * 4, __func__, 2); wr_opt(cr, (size_t)H * W * D * 4, __func__, 3);
    return SMT_OK;
}
int smt_asw_crosscheck(const float *dl, const float *dr, int H, int W, uint8_t *out, void *)
{
    ENTER(H, W);
    if (!dl || !dr || !out || bad_size(H, W)) return SMT_ERR_ARG;
    rd(dl, (size_t)H * W * 4); rd(dr, (size_t)H * W * 4);
    wr(out, (size_t)H * W, __func__, 0);
    return SMT_OK;
}

// ---- post-filters
int smt_median_filter(const float *in, float *out, int W, int H, int wnd, void *)
{
    ENTER(W, H, wnd);
    if (!in || !out || in == out || bad_size(H, W) || wnd < 1 || wnd > 7) return SMT_ERR_ARG;
    rd(in, (size_t)H * W * 4);
    wr(out, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}
int smt_median_filter_inplace(float *disp, int W, int H, int wnd, void *)
{
    ENTER(W, H, wnd);
    if (!disp || bad_size(H, W) || wnd < 1 || wnd > 7) return SMT_ERR_ARG;
    rd(disp, (size_t)H * W * 4);
    wr(disp, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}
int smt_remove_speckles(float *map, int W, int H, int diff, unsigned min_area, int invalid, void *)
{
    ENTER(W, H, diff, (long long)min_area, invalid);
    if (!map || bad_size(H, W)) return SMT_ERR_ARG;
    rd(map, (size_t)H * W * 4);
    wr(map, (size_t)H * W * 4, __func__, 0);
    return SMT_OK;
}
int smt_fill_image_new_batch(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts, void *)
{
    ENTER(pairs, (long long)stride, H, W, fix, counts != nullptr);
    const size_t n = (size_t)H * W;
    if (!maps || pairs <= 0 || bad_size(H, W) || W > 65535 || (stride && stride < n) || (fix & ~SMT_ASW_FIX_FILL_ROW_END)) return SMT_ERR_ARG;
    for (int b = 0; b < pairs; b++) { rd(maps + b * (stride ? stride : n), n); wr(maps + b * (stride ? stride : n), n, __func__, 0); }
    wr_opt(counts, (size_t)pairs * 8, __func__, 1);
    return SMT_OK;
}
int smt_asw_tail_batch(uint8_t *last, int pairs, size_t stride, int H, int W, const smt_asw_post_params *post, uint8_t *am, uint8_t *af,
                       int *counts, int *err_dev, void *)
{
    ENTER(pairs, (long long)stride, H, W, post != nullptr, am != nullptr, af != nullptr, counts != nullptr, err_dev != nullptr);
    const size_t n = (size_t)H * W;
    if (!last || pairs < 0 || bad_size(H, W) || W > 65535 || (stride && stride < n)) return SMT_ERR_ARG;
    if (post && ((post->median_first != 3 && post->median_first != 5) || (post->median_last != 3 && post->median_last != 5) ||
                 (post->fix & ~SMT_ASW_FIX_FILL_ROW_END)))
        return SMT_ERR_ARG;
    for (int b = 0; b < pairs; b++) {
        const size_t o = b * (stride ? stride : n);
        rd(last + o, n); wr(last + o, n, __func__, 0);
        if (am) wr(am + o, n, __func__, 1);
        if (af) wr(af + o, n, __func__, 2);
    }
    wr_opt(counts, (size_t)pairs * 8, __func__, 3);
    if (err_dev) { rd(err_dev, 4); if (flagged(__func__)) *err_dev = 1; }
    return SMT_OK;
}

// ---- images
int smt_image_read(const char *path, int want, uint8_t **pixels, int *H, int *W, int *channels)
{
    ENTER(want);
    if (!path || !pixels || !H || !W || !channels || want < 0 || want > 3 || want == 2) return SMT_ERR_ARG;
    *H = 2; *W = 3; *channels = want ? want : 1;
    *pixels = static_cast<uint8_t *>(malloc((size_t)6 * *channels));
    wr(*pixels, (size_t)6 * *channels, __func__, 0);
    return SMT_OK;
}
int smt_image_free(uint8_t *pixels) { ENTER(); free(pixels); return SMT_OK; }
int smt_image_write(const char *path, const uint8_t *pixels, int H, int W, int channels)
{
    ENTER(H, W, channels);
    if (!path || !pixels || bad_size(H, W) || (channels != 1 && channels != 3)) return SMT_ERR_ARG;
    rd(pixels, (size_t)H * W * channels);
    return SMT_OK;
}
int smt_bgr2gray(const uint8_t *bgr, int H, int W, uint8_t *gray, void *)
{
    ENTER(H, W);
    if (!bgr || !gray || bad_size(H, W)) return SMT_ERR_ARG;
    rd(bgr, (size_t)H * W * 3);
    wr(gray, (size_t)H * W, __func__, 0);
    return SMT_OK;
}

}  // extern "C"
