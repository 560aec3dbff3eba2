// Host-only contract stub of the entries that host/smt_refine.hpp calls (include/smt_refine.h and the plumbing of
// include/smt.h), in the manner of tests/cpp_mirror_bilateral/bilateral_stub.cpp.  No HIP.  It refines nothing: "device"
// memory is malloc'ed with the exact byte count, every entry rejects what its header says it rejects, reads every byte of
// every input extent and fills every output extent with a byte that names the output, so under AddressSanitizer a mirror
// that sizes, uploads or downloads a buffer wrongly faults here.
#include "refine_stub.hpp"

#include <cstdlib>
#include <cstring>

#include "../../include/smt_refine.h"

struct smt_crossarm {                          // what ArmMaps needs of a handle: its size, its parameters, four maps
    int H, W;
    smt_crossarm_params P;
    int *maps;
    bool armed;
};

namespace {
int g_allocs = 0;
std::vector<std::string> g_log;
std::string g_fail;
volatile unsigned g_sink = 0;
StubCall g_last = {};
unsigned g_last_quirks = 0;

bool fail(const char *entry)
{
    g_log.push_back(entry);
    if (g_fail != entry) return false;
    g_fail.clear();
    return true;
}
void rd(const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    unsigned s = 0;
    for (size_t i = 0; i < bytes; i++) s += b[i];
    g_sink = g_sink + s;
}
bool stride_ok(size_t s, size_t n) { return s == 0 || s >= n; }

int entry(float *maps, int pairs, size_t map_stride, const int *const arm[4], size_t arm_stride, bool want_arms, const uint8_t *cls,
          size_t cls_stride, const uint8_t *gray, size_t gray_stride, bool want_cls, int H, int W, int D, const smt_refine_params *params,
          uint8_t *state, size_t state_stride, int *status)
{
    smt_refine_params p;
    if (params) p = *params; else smt_refine_default_params(&p);
    if (!maps || pairs < 0 || H <= 0 || W <= 0 || D < 1 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    if (p.irv_iters < 0 || p.irv_iters > 16 || p.search < 0) return SMT_ERR_ARG;
    if (want_arms && (!arm[0] || !arm[1] || !arm[2] || !arm[3])) return SMT_ERR_ARG;
    if (want_cls && (!cls || !gray)) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    if (!stride_ok(map_stride, n) || !stride_ok(arm_stride, n) || !stride_ok(cls_stride, n) || !stride_ok(gray_stride, n) ||
        !stride_ok(state_stride, n))
        return SMT_ERR_ARG;
    for (int b = 0; b < pairs; b++) {
        float *m = maps + b * (map_stride ? map_stride : n);
        rd(m, n * 4);
        if (want_arms)
            for (int k = 0; k < 4; k++) rd(arm[k] + b * (arm_stride ? arm_stride : n), n * 4);
        if (want_cls) { rd(cls + b * (cls_stride ? cls_stride : n), n); rd(gray + b * (gray_stride ? gray_stride : n), n); }
        memset(m, STUB_MAP, n * 4);
        if (state) memset(state + b * (state_stride ? state_stride : n), STUB_STATE, n);
        if (status) memset(status + 4 * b, STUB_STATUS, 16);
    }
    g_last = StubCall{pairs, H, W, D, p.irv_ts, p.irv_iters, p.search, p.irv_th, want_arms, want_cls, state != nullptr, status != nullptr};
    return SMT_OK;
}
}  // namespace

const std::vector<std::string> &stub_log() { return g_log; }
void stub_log_clear() { g_log.clear(); }
void stub_fail(const char *entry) { g_fail = entry; }
int stub_live_allocs() { return g_allocs; }
const StubCall &stub_last_refine() { return g_last; }
unsigned stub_last_arm_quirks() { return g_last_quirks; }

#define ENTER() do { if (fail(__func__)) return SMT_ERR_HIP; } while (0)

extern "C" {

const char *smt_strerror(int status) { return status == SMT_OK ? "ok" : status == SMT_ERR_ARG ? "bad argument" : "error"; }
int smt_malloc(void **dptr, size_t bytes)
{
    ENTER();
    if (!dptr) return SMT_ERR_ARG;
    *dptr = malloc(bytes);
    if (!*dptr) return SMT_ERR_ALLOC;
    memset(*dptr, 0xCD, bytes);
    g_allocs++;
    return SMT_OK;
}
int smt_free(void *dptr) { if (dptr) { free(dptr); g_allocs--; } return SMT_OK; }
int smt_memcpy_h2d(void *d, const void *s, size_t n, void *) { ENTER(); if (n) memcpy(d, s, n); return SMT_OK; }
int smt_memcpy_d2h(void *d, const void *s, size_t n, void *) { ENTER(); if (n) memcpy(d, s, n); return SMT_OK; }
int smt_stream_sync(void *) { ENTER(); return SMT_OK; }

void smt_crossarm_default_params(smt_crossarm_params *p)
{
    p->tau = 30; p->tau_low = 6; p->sec_length = 17; p->max_length = 34; p->chain_tau = 1; p->quirks = 0;
}
int smt_crossarm_create(int H, int W, int D, const smt_crossarm_params *p, smt_crossarm **out)
{
    ENTER();
    if (!out || !p || H <= 0 || W <= 0 || D <= 0 || (p->quirks & ~SMT_QUIRK_FIX_ALL)) return SMT_ERR_ARG;
    smt_crossarm *h = static_cast<smt_crossarm *>(malloc(sizeof(smt_crossarm)));
    h->H = H; h->W = W; h->P = *p; h->armed = false;
    h->maps = static_cast<int *>(malloc((size_t)4 * H * W * sizeof(int)));
    g_allocs += 2;
    *out = h;
    return SMT_OK;
}
int smt_crossarm_destroy(smt_crossarm *h)
{
    if (!h) return SMT_ERR_ARG;
    free(h->maps); free(h);
    g_allocs -= 2;
    return SMT_OK;
}
int smt_crossarm_arms(smt_crossarm *h, const uint8_t *img, int channels)
{
    ENTER();
    if (!h || !img || (channels != 1 && channels != 3)) return SMT_ERR_ARG;
    rd(img, (size_t)h->H * h->W * channels);
    for (int k = 0; k < 4; k++)                                       // map k holds tau + k everywhere
        for (size_t x = 0; x < (size_t)h->H * h->W; x++) h->maps[k * (size_t)h->H * h->W + x] = h->P.tau + k;
    h->armed = true;
    g_last_quirks = h->P.quirks;
    return SMT_OK;
}
int smt_crossarm_arm_maps(smt_crossarm *h, int **left, int **right, int **top, int **bottom)
{
    ENTER();
    if (!h || !h->armed) return SMT_ERR_STATE;
    const size_t n = (size_t)h->H * h->W;
    *left = h->maps; *right = h->maps + n; *top = h->maps + 2 * n; *bottom = h->maps + 3 * n;
    return SMT_OK;
}

void smt_refine_default_params(smt_refine_params *p)
{
    if (!p) return;
    p->irv_ts = 20; p->irv_th = 0.4f; p->irv_iters = 5; p->search = 0;
}

int smt_region_vote_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT, const int *armB,
                          size_t arm_stride, int H, int W, int D, const smt_refine_params *params, uint8_t *state, size_t state_stride,
                          int *status, void *)
{
    ENTER();
    const int *arm[4] = {armL, armR, armT, armB};
    return entry(maps, pairs, map_stride, arm, arm_stride, true, nullptr, 0, nullptr, 0, false, H, W, D, params, state, state_stride, status);
}

int smt_interpolate_outliers_batch(float *maps, int pairs, size_t map_stride, const uint8_t *cls, size_t cls_stride, const uint8_t *gray,
                                   size_t gray_stride, int H, int W, int D, const smt_refine_params *params, uint8_t *state,
                                   size_t state_stride, int *status, void *)
{
    ENTER();
    const int *arm[4] = {nullptr, nullptr, nullptr, nullptr};
    return entry(maps, pairs, map_stride, arm, 0, false, cls, cls_stride, gray, gray_stride, true, H, W, D, params, state, state_stride, status);
}

int smt_refine_batch(float *maps, int pairs, size_t map_stride, const int *armL, const int *armR, const int *armT, const int *armB,
                     size_t arm_stride, const uint8_t *cls, size_t cls_stride, const uint8_t *gray, size_t gray_stride, int H, int W, int D,
                     const smt_refine_params *params, uint8_t *state, size_t state_stride, int *status, void *)
{
    ENTER();
    const int *arm[4] = {armL, armR, armT, armB};
    return entry(maps, pairs, map_stride, arm, arm_stride, true, cls, cls_stride, gray, gray_stride, true, H, W, D, params, state,
                 state_stride, status);
}

}  // extern "C"
