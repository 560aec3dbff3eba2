// Host-only contract stub of the entries that host/smt_scan_views.hpp calls (include/smt_scan_views.h and the plumbing
// of include/smt.h), in the manner of tests/cpp_mirror/smt_contract_stub.cpp.  No HIP.  It computes nothing: "device"
// memory is malloc'ed with the exact byte count, every entry rejects what its header says it rejects, reads every byte
// of every input extent and fills every output extent with a byte that names the output, so under AddressSanitizer a
// mirror that sizes, uploads or downloads a buffer wrongly faults here.
#include "scan_views_stub.hpp"

#include <cstdlib>
#include <cstring>

#include "../../include/smt_scan_views.h"

namespace {
int g_allocs = 0, g_handles = 0;
std::vector<std::string> g_log;
std::string g_fail;
volatile unsigned g_sink = 0;

struct Handle {
    int H, W, D, views;
    unsigned quirks;
    float min_den;
    float *lent;
    bool ran_both;
};
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
Handle *make(int H, int W, int D)
{
    g_handles++;
    return new Handle{H, W, D, SMT_VIEW_LEFT, 0u, 0.0f, nullptr, false};
}
int drop(void *p)
{
    if (!p) return SMT_ERR_ARG;
    Handle *h = static_cast<Handle *>(p);
    free(h->lent);
    delete h;
    g_handles--;
    return SMT_OK;
}
size_t vol(const Handle *h) { return (size_t)h->H * h->W * h->D * 4; }
size_t map(const Handle *h) { return (size_t)h->H * h->W * 4; }
}  // namespace

const std::vector<std::string> &stub_log() { return g_log; }
void stub_log_clear() { g_log.clear(); }
void stub_fail(const char *entry) { g_fail = entry; }
int stub_live_allocs() { return g_allocs; }
int stub_live_handles() { return g_handles; }

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

int smt_scanline_create(int H, int W, int D, int, int, smt_scanline **out)
{
    ENTER();
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_scanline *>(make(H, W, D));
    return SMT_OK;
}
int smt_scanline_destroy(smt_scanline *h) { return drop(h); }
int smt_scanline_set_quirks(smt_scanline *h, unsigned quirks)
{
    ENTER();
    if (!h || (quirks & ~SMT_QUIRK_FIX_ALL)) return SMT_ERR_ARG;
    reinterpret_cast<Handle *>(h)->quirks = quirks;
    return SMT_OK;
}
int smt_scanline_set_subpixel(smt_scanline *h, const smt_subpixel_params *p)
{
    ENTER();
    if (!h || (p && !(p->min_den > 0.0f))) return SMT_ERR_ARG;
    reinterpret_cast<Handle *>(h)->min_den = p ? p->min_den : 0.0f;
    return SMT_OK;
}
int smt_scanline_run_pair(smt_scanline *hh, const float *vinL, const float *grayL, float *voutL, float *dispL, const float *vinR,
                          const float *grayR, float *voutR, float *dispR)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !vinL || !grayL || !vinR || !grayR || (!voutL && !dispL) || (!voutR && !dispR)) return SMT_ERR_ARG;
    if ((voutL && (voutL == vinL || voutL == vinR || voutL == voutR)) || (voutR && (voutR == vinL || voutR == vinR)) ||
        (dispL && dispL == dispR))
        return SMT_ERR_ARG;
    rd(vinL, vol(h)); rd(vinR, vol(h)); rd(grayL, map(h)); rd(grayR, map(h));
    if (voutL) memset(voutL, STUB_VOUT_L, vol(h));
    if (voutR) memset(voutR, STUB_VOUT_R, vol(h));
    if (dispL) memset(dispL, STUB_DISP_L, map(h));
    if (dispR) memset(dispR, STUB_DISP_R, map(h));
    return SMT_OK;
}
int smt_scanline_run_map(smt_scanline *hh, const float *vin, const float *gray, float *disp)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !vin || !gray || !disp) return SMT_ERR_ARG;
    rd(vin, vol(h)); rd(gray, map(h));
    memset(disp, STUB_DISP_L, map(h));
    return SMT_OK;
}

int smt_pipeline_create(int H, int W, int D, const smt_pipeline_params *, smt_pipeline **out)
{
    ENTER();
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY) return SMT_ERR_ARG;
    *out = reinterpret_cast<smt_pipeline *>(make(H, W, D));
    return SMT_OK;
}
int smt_pipeline_destroy(smt_pipeline *h) { return drop(h); }
int smt_pipeline_set_quirks(smt_pipeline *h, unsigned quirks)
{
    ENTER();
    return !h || (quirks & ~SMT_QUIRK_FIX_ALL) ? SMT_ERR_ARG : SMT_OK;
}
int smt_pipeline_set_subpixel(smt_pipeline *h, const smt_subpixel_params *p)
{
    ENTER();
    return !h || (p && !(p->min_den > 0.0f)) ? SMT_ERR_ARG : SMT_OK;
}
int smt_pipeline_set_scan_views(smt_pipeline *h, int views)
{
    ENTER();
    if (!h || (views != SMT_VIEW_LEFT && views != SMT_VIEW_BOTH)) return SMT_ERR_ARG;
    reinterpret_cast<Handle *>(h)->views = views;
    return SMT_OK;
}
int smt_pipeline_run_batch(smt_pipeline *hh, const uint8_t *L, const uint8_t *R, int pairs, float *dispL, float *dispR, uint8_t *cls,
                           int *counts)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !L || !R || !dispL || !dispR || !cls || pairs <= 0) return SMT_ERR_ARG;
    const size_t n = (size_t)h->H * h->W * (size_t)pairs;
    rd(L, n); rd(R, n);
    memset(dispL, STUB_DISP_L, n * 4);
    memset(dispR, h->views == SMT_VIEW_BOTH ? STUB_DISP_R : STUB_DISP_R_LEFT, n * 4);
    memset(cls, STUB_CLS, n);
    if (counts) memset(counts, 0, (size_t)pairs * 8);
    if (h->views == SMT_VIEW_BOTH) {
        if (!h->lent) h->lent = static_cast<float *>(malloc(vol(h)));
        memset(h->lent, STUB_VOUT_R, vol(h));
        h->ran_both = true;
    }
    return SMT_OK;
}
int smt_pipeline_status(smt_pipeline *h) { ENTER(); return h ? SMT_OK : SMT_ERR_ARG; }
int smt_pipeline_scan_right_volume(smt_pipeline *hh, float **sum)
{
    ENTER();
    Handle *h = reinterpret_cast<Handle *>(hh);
    if (!h || !sum) return SMT_ERR_ARG;
    if (!h->ran_both) return SMT_ERR_STATE;
    *sum = h->lent;
    return SMT_OK;
}

}  // extern "C"
