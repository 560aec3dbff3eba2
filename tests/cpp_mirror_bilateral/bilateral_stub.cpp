// Host-only contract stub of the entries that host/smt_bilateral.hpp calls (include/smt_bilateral.h and the plumbing of
// include/smt.h), in the manner of tests/cpp_mirror_scan_views/scan_views_stub.cpp.  No HIP.  It filters nothing: "device"
// memory is malloc'ed with the exact byte count, every entry rejects what its header says it rejects, reads every byte of
// every input extent (all wsize_h * wsize_w and 256 table entries) and fills every output extent with a byte that names
// the output, so under AddressSanitizer a mirror that sizes, uploads or downloads a buffer wrongly faults here.  The
// tables are the header's formulas, so that the mirror's getGausssianMask / getColorMask can be checked by value.
#include "bilateral_stub.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/smt_bilateral.h"

namespace {
int g_allocs = 0;
std::vector<std::string> g_log;
std::string g_fail;
volatile unsigned g_sink = 0;
StubCall g_last = {};

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
}  // namespace

const std::vector<std::string> &stub_log() { return g_log; }
void stub_log_clear() { g_log.clear(); }
void stub_fail(const char *entry) { g_fail = entry; }
int stub_live_allocs() { return g_allocs; }
const StubCall &stub_last_filter() { return g_last; }

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

int smt_bilateral_masks(int wsize_h, int wsize_w, double sigma_space, double sigma_color, double *space_host, double *color_host)
{
    ENTER();
    if (!space_host || !color_host || wsize_h < 1 || wsize_h > 64 || wsize_w < 1 || wsize_w > 64) return SMT_ERR_ARG;
    const int ch = (wsize_h - 1) / 2, cw = (wsize_w - 1) / 2;
    for (int i = 0; i < wsize_h; i++)
        for (int j = 0; j < wsize_w; j++)
            space_host[i * wsize_w + j] = exp(-(double)((j - cw) * (j - cw) + (i - ch) * (i - ch)) / (2 * sigma_space * sigma_space));
    for (int i = 0; i < 256; i++) color_host[i] = exp(-(i * i) / (2 * sigma_color * sigma_color));
    return SMT_OK;
}

int smt_bilateral_filter_batch(const uint8_t *src, int images, int H, int W, int channels, int wsize_h, int wsize_w, const double *space,
                               const double *color, int norm, uint8_t *dst, double *acc, void *)
{
    ENTER();
    if (!src || !dst || !space || !color || src == dst || images < 0 || H <= 0 || W <= 0) return SMT_ERR_ARG;
    if ((channels != 1 && channels != 3) || wsize_h < 1 || wsize_h > 64 || wsize_w < 1 || wsize_w > 64) return SMT_ERR_ARG;
    if (norm != SMT_BILATERAL_NORM_RECIPROCAL && norm != SMT_BILATERAL_NORM_DIVIDE) return SMT_ERR_ARG;
    const size_t n = (size_t)images * H * W * channels;
    rd(src, n); rd(space, (size_t)wsize_h * wsize_w * 8); rd(color, 256 * 8);
    memset(dst, STUB_DST, n);
    if (acc) memset(acc, STUB_ACC, n * 8);
    g_last = StubCall{images, H, W, channels, wsize_h, wsize_w, norm, acc != nullptr};
    return SMT_OK;
}

}  // extern "C"
