// Host-only contract stub of the entries that host/smt_fill_holes.hpp calls (include/smt_fill_holes.h and the plumbing
// of include/smt.h), in the manner of tests/cpp_mirror_refine/refine_stub.cpp.  No HIP.  It fills nothing: "device"
// memory is malloc'ed with the exact byte count, the entry rejects what its header says it rejects, reads every byte of
// every input extent and fills every output extent with a byte that names the output, so under AddressSanitizer a mirror
// that sizes, uploads or downloads a buffer wrongly faults here.
#include "fill_holes_stub.hpp"

#include <cstdlib>
#include <cstring>

#include "../../include/smt_fill_holes.h"

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
bool stride_ok(size_t s, size_t n) { return s == 0 || s >= n; }
}  // namespace

const std::vector<std::string> &stub_log() { return g_log; }
void stub_log_clear() { g_log.clear(); }
void stub_fail(const char *entry) { g_fail = entry; }
int stub_live_allocs() { return g_allocs; }
const StubCall &stub_last_fill() { return g_last; }

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

int smt_fill_holes_batch(float *maps, const uint8_t *cls, int pairs, size_t map_stride, size_t cls_stride, int H, int W, float invalid,
                         int *status, void *)
{
    ENTER();
    if (!maps || !cls || pairs < 0 || H <= 0 || W <= 0 || H > SMT_FILLHOLES_MAX_DIM || W > SMT_FILLHOLES_MAX_DIM) return SMT_ERR_ARG;
    if (invalid != invalid) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    if (!stride_ok(map_stride, n) || !stride_ok(cls_stride, n)) return SMT_ERR_ARG;
    g_last = StubCall{pairs, H, W, invalid, status != nullptr, {}};
    for (int b = 0; b < pairs; b++) {
        float *m = maps + b * (map_stride ? map_stride : n);
        const uint8_t *c = cls + b * (cls_stride ? cls_stride : n);
        rd(m, n * 4);
        rd(c, n);
        g_last.cls.insert(g_last.cls.end(), c, c + n);
        memset(m, STUB_MAP, n * 4);
        if (status) memset(status + 4 * b, STUB_STATUS, 16);
    }
    return SMT_OK;
}

}  // extern "C"
