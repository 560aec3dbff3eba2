// Every public function of host/smt_scan_views.hpp against the contract stub, with exact-size heap buffers, under
// AddressSanitizer: the entry called, the stub's byte in every output element, untouched inputs, a std::runtime_error
// when an entry fails -- each in turn -- and nothing left allocated.  A stand-alone program; no GPU.
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "../../stereo_match_traditional_amd/host/smt_scan_views.hpp"
#include "scan_views_stub.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

namespace {
constexpr int H = 3, W = 5, D = 7, P = 2;
constexpr size_t N = (size_t)H * W, V = N * D;

template <class T> std::unique_ptr<T[]> buf(size_t n, unsigned char fill)
{
    std::unique_ptr<T[]> p(new T[n]);
    memset(p.get(), fill, n * sizeof(T));
    return p;
}
template <class T> bool all(const T *p, size_t n, unsigned char byte)
{
    const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
    for (size_t k = 0; k < n * sizeof(T); k++)
        if (b[k] != byte) return false;
    return true;
}
bool called(const char *entry)
{
    for (const std::string &e : stub_log())
        if (e == entry) return true;
    return false;
}

int scanline(const char *fail)
{
    auto cL = buf<float>(V, 1), cR = buf<float>(V, 2), gL = buf<float>(N, 3), gR = buf<float>(N, 4);
    auto oL = buf<float>(V, 0xEE), dL = buf<float>(N, 0xEE), dR = buf<float>(N, 0xEE), dM = buf<float>(N, 0xEE);
    stub_log_clear();
    if (fail) stub_fail(fail);
    {
        smt::ScanlinePairOptimizer so;
        so.setQuirks(SMT_QUIRK_FIX_SCAN_VERTICAL);
        so.setSubpixel(1.0f);
        so.Initialize(H, W, D, 10, 150);
        so.ScanLinePair(cL.get(), gL.get(), cR.get(), gR.get(), oL.get(), dL.get(), nullptr, dR.get());   // the right view maps-only
        so.ScanLineMap(cR.get(), gR.get(), dM.get());
        so.Initialize(H, W, D, 10, 150);                                                                    // a second handle, the first destroyed
        so.ScanLinePair(cL.get(), gL.get(), cR.get(), gR.get(), oL.get(), nullptr, nullptr, dR.get());
    }
    REQUIRE(called("smt_scanline_run_pair") && called("smt_scanline_run_map") && called("smt_scanline_set_quirks") && called("smt_scanline_set_subpixel"));
    REQUIRE(all(oL.get(), V, STUB_VOUT_L) && all(dL.get(), N, STUB_DISP_L) && all(dR.get(), N, STUB_DISP_R) && all(dM.get(), N, STUB_DISP_L));
    REQUIRE(all(cL.get(), V, 1) && all(cR.get(), V, 2) && all(gL.get(), N, 3) && all(gR.get(), N, 4));
    return 0;
}

int pipeline(const char *fail)
{
    auto L = buf<unsigned char>(N * P, 5), R = buf<unsigned char>(N * P, 6), cls = buf<unsigned char>(N * P, 0xEE);
    auto dl = buf<float>(N * P, 0xEE), dr = buf<float>(N * P, 0xEE), sum = buf<float>(V, 0xEE);
    stub_log_clear();
    if (fail) stub_fail(fail);
    {
        smt::ScanViewsPipeline pipe(H, W, D);
        pipe.setQuirks(SMT_QUIRK_FIX_ALL);
        pipe.setSubpixel(0.5f);
        pipe.RunBatch(L.get(), R.get(), P, dl.get(), dr.get(), cls.get());
        REQUIRE(all(dr.get(), N * P, STUB_DISP_R));
        pipe.ScanRightVolume(sum.get());
        pipe.setScanViews(SMT_VIEW_LEFT);
        pipe.RunBatch(L.get(), R.get(), P, nullptr, dr.get(), nullptr);
        REQUIRE(all(dr.get(), N * P, STUB_DISP_R_LEFT));
    }
    REQUIRE(called("smt_pipeline_set_scan_views") && called("smt_pipeline_scan_right_volume") && called("smt_pipeline_run_batch"));
    REQUIRE(all(dl.get(), N * P, STUB_DISP_L) && all(cls.get(), N * P, STUB_CLS) && all(sum.get(), V, STUB_VOUT_R));
    REQUIRE(all(L.get(), N * P, 5) && all(R.get(), N * P, 6));
    return 0;
}

// what the headers reject must come out as std::runtime_error, with nothing left behind
int rejected()
{
    int thrown = 0;
    try { smt::ScanViewsPipeline pipe(H, W, D, SMT_VIEW_RIGHT); } catch (const std::runtime_error &) { thrown++; }
    try { smt::ScanViewsPipeline pipe(H, W, D, SMT_VIEW_LEFT); auto s = buf<float>(V, 0); pipe.ScanRightVolume(s.get()); }
    catch (const std::runtime_error &) { thrown++; }
    try {
        smt::ScanlinePairOptimizer so;
        so.Initialize(H, W, D, 10, 150);
        auto c = buf<float>(V, 1), g = buf<float>(N, 1), d = buf<float>(N, 0);
        so.ScanLinePair(c.get(), g.get(), c.get(), g.get(), nullptr, nullptr, nullptr, d.get());   // a view with neither output
    } catch (const std::runtime_error &) { thrown++; }
    REQUIRE(thrown == 3);
    return 0;
}

const char *const SCAN_ENTRIES[] = {"smt_scanline_create", "smt_scanline_set_quirks", "smt_scanline_set_subpixel", "smt_malloc", "smt_memcpy_h2d",
                                    "smt_scanline_run_pair", "smt_scanline_run_map", "smt_memcpy_d2h", "smt_stream_sync"};
const char *const PIPE_ENTRIES[] = {"smt_pipeline_create", "smt_pipeline_set_scan_views", "smt_pipeline_set_quirks", "smt_pipeline_set_subpixel",
                                    "smt_malloc", "smt_memcpy_h2d", "smt_pipeline_run_batch", "smt_pipeline_status", "smt_memcpy_d2h",
                                    "smt_stream_sync", "smt_pipeline_scan_right_volume"};

template <size_t K> int failing(int (*family)(const char *), const char *const (&entries)[K])
{
    for (const char *e : entries) {
        bool thrown = false;
        try { (void)family(e); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "%s failed and nothing was thrown\n", e); return 1; }
        REQUIRE(stub_live_allocs() == 0 && stub_live_handles() == 0);
    }
    return 0;
}
}  // namespace

int main()
{
    if (scanline(nullptr) || pipeline(nullptr) || rejected()) return 1;
    REQUIRE(stub_live_allocs() == 0 && stub_live_handles() == 0);
    if (failing(scanline, SCAN_ENTRIES) || failing(pipeline, PIPE_ENTRIES)) return 1;
    printf("scan views: contract held\n");
    return 0;
}
