// Every public function of host/smt_refine.hpp against the contract stub, with exact-size heap buffers, under
// AddressSanitizer: the entry called with the sizes and parameters given, the stub's byte in every output element,
// untouched inputs, a std::runtime_error when an entry fails -- each in turn -- and nothing left allocated.  A
// stand-alone program; no GPU.
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "../../stereo_match_traditional_amd/host/smt_refine.hpp"
#include "refine_stub.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

namespace {
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

int calls(const char *fail)
{
    constexpr int H = 3, W = 5, D = 64;
    const size_t n = (size_t)H * W;
    auto disp = buf<float>(n, 0x11);
    auto aL = buf<int>(n, 1), aR = buf<int>(n, 2), aT = buf<int>(n, 3), aB = buf<int>(n, 4);
    auto cls = buf<unsigned char>(n, 1), gray = buf<unsigned char>(n, 9), state = buf<unsigned char>(n, 0xEE);
    auto status = buf<int>(4, 0xEE);
    smt_refine_params p = smt::RefineDefaultParams();
    REQUIRE(p.irv_ts == 20 && p.irv_th == 0.4f && p.irv_iters == 5 && p.search == 0);
    p.irv_ts = 7; p.irv_th = 0.25f; p.irv_iters = 2; p.search = 3;
    stub_log_clear();
    if (fail) stub_fail(fail);
    smt::RefineOutputs out;
    out.state = state.get(); out.status = status.get();
    smt::RegionVote(disp.get(), aL.get(), aR.get(), aT.get(), aB.get(), H, W, D, p, out);
    REQUIRE(called("smt_region_vote_batch"));
    {
        const StubCall &c = stub_last_refine();
        REQUIRE(c.pairs == 1 && c.H == H && c.W == W && c.D == D && c.irv_ts == 7 && c.irv_th == 0.25f && c.irv_iters == 2 && c.search == 3);
        REQUIRE(c.arms && !c.cls && c.state && c.status);
    }
    REQUIRE(all(disp.get(), n, STUB_MAP) && all(state.get(), n, STUB_STATE) && all(status.get(), 4, STUB_STATUS));
    REQUIRE(all(aL.get(), n, 1) && all(aR.get(), n, 2) && all(aT.get(), n, 3) && all(aB.get(), n, 4));
    memset(disp.get(), 0x11, n * 4);
    smt::InterpolateOutliers(disp.get(), cls.get(), gray.get(), H, W, D);           // defaults, no state, no status
    {
        const StubCall &c = stub_last_refine();
        REQUIRE(called("smt_interpolate_outliers_batch") && !c.arms && c.cls && !c.state && !c.status && c.irv_iters == 5 && c.search == 0);
    }
    REQUIRE(all(disp.get(), n, STUB_MAP) && all(cls.get(), n, 1) && all(gray.get(), n, 9));
    memset(disp.get(), 0x11, n * 4);
    memset(state.get(), 0xEE, n);
    smt::RefineOutputs only_state;
    only_state.state = state.get();
    smt::Refine(disp.get(), aL.get(), aR.get(), aT.get(), aB.get(), cls.get(), gray.get(), H, W, D, p, only_state);
    {
        const StubCall &c = stub_last_refine();
        REQUIRE(called("smt_refine_batch") && c.arms && c.cls && c.state && !c.status && c.irv_ts == 7);
    }
    REQUIRE(all(disp.get(), n, STUB_MAP) && all(state.get(), n, STUB_STATE));
    return 0;
}

// ArmMaps: a handle with the caller's tao and quirk bits, four maps of exactly row * col ints, the handle destroyed
int arms(const char *fail)
{
    constexpr int H = 3, W = 5;
    const size_t n = (size_t)H * W;
    auto img = buf<unsigned char>(n, 7);
    auto aL = buf<int>(n, 0xEE), aR = buf<int>(n, 0xEE), aT = buf<int>(n, 0xEE), aB = buf<int>(n, 0xEE);
    stub_log_clear();
    if (fail) stub_fail(fail);
    smt::ArmMaps(img.get(), H, W, 64, 25, SMT_QUIRK_FIX_RIGHT_ARM_STRIDE, aL.get(), aR.get(), aT.get(), aB.get());
    REQUIRE(called("smt_crossarm_create") && called("smt_crossarm_arms") && called("smt_crossarm_arm_maps"));
    REQUIRE(stub_last_arm_quirks() == SMT_QUIRK_FIX_RIGHT_ARM_STRIDE);
    for (size_t k = 0; k < n; k++) REQUIRE(aL[k] == 25 && aR[k] == 26 && aT[k] == 27 && aB[k] == 28);
    REQUIRE(all(img.get(), n, 7));
    std::vector<std::pair<int, int>> occ = {{0, 1}, {2, 4}}, mis = {{1, 0}};
    auto cls = buf<unsigned char>(n, 0xEE);
    smt::ClassMap(occ, mis, H, W, cls.get());
    for (size_t k = 0; k < n; k++) REQUIRE(cls[k] == (k == 1 || k == 14 ? 1 : k == 5 ? 2 : 0));
    bool thrown = false;
    mis.emplace_back(3, 0);                                            // a row the image does not have
    try { smt::ClassMap(occ, mis, H, W, cls.get()); } catch (const std::runtime_error &) { thrown = true; }
    REQUIRE(thrown);
    return 0;
}

// what the header rejects must come out as std::runtime_error, with nothing left behind
int rejected()
{
    auto disp = buf<float>(15, 2);
    auto a = buf<int>(15, 0);
    auto u = buf<unsigned char>(15, 0);
    smt_refine_params p = smt::RefineDefaultParams();
    int thrown = 0;
    try { smt::RegionVote(disp.get(), a.get(), a.get(), a.get(), a.get(), 0, 5, 16); } catch (const std::runtime_error &) { thrown++; }
    try { smt::RegionVote(disp.get(), a.get(), a.get(), a.get(), a.get(), 3, 5, 0); } catch (const std::runtime_error &) { thrown++; }
    try { smt::RegionVote(disp.get(), a.get(), a.get(), a.get(), a.get(), 3, 5, 513); } catch (const std::runtime_error &) { thrown++; }
    try { smt::RegionVote(disp.get(), a.get(), nullptr, a.get(), a.get(), 3, 5, 16); } catch (const std::runtime_error &) { thrown++; }
    p.irv_iters = 17;
    try { smt::RegionVote(disp.get(), a.get(), a.get(), a.get(), a.get(), 3, 5, 16, p); } catch (const std::runtime_error &) { thrown++; }
    p.irv_iters = 5; p.search = -1;
    try { smt::InterpolateOutliers(disp.get(), u.get(), u.get(), 3, 5, 16, p); } catch (const std::runtime_error &) { thrown++; }
    try { smt::InterpolateOutliers(disp.get(), nullptr, u.get(), 3, 5, 16); } catch (const std::runtime_error &) { thrown++; }
    try { smt::Refine(disp.get(), a.get(), a.get(), a.get(), a.get(), u.get(), nullptr, 3, 5, 16); } catch (const std::runtime_error &) { thrown++; }
    REQUIRE(thrown == 8 && all(disp.get(), 15, 2));
    return 0;
}

const char *const ENTRIES[] = {"smt_malloc", "smt_memcpy_h2d", "smt_region_vote_batch", "smt_memcpy_d2h", "smt_stream_sync"};
}  // namespace

int main()
{
    if (calls(nullptr) || arms(nullptr) || rejected()) return 1;
    REQUIRE(stub_live_allocs() == 0);
    for (const char *e : ENTRIES) {
        bool thrown = false;
        try { (void)calls(e); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "%s failed and nothing was thrown\n", e); return 1; }
        REQUIRE(stub_live_allocs() == 0);
    }
    for (const char *e : {"smt_malloc", "smt_memcpy_h2d", "smt_crossarm_create", "smt_crossarm_arms", "smt_crossarm_arm_maps", "smt_memcpy_d2h",
                          "smt_stream_sync"}) {
        bool thrown = false;
        try { (void)arms(e); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "%s failed in ArmMaps and nothing was thrown\n", e); return 1; }
        REQUIRE(stub_live_allocs() == 0);
    }
    printf("refine: contract held\n");
    return 0;
}
