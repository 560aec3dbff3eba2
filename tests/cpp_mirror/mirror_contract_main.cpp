// Every public function and method of host/smt_host.hpp, run against the contract stub (smt_contract_stub.cpp) under
// AddressSanitizer: exact-size heap buffers on the host side, exact-size "device" buffers on the stub's side.  After
// each call: the stub's log names the entry and its scalar arguments (rows against columns at H=3, W=5, D=4), every
// output byte carries the entry's pattern, every input is unchanged.  Then each function runs once per entry it calls
// with that entry failing: std::runtime_error, and no handle, device buffer or stream left behind.
//
//   mirror_contract_main <family>     one family of CASES (see --list)
//   mirror_contract_main --list       "family name name ..." per line: what tests/test_cpp_mirror_cpu.py holds to the header
//   mirror_contract_main --wrong N    a deliberately wrong mini-mirror (1 short DevBuf, 2 long download, 3 leak on throw)
//
// The RCCL block (SMT_HOST_WITH_RCCL) needs rccl.h and a HIP runtime: it is left out here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>

#include "../../stereo_match_traditional_amd/host/smt_host.hpp"
#include "smt_contract_stub.hpp"

namespace {

constexpr int H = 3, W = 5, D = 4;
constexpr size_t N = (size_t)H * W, V = N * D;
constexpr unsigned char PRE = 0xEE;

#define REQUIRE(c)                                                                      \
    do {                                                                                \
        if (!(c)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

// a caller buffer of exactly n elements on the heap: the allocator's redzones are its guards
template <class T> struct HB {
    explicit HB(size_t n, bool input = false) : n(n), p(static_cast<T *>(malloc(n * sizeof(T))))
    {
        unsigned char *b = bytes();
        for (size_t i = 0; i < n * sizeof(T); i++) b[i] = input ? (unsigned char)(i * 7 + 3) % 5 : PRE;
        if (input) keep.assign(b, b + n * sizeof(T));
    }
    ~HB() { free(p); }
    HB(const HB &) = delete;
    unsigned char *bytes() const { return reinterpret_cast<unsigned char *>(p); }
    bool all(unsigned char v) const { for (size_t i = 0; i < n * sizeof(T); i++) if (bytes()[i] != v) return false; return true; }
    bool untouched() const { return all(PRE); }
    bool same() const { return keep.size() == n * sizeof(T) && memcmp(keep.data(), p, keep.size()) == 0; }
    operator T *() const { return p; }
    size_t n;
    T *p;
    std::vector<unsigned char> keep;
};
template <class T> HB<T> in(size_t n) { return HB<T>(n, true); }

int count(const char *entry)
{
    int c = 0;
    for (const StubCall &k : stub_log()) c += k.entry == entry;
    return c;
}
const StubCall &call(const char *entry, int nth = 0)
{
    for (const StubCall &k : stub_log()) if (k.entry == entry && nth-- == 0) return k;
    fprintf(stderr, "no call of %s in the log\n", entry);
    exit(1);
}
bool ran(const char *entry, std::vector<long long> args, int nth = 0) { return call(entry, nth).args == args; }
unsigned char pat(const char *entry, int k = 0) { return stub_pattern(entry, k); }

bool throws(const std::function<void()> &f)
{
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}
void nothing_live()
{
    REQUIRE(stub_live_handles() == 0);
    REQUIRE(stub_live_allocs() == 0);
    REQUIRE(stub_live_streams() == 0);
}
// f builds everything it uses.  Once clean to learn which entries it calls, then once per entry with that entry failing.
void sweep(const char *what, const std::function<void()> &f)
{
    stub_log_clear();
    f();
    nothing_live();
    std::set<std::string> entries;
    for (const StubCall &k : stub_log()) entries.insert(k.entry);
    for (const std::string &e : entries) {
        if (e.find("destroy") != std::string::npos || e == "smt_free" || e == "smt_image_free") continue;   // not checked by the mirror
        stub_log_clear();
        stub_fail(e.c_str(), SMT_ERR_HIP);
        if (!throws(f)) { fprintf(stderr, "%s: no std::runtime_error when %s fails\n", what, e.c_str()); exit(1); }
        if (stub_live_handles() || stub_live_allocs() || stub_live_streams()) {
            fprintf(stderr, "%s: %d handles, %d buffers, %d streams left when %s fails\n", what, stub_live_handles(), stub_live_allocs(),
                    stub_live_streams(), e.c_str());
            exit(1);
        }
    }
    stub_log_clear();
}

// ------------------------------------------------------------------------------------------------ DevBuf, check
void f_devbuf()
{
    REQUIRE(throws([] { smt::check(SMT_ERR_ARG, "x"); }));
    smt::check(SMT_OK, "x");
    {
        smt::DevBuf<int> e;
        REQUIRE(e.get() == nullptr && e.size() == 0);
        smt::DevBuf<int> b(7);
        REQUIRE(b.size() == 7 && ran("smt_malloc", {28}));
        auto h = in<int>(7);
        HB<int> o(7);
        b.upload(h); b.download(o);
        REQUIRE(memcmp(h.p, o.p, 28) == 0 && h.same());
        b.resize(3);
        REQUIRE(b.size() == 3 && stub_live_allocs() == 1);
        smt::DevBuf<char> z(0);
        z.upload(nullptr); z.download(nullptr);
    }
    nothing_live();
    sweep("DevBuf", [] { smt::DevBuf<int> b(2); int x[2] = {1, 2}; b.upload(x); b.download(x); b.resize(4); });
    REQUIRE(throws([] { smt::batch_elems_(4, -1); }) && smt::batch_elems_(4, 0) == 0 && smt::batch_elems_(4, 3) == 12);
    int h = 0, w = 0;
    smt::inner_size_(7, 9, 2, h, w);
    REQUIRE(h == 3 && w == 5 && throws([&] { smt::inner_size_(4, 9, 2, h, w); }));
}

// ------------------------------------------------------------------------------------------------ AD_Census
void f_adcensus()
{
    auto L = in<float>(N), R = in<float>(N), L2 = in<float>(2 * N), R2 = in<float>(2 * N);
    {
        smt::AD_Census a;
        stub_log_clear();
        a.setQuirks(SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE);         // before Initialize: kept
        REQUIRE(count("smt_adcensus_set_quirks") == 0);
        a.Initialize(L, R, D, H, W, 10.f, 30.f);
        REQUIRE(ran("smt_adcensus_create", {H, W, D}) && ran("smt_adcensus_set_quirks", {SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE}));
        a.ComputeADcensus();
        REQUIRE(ran("smt_adcensus_compute", {SMT_VIEW_LEFT}));
        a.ComputeADcensusRight();
        REQUIRE(ran("smt_adcensus_compute", {SMT_VIEW_RIGHT}, 1));
        stub_log_clear();
        float *pl = a.GetPtrLeft(), *pr = a.GetPtrRight();
        REQUIRE(ran("smt_memcpy_d2h", {(long long)V * 4}) && ran("smt_memcpy_d2h", {(long long)V * 4}, 1) && count("smt_adcensus_status") == 2);
        for (size_t i = 0; i < V * 4; i++) {
            REQUIRE(reinterpret_cast<unsigned char *>(pl)[i] == pat("smt_adcensus_compute", 2));
            REQUIRE(reinterpret_cast<unsigned char *>(pr)[i] == pat("smt_adcensus_compute", 3));
        }
        stub_log_clear();
        REQUIRE(a.GetPtrLeft() == pl && a.GetPtrRight() == pr && count("smt_memcpy_d2h") == 0);   // cached
        REQUIRE(a.DevicePtrLeft() != a.DevicePtrRight());
        HB<float> dl(N), dr(N);
        stub_log_clear();
        a.WTA(dl, dr);
        REQUIRE(ran("smt_wta", {H, W, D}) && ran("smt_wta", {H, W, D}, 1) && dl.all(pat("smt_wta")) && dr.all(pat("smt_wta")));
        // a live object initialised again with other images and another size: nothing cached survives
        a.Initialize(L2, R2, D, H, 2 * W, 10.f, 30.f);
        a.ComputeADcensus(); a.ComputeADcensusRight();
        stub_log_clear();
        pl = a.GetPtrLeft(); pr = a.GetPtrRight();
        REQUIRE(count("smt_memcpy_d2h") == 2 && ran("smt_memcpy_d2h", {(long long)V * 8}) && ran("smt_memcpy_d2h", {(long long)V * 8}, 1));
        REQUIRE(reinterpret_cast<unsigned char *>(pl)[V * 8 - 1] == pat("smt_adcensus_compute", 2));
        // a compute invalidates the host copy of its view only
        a.ComputeADcensus();
        stub_log_clear();
        a.GetPtrLeft(); a.GetPtrRight();
        REQUIRE(count("smt_memcpy_d2h") == 1);
        a.setQuirks(0);
        REQUIRE(ran("smt_adcensus_set_quirks", {0}));
        REQUIRE(throws([&] { a.setQuirks(0x100); }));
    }
    REQUIRE(L.same() && R.same() && L2.same() && R2.same());
    nothing_live();
    REQUIRE(throws([] { smt::AD_Census a; a.ComputeADcensus(); }));       // before Initialize
    sweep("AD_Census", [&] {
        smt::AD_Census a;
        a.setQuirks(SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE);
        a.Initialize(L, R, D, H, W, 10.f, 30.f);
        a.ComputeADcensus(); a.ComputeADcensusRight();
        a.GetPtrLeft(); a.GetPtrRight();
        HB<float> dl(N), dr(N);
        a.WTA(dl, dr);
        a.Initialize(L, R, D, H, W, 10.f, 30.f);
    });
}

void f_multi()
{
    const int pairs = 3;
    auto L = in<float>(pairs * N), R = in<float>(pairs * N);
    HB<float> dl(pairs * N), dr(pairs * N);
    stub_log_clear();
    REQUIRE(smt::AD_Census_batch_all_devices(L, R, pairs, D, H, W, 10.f, 30.f, dl, dr) == 2);     // the stub has two devices
    REQUIRE(ran("smt_adcensus_create_on", {0, H, W, D}) && ran("smt_adcensus_create_on", {1, H, W, D}, 1));
    REQUIRE(ran("smt_adcensus_compute_batch", {2, SMT_VIEW_BOTH}) && ran("smt_adcensus_compute_batch", {1, SMT_VIEW_BOTH}, 1));
    REQUIRE(dl.all(pat("smt_adcensus_compute_batch", 0)) && dr.all(pat("smt_adcensus_compute_batch", 1)) && L.same() && R.same());
    REQUIRE(stub_log().back().entry == "smt_set_device" && stub_log().back().args == std::vector<long long>{0});
    nothing_live();
    HB<float> d1(N), d2(N);
    REQUIRE(smt::AD_Census_batch_all_devices(L, R, 1, D, H, W, 10.f, 30.f, d1, d2) == 1 && d1.all(pat("smt_adcensus_compute_batch", 0)));
    REQUIRE(smt::AD_Census_batch_all_devices(L, R, pairs, D, H, W, 10.f, 30.f, dl, dr, 1) == 1);
    REQUIRE(throws([&] { smt::AD_Census_batch_all_devices(L, R, 0, D, H, W, 10.f, 30.f, dl, dr); }));
    REQUIRE(throws([&] { smt::AD_Census_batch_all_devices(L, R, -1, D, H, W, 10.f, 30.f, dl, dr); }));
    nothing_live();
    sweep("AD_Census_batch_all_devices", [&] { smt::AD_Census_batch_all_devices(L, R, pairs, D, H, W, 10.f, 30.f, dl, dr); });
}

// ------------------------------------------------------------------------------------------------ CrossArmAggregation
void f_crossarm()
{
    auto img1 = in<unsigned char>(N), img3 = in<unsigned char>(3 * N);
    auto vol = in<float>(V);
    {
        smt::CrossArmAggregation c;
        c.setQuirks(SMT_QUIRK_FIX_STICKY_TAU);
        c.setSubpixel(0.5f);                          // before Initialize: kept
        stub_log_clear();
        c.Initialize(H, W, nullptr, nullptr, 31, D);
        REQUIRE(ran("smt_crossarm_create", {H, W, D, 31, 34, 17, SMT_QUIRK_FIX_STICKY_TAU}) && ran("smt_crossarm_set_subpixel", {500}));
        HB<float> out(V);
        REQUIRE(throws([&] { c.AggregationVertical(vol, out); }) && out.untouched());     // aggregate before arms: SMT_ERR_STATE
        c.ComputeArmLengths(img3, 3);
        REQUIRE(ran("smt_crossarm_arms", {3}) && ran("smt_memcpy_h2d", {(long long)N * 3}, 1));
        stub_log_clear();
        c.ComputeLeftArmLength(img1, 1); c.ComputeRightArmLength(img1, 1); c.ComputeTopArmLength(img1, 1); c.ComputeButtonArmLength(img1, 1);
        REQUIRE(count("smt_crossarm_reset") == 1);
        for (int d = 0; d < 4; d++) REQUIRE(ran("smt_crossarm_arm_dir", {1, d}, d));
        stub_log_clear();
        c.AggregationVertical(vol, out);
        REQUIRE(ran("smt_crossarm_aggregate", {0, 0}) && out.all(pat("smt_crossarm_aggregate")) && count("smt_crossarm_status") == 1);
        HB<float> out2(V);
        stub_log_clear();
        c.Aggregation(vol, out2);
        REQUIRE(ran("smt_crossarm_aggregate", {2, 0}) && out2.all(pat("smt_crossarm_aggregate")));
        HB<float> disp(N);
        stub_log_clear();
        c.WTA(out, disp);
        REQUIRE(ran("smt_wta_subpixel", {H, W, D, 500}) && count("smt_wta") == 0 && disp.all(pat("smt_wta_subpixel")));
        c.setSubpixel(0.0f);
        REQUIRE(ran("smt_crossarm_set_subpixel", {-1}));
        HB<float> disp2(N);
        stub_log_clear();
        c.WTA(out, disp2);
        REQUIRE(ran("smt_wta", {H, W, D}) && count("smt_wta_subpixel") == 0 && disp2.all(pat("smt_wta")));
        // device form with the fused map
        smt::DevBuf<float> di(V), dn(V), dd(N);
        stub_log_clear();
        c.AggregationVerticalDevice(di.get(), dn.get(), dd.get());
        REQUIRE(ran("smt_crossarm_aggregate", {0, 1}));
        c.Initialize(W, H, nullptr, nullptr, 30, D);          // again, transposed: the started_ flag resets with it
        stub_log_clear();
        c.ComputeTopArmLength(img1, 1);
        REQUIRE(count("smt_crossarm_reset") == 1);
    }
    REQUIRE(img1.same() && img3.same() && vol.same());
    nothing_live();
    sweep("CrossArmAggregation", [&] {
        smt::CrossArmAggregation c;
        c.setSubpixel(1.0f);
        c.Initialize(H, W, nullptr, nullptr, 30, D);
        c.ComputeArmLengths(img3, 3);
        c.ComputeLeftArmLength(img1, 1);
        HB<float> out(V), disp(N);
        c.Aggregation(vol, out); c.AggregationVertical(vol, out); c.WTA(out, disp);
        c.setSubpixel(0.0f);
        c.WTA(out, disp);
    });
}

// ------------------------------------------------------------------------------------------------ ScanlineOptimizer
void f_scanline()
{
    auto vol = in<float>(V), g = in<float>(N);
    {
        smt::ScanlineOptimizer s;
        s.setQuirks(SMT_QUIRK_FIX_SCAN_VERTICAL);
        s.setSubpixel(0.25f);
        stub_log_clear();
        s.Initialize(H, W, D, nullptr, 10, 150);
        REQUIRE(ran("smt_scanline_create", {H, W, D, 10, 150}) && ran("smt_scanline_set_quirks", {SMT_QUIRK_FIX_SCAN_VERTICAL}) &&
                ran("smt_scanline_set_subpixel", {250}) && ran("smt_malloc", {(long long)V * 4}));
        s.ScanLine(vol, g);
        REQUIRE(ran("smt_scanline_run", {0}) && s.DeviceProcessedVolume() != nullptr);
        HB<float> d(N);
        stub_log_clear();
        s.WTA(d);
        REQUIRE(ran("smt_wta_subpixel", {H, W, D, 250}) && d.all(pat("smt_wta_subpixel")));
        s.setSubpixel(0.0f);
        HB<float> d2(N);
        stub_log_clear();
        s.WTA(d2);
        REQUIRE(ran("smt_wta", {H, W, D}) && d2.all(pat("smt_wta")));
        s.setQuirks(0);
        stub_log_clear();
        s.Initialize(W, H, D, nullptr, 1, 2);                   // again, transposed
        REQUIRE(ran("smt_scanline_create", {W, H, D, 1, 2}) && count("smt_scanline_set_quirks") == 0 && stub_live_handles() == 1);
    }
    REQUIRE(vol.same() && g.same());
    nothing_live();
    sweep("ScanlineOptimizer", [&] {
        smt::ScanlineOptimizer s;
        s.setQuirks(SMT_QUIRK_FIX_SCAN_VERTICAL);
        s.setSubpixel(1.0f);
        s.Initialize(H, W, D, nullptr, 10, 150);
        s.ScanLine(vol, g);
        HB<float> d(N);
        s.WTA(d);
        s.setSubpixel(0.0f);
        s.WTA(d);
    });
}

// ------------------------------------------------------------------------------------------------ PostProcessing.h
using List = std::vector<std::pair<int, int>>;
void f_post()
{
    // the stub's class map is i % 3: pixels 1, 4, 7, 10, 13 occluded, 2, 5, 8, 11, 14 mismatched
    auto dr = in<float>(N);
    {
        auto dl = in<float>(N);
        List occ{{9, 9}}, mis{{8, 8}, {7, 7}};
        stub_log_clear();
        smt::LeftRightConsistency(W, H, 2, dl, dr, occ, mis);
        REQUIRE(ran("smt_lrcheck", {H, W, 2, 0}) && ran("smt_lrcheck_lists", {H, W}) && dl.all(pat("smt_lrcheck")) && dr.same());
        REQUIRE(occ.size() == 5 && mis.size() == 5 && occ[0] == std::make_pair(0, 1) && mis[4] == std::make_pair(2, 4));   // cleared first
    }
    {
        auto dl = in<float>(N);
        HB<float> last(N);
        List occ{{9, 9}}, mis{{8, 8}, {7, 7}};
        stub_log_clear();
        smt::LeftAndRightConsistency(dl, dr, last, W, H, 1.5f, occ, mis);
        REQUIRE(ran("smt_lrcheck_variant", {H, W, 1500, 0}) && last.all(pat("smt_lrcheck_variant")) && dl.same() && dr.same());
        REQUIRE(occ.size() == 6 && mis.size() == 7 && occ[0] == std::make_pair(9, 9) && occ[1] == std::make_pair(0, 1) &&
                mis[1] == std::make_pair(7, 7) && mis[6] == std::make_pair(2, 4));                                          // appended
    }
    {   // FillTheHole: `mismatch` is replaced only when a third list came back, i.e. when it was not empty
        auto d = in<float>(N);
        List occ{{0, 1}, {1, 1}}, mis{{2, 2}};
        stub_log_clear();
        smt::FillTheHole(H, W, D, d, occ, mis);
        REQUIRE(ran("smt_fill_the_hole", {H, W, D, 2, 1, 1, 1}) && d.all(pat("smt_fill_the_hole")));
        REQUIRE(occ.size() == 2 && mis.size() == 1 && mis[0] == std::make_pair(H - 1, W - 1));
        List none, keep;
        auto d2 = in<float>(N);
        stub_log_clear();
        smt::FillTheHole(H, W, D, d2, none, keep);                   // both lists empty: data() of an empty vector with count 0
        REQUIRE(ran("smt_fill_the_hole", {H, W, D, 0, 0, 1, 1}) && d2.all(pat("smt_fill_the_hole")) && none.empty() && keep.empty());
        List occ3{{0, 0}};
        auto d3 = in<float>(N);
        smt::FillTheHole(H, W, D, d3, occ3, keep);
        REQUIRE(occ3.size() == 1 && keep.empty());
    }
    {
        const int pairs = 3;
        auto d = in<float>(pairs * N);
        auto cls = in<uint8_t>(pairs * N);
        std::vector<std::array<int, 4>> st;
        stub_log_clear();
        smt::FillTheHoleBatch(pairs, H, W, D, d, cls, st);
        REQUIRE(ran("smt_fill_the_hole_batch", {pairs, 0, 0, H, W, D, 1}) && d.all(pat("smt_fill_the_hole_batch")) && cls.same());
        REQUIRE(st.size() == 3);
        for (auto &s : st) for (int v : s) { unsigned char b[4]; memcpy(b, &v, 4); REQUIRE(b[0] == pat("smt_fill_the_hole_batch", 1) && b[3] == b[0]); }
        stub_log_clear();
        smt::FillTheHoleBatch(0, H, W, D, nullptr, nullptr, st);
        REQUIRE(st.empty() && stub_log().empty());
        st.resize(2);
        REQUIRE(throws([&] { smt::FillTheHoleBatch(-1, H, W, D, d, cls, st); }) && st.empty() && stub_log().empty());
    }
    nothing_live();
    sweep("LeftRightConsistency", [&] { auto dl = in<float>(N); List o, m; smt::LeftRightConsistency(W, H, 2, dl, dr, o, m); });
    sweep("LeftAndRightConsistency", [&] { auto dl = in<float>(N); HB<float> last(N); List o, m; smt::LeftAndRightConsistency(dl, dr, last, W, H, 2.f, o, m); });
    sweep("FillTheHole", [&] { auto d = in<float>(N); List o{{0, 0}}, m{{1, 1}}; smt::FillTheHole(H, W, D, d, o, m); });
    sweep("FillTheHoleBatch", [&] { auto d = in<float>(N); auto c = in<uint8_t>(N); std::vector<std::array<int, 4>> st; smt::FillTheHoleBatch(1, H, W, D, d, c, st); });
    {   // a failing entry leaves the caller's lists and map as they were
        auto dl = in<float>(N);
        List occ{{9, 9}}, mis{{8, 8}};
        stub_fail("smt_lrcheck_lists", SMT_ERR_HIP);
        REQUIRE(throws([&] { smt::LeftAndRightConsistency(dl, dr, HB<float>(N), W, H, 2.f, occ, mis); }) && occ.size() == 1 && mis.size() == 1);
        stub_fail("smt_fill_the_hole", SMT_ERR_REF_UB);
        REQUIRE(throws([&] { smt::FillTheHole(H, W, D, dl, occ, mis); }) && dl.same() && mis[0] == std::make_pair(8, 8));
    }
}

// ------------------------------------------------------------------------------------------------ CBLSM.h
smt::Image image(int rows, int cols, int ch)
{
    smt::Image im;
    im.rows = rows; im.cols = cols; im.channels = ch;
    im.data.resize((size_t)rows * cols * ch);
    im.data.shrink_to_fit();
    for (size_t i = 0; i < im.data.size(); i++) im.data[i] = (unsigned char)(i * 5 + 1);
    return im;
}
void f_cblsm()
{
    auto a = in<int>(N), b = in<int>(N), c = in<int>(N), d = in<int>(N), e = in<int>(N), f = in<int>(N);
    {
        HB<int> o0(V), o1(V), o2(V), o3(V);
        stub_log_clear();
        smt::chooseArmLengthLeft(a, b, c, d, D, o0, H, W);
        smt::chooseArmLengthRight(a, b, c, d, D, o1, H, W);
        smt::chooseArmLengthUp(a, b, c, d, e, f, D, o2, H, W);
        smt::chooseArmLengthDown(a, b, c, d, e, f, D, o3, H, W);
        REQUIRE(ran("smt_cblsm_choose_arm_length", {0, H, W, D, 0}, 0) && ran("smt_cblsm_choose_arm_length", {1, H, W, D, 0}, 1) &&
                ran("smt_cblsm_choose_arm_length", {2, H, W, D, 1}, 2) && ran("smt_cblsm_choose_arm_length", {3, H, W, D, 1}, 3));
        REQUIRE(o0.all(pat("smt_cblsm_choose_arm_length", 0)) && o1.all(pat("smt_cblsm_choose_arm_length", 1)) &&
                o2.all(pat("smt_cblsm_choose_arm_length", 2)) && o3.all(pat("smt_cblsm_choose_arm_length", 3)));
        REQUIRE(a.same() && b.same() && c.same() && d.same() && e.same() && f.same());
    }
    {   // ArmLength*: one handle per call, the map of the direction asked for
        const smt::Image g = image(H, W, 1), bgr = image(H, W, 3);
        void (*fn[4])(const smt::Image &, unsigned char, int *, int, int) = {smt::ArmLengthL, smt::ArmLengthR, smt::ArmLengthUp, smt::ArmLengthDown};
        for (int dir = 0; dir < 4; dir++) {
            HB<int> arm(N);
            stub_log_clear();
            fn[dir](dir & 1 ? bgr : g, 25, arm, 34, 17);
            REQUIRE(ran("smt_crossarm_create", {H, W, 1, 25, 34, 17, SMT_QUIRK_FIX_RIGHT_ARM_STRIDE}) &&
                    ran("smt_crossarm_arm_dir", {dir & 1 ? 3 : 1, dir}) && arm.all(pat("smt_crossarm_arm_dir", dir)));
            nothing_live();
        }
        smt::Image bad = image(H, W, 1);
        bad.data.resize(N - 1);
        HB<int> arm(N);
        stub_log_clear();
        REQUIRE(throws([&] { smt::ArmLengthL(bad, 25, arm, 34, 17); }) && arm.untouched() && stub_log().empty());
        sweep("ArmLength", [&] { HB<int> m(N); smt::ArmLengthL(g, 25, m, 34, 17); smt::ArmLengthDown(bgr, 25, m, 34, 17); });
    }
    {
        auto L = in<unsigned char>(N), R = in<unsigned char>(N);
        HB<float> v0(V), v1(V);
        stub_log_clear();
        smt::ComputeAD(W, H, D, L, R, v0);
        smt::ComputeADRight(W, H, D, L, R, v1);
        REQUIRE(ran("smt_cblsm_ad", {H, W, D, SMT_VIEW_LEFT}) && ran("smt_cblsm_ad", {H, W, D, SMT_VIEW_RIGHT}, 1));
        REQUIRE(v0.all(pat("smt_cblsm_ad")) && v1.all(pat("smt_cblsm_ad")) && L.same() && R.same());
        sweep("ComputeAD", [&] { HB<float> v(V); smt::ComputeAD(W, H, D, L, R, v); smt::ComputeADRight(W, H, D, L, R, v); });
    }
    {   // ComputeDisp*: padded images, unpadded sizes
        const int ws = 1, w = ws + 1;
        const smt::Image Lp = image(H + 2 * w, W + 2 * w, 1), Rp = image(H + 2 * w, W + 2 * w, 1);
        const smt::Image L3 = image(H + 2 * w, W + 2 * w, 3), R3 = image(H + 2 * w, W + 2 * w, 3);
        HB<float> v0(V), v1(V), v2(V);
        stub_log_clear();
        smt::ComputeDispLeft(v0, Lp, Rp, ws, D, H, W);
        smt::ComputeDispRight(v1, Lp, Rp, ws, D, H, W);
        smt::ComputeDispV4(v2, L3, R3, ws, D, H, W);
        for (int k = 0; k < 3; k++) REQUIRE(ran("smt_cblsm_window_cost_batch", {1, 0, H, W, D, ws, k + 1, 0}, k));
        REQUIRE(v0.all(pat("smt_cblsm_window_cost_batch")) && v1.all(pat("smt_cblsm_window_cost_batch")) && v2.all(pat("smt_cblsm_window_cost_batch")));
        // wrong padding, wrong channels, a short vector, and the right view's read before its buffer: a throw, no device work
        HB<float> v(V);
        stub_log_clear();
        REQUIRE(throws([&] { smt::ComputeDispLeft(v, Lp, Rp, ws + 1, D, H, W); }));
        REQUIRE(throws([&] { smt::ComputeDispLeft(v, Lp, Rp, ws, D, W, H); }));
        REQUIRE(throws([&] { smt::ComputeDispLeft(v, L3, R3, ws, D, H, W); }));
        REQUIRE(throws([&] { smt::ComputeDispV4(v, Lp, Rp, ws, D, H, W); }));
        REQUIRE(throws([&] { smt::ComputeDispRight(v, Lp, image(H + 2 * w, W + 2 * w + 1, 1), ws, D, H, W); }));
        smt::Image shortL = Lp;
        shortL.data.pop_back();
        REQUIRE(throws([&] { smt::ComputeDispLeft(v, shortL, Rp, ws, D, H, W); }));
        const int ws2 = W - 1;                                              // _col_ <= winsize + 1
        const smt::Image Lw = image(H + 2 * (ws2 + 1), W + 2 * (ws2 + 1), 1);
        REQUIRE(throws([&] { smt::ComputeDispRight(v, Lw, Lw, ws2, D, H, W); }));
        REQUIRE(v.untouched() && stub_log().empty());
        smt::ComputeDispLeft(v, Lw, Lw, ws2, D, H, W);                      // the left view has no such read
        REQUIRE(v.all(pat("smt_cblsm_window_cost_batch")));
        sweep("ComputeDisp", [&] { HB<float> o(V); smt::ComputeDispLeft(o, Lp, Rp, ws, D, H, W); smt::ComputeDispV4(o, L3, R3, ws, D, H, W); });
    }
    {   // V5 (arm maps) and V4 (arm volumes)
        auto vol = in<float>(V);
        HB<float> out(V);
        stub_log_clear();
        smt::costAggregationV5(vol, out, a, b, c, d, D, H, W, 0);
        REQUIRE(ran("smt_crossarm_create", {H, W, D, 25, 34, 17, SMT_QUIRK_FIX_RIGHT_ARM_STRIDE}) && ran("smt_crossarm_aggregate", {1, 0}) &&
                out.all(pat("smt_crossarm_aggregate")) && vol.same());
        nothing_live();
        auto va = in<int>(V), vb = in<int>(V), vc = in<int>(V), vd = in<int>(V);
        HB<float> out4(V);
        stub_log_clear();
        smt::costAggregationV4(vol, out4, va, vb, vc, vd, D, H, W, 0);
        REQUIRE(ran("smt_cblsm_cost_aggregation_v4", {H, W, D, 0, 1}) && out4.all(pat("smt_cblsm_cost_aggregation_v4")));
        REQUIRE(vol.same() && va.same() && vb.same() && vc.same() && vd.same());
        HB<float> out5(V);
        stub_flag("smt_cblsm_cost_aggregation_v4");                         // a rectangle left the plane: throw, volume still written
        REQUIRE(throws([&] { smt::costAggregationV4(vol, out5, va, vb, vc, vd, D, H, W, 0); }) && out5.all(pat("smt_cblsm_cost_aggregation_v4")));
        sweep("costAggregationV5", [&] { HB<float> o(V); smt::costAggregationV5(vol, o, a, b, c, d, D, H, W, 0); });
        sweep("costAggregationV4", [&] { HB<float> o(V); smt::costAggregationV4(vol, o, va, vb, vc, vd, D, H, W, 0); });
        HB<float> d0(N), d1(N), d2(N);
        stub_log_clear();
        smt::ComputeDispOringin(vol, d0, D, H, W);
        smt::WTASubpixel(vol, d1, D, H, W);
        smt::WTASubpixel(vol, d2, D, H, W, 0.125f);
        REQUIRE(ran("smt_wta", {H, W, D}) && ran("smt_wta_subpixel", {H, W, D, 1000}) && ran("smt_wta_subpixel", {H, W, D, 125}, 1));
        REQUIRE(d0.all(pat("smt_wta")) && d1.all(pat("smt_wta_subpixel")) && d2.all(pat("smt_wta_subpixel")) && vol.same());
        HB<float> d3(N);
        REQUIRE(throws([&] { smt::WTASubpixel(vol, d3, D, H, W, 0.0f); }) && d3.untouched());
        sweep("WTA", [&] { HB<float> o(N); smt::ComputeDispOringin(vol, o, D, H, W); smt::WTASubpixel(vol, o, D, H, W); });
    }
    {   // CBLSMFlow
        const int pairs = 3;
        auto L = in<unsigned char>(pairs * N), R = in<unsigned char>(pairs * N);
        {
            smt::CBLSMFlow fl(H, W, D);
            REQUIRE(ran("smt_cblsm_flow_create_on", {0, H, W, D}));
            HB<float> dl(pairs * N), dr(pairs * N);
            stub_log_clear();
            fl.run(L, R, pairs, dl, dr);
            REQUIRE(ran("smt_cblsm_flow_run_batch", {pairs}) && dl.all(pat("smt_cblsm_flow_run_batch", 0)) && dr.all(pat("smt_cblsm_flow_run_batch", 1)));
            HB<float> wl(pairs * N);
            stub_log_clear();
            fl.runWindow(L, R, pairs, 2, wl, nullptr);
            REQUIRE(ran("smt_cblsm_flow_run_batch_window", {pairs, 2}) && wl.all(pat("smt_cblsm_flow_run_batch_window", 0)));
            fl.run(L, R, pairs, nullptr, nullptr);
            fl.run(L, R, 0, nullptr, nullptr);
            HB<float> u(pairs * N);
            REQUIRE(throws([&] { fl.run(L, R, -1, u, u); }) && throws([&] { fl.runWindow(L, R, 1, W, u, u); }) && u.untouched());
        }
        REQUIRE(L.same() && R.same());
        nothing_live();
        sweep("CBLSMFlow", [&] { smt::CBLSMFlow fl(H, W, D); HB<float> o(N), p(N); fl.run(L, R, 1, o, p); fl.runWindow(L, R, 1, 1, o, p); });
    }
}

// ------------------------------------------------------------------------------------------------ CrossAggregator
void f_crossagg()
{
    auto img = in<uint8_t>(3 * N);
    auto cost = in<float>(V);
    {
        smt::CrossAggregator c;
        stub_log_clear();
        c.Aggregate(4);                                   // before Initialize: returns, like the reference (:91-93)
        REQUIRE(stub_log().empty() && c.get_cost_ptr() == nullptr);
        c.SetParams(20, 10, 15, 5);                       // before Initialize: the reference keeps the four values
        REQUIRE(stub_log().empty());
        REQUIRE(!c.Initialize(W, H, 3, 3));               // empty range: false
        REQUIRE(ran("smt_crossagg_create", {W, H, 0}) && c.get_cost_ptr() == nullptr);
        c.Aggregate(4);
        REQUIRE(count("smt_crossagg_aggregate") == 0);
        stub_log_clear();
        REQUIRE(c.Initialize(W, H, 2, 2 + D));
        REQUIRE(ran("smt_crossagg_create", {W, H, D}) && ran("smt_crossagg_set_params", {20, 10, 15, 5}));
        REQUIRE(c.get_cost_ptr() != nullptr && c.get_arms_ptr()[N - 1].bottom == 0);          // :34-35, :52: allocated by Initialize
        REQUIRE(throws([&] { c.Aggregate(4); }) && count("smt_crossagg_aggregate") == 0);     // no SetData yet
        c.SetData(img, nullptr, cost);
        stub_log_clear();
        c.Aggregate(4);
        REQUIRE(ran("smt_crossagg_aggregate", {4}) && ran("smt_memcpy_d2h", {(long long)V * 4}) && ran("smt_memcpy_d2h", {(long long)N * 4}, 1));
        const unsigned char *pc = reinterpret_cast<unsigned char *>(c.get_cost_ptr()), *pa = reinterpret_cast<unsigned char *>(c.get_arms_ptr());
        for (size_t i = 0; i < V * 4; i++) REQUIRE(pc[i] == pat("smt_crossagg_aggregate", 0));
        for (size_t i = 0; i < N * 4; i++) REQUIRE(pa[i] == pat("smt_crossagg_aggregate", 1));
        c.SetParams(34, 17, 20, 6);
        REQUIRE(ran("smt_crossagg_set_params", {34, 17, 20, 6}));
        // again at another size: the parameters hold, the buffers follow the size
        auto img2 = in<uint8_t>(3 * 2 * N);
        auto cost2 = in<float>(2 * N * 2);
        stub_log_clear();
        REQUIRE(c.Initialize(2 * W, H, 0, 2));
        REQUIRE(ran("smt_crossagg_create", {2 * W, H, 2}) && ran("smt_crossagg_set_params", {34, 17, 20, 6}) && stub_live_handles() == 1);
        c.SetData(img2, nullptr, cost2);
        c.Aggregate(1);
        REQUIRE(ran("smt_memcpy_d2h", {(long long)2 * N * 2 * 4}) && img2.same() && cost2.same());
        REQUIRE(reinterpret_cast<unsigned char *>(c.get_cost_ptr())[2 * N * 2 * 4 - 1] == pat("smt_crossagg_aggregate", 0));
        REQUIRE(throws([&] { c.SetParams(-1, 0, 0, 0); }));
    }
    REQUIRE(img.same() && cost.same());
    nothing_live();
    sweep("CrossAggregator", [&] {
        smt::CrossAggregator c;
        c.SetParams(1, 2, 3, 4);
        if (!c.Initialize(W, H, 0, D)) throw std::runtime_error("Initialize");
        c.SetData(img, nullptr, cost);
        c.SetParams(34, 17, 20, 6);
        c.Aggregate(2);
    });
}

// ------------------------------------------------------------------------------------------------ SAD
void f_sad()
{
    const int ws = 1, w = ws + 1, rows = H + 2 * w, cols = W + 2 * w;
    auto Lp = in<unsigned char>((size_t)rows * cols), Rp = in<unsigned char>((size_t)rows * cols);
    HB<int> d0(N), d1(N), d2(N), bl(N), br(N);
    stub_log_clear();
    smt::GetPointDepthLeft(d0, Lp, Rp, rows, cols, D, ws);
    smt::GetPointDepthRight(d1, Lp, Rp, rows, cols, D, ws);
    smt::GetPointDepth(d2, Lp, Rp, rows, cols, D, ws, false);
    smt::GetPointDepthBoth(bl, br, Lp, Rp, rows, cols, D, ws);
    REQUIRE(ran("smt_sad", {H, W, D, ws, SMT_VIEW_LEFT}) && ran("smt_sad", {H, W, D, ws, SMT_VIEW_RIGHT}, 1) && ran("smt_sad", {H, W, D, ws, SMT_VIEW_RIGHT}, 2));
    REQUIRE(ran("smt_sad_both", {H, W, D, ws, 0}) && d0.all(pat("smt_sad")) && d1.all(pat("smt_sad")) && d2.all(pat("smt_sad")));
    REQUIRE(bl.all(pat("smt_sad_both", 0)) && br.all(pat("smt_sad_both", 1)) && Lp.same() && Rp.same());
    HB<int> u(N);
    stub_log_clear();
    REQUIRE(throws([&] { smt::GetPointDepthLeft(u, Lp, Rp, 2 * w, cols, D, ws); }) && throws([&] { smt::GetPointDepthBoth(u, u, Lp, Rp, rows, 2 * w, D, ws); }));
    REQUIRE(u.untouched() && stub_log().empty());
    sweep("GetPointDepth", [&] { HB<int> a(N), b(N); smt::GetPointDepthLeft(a, Lp, Rp, rows, cols, D, ws); smt::GetPointDepthBoth(a, b, Lp, Rp, rows, cols, D, ws); });
    const int pairs = 3;
    auto L = in<unsigned char>(pairs * N), R = in<unsigned char>(pairs * N);
    {
        smt::SadFlow f(H, W, D, 2);
        REQUIRE(ran("smt_sad_flow_create_on", {0, H, W, D, 2}));
        HB<int> a(pairs * N), b(pairs * N), c(pairs * N);
        stub_log_clear();
        f.run(L, R, pairs, a, b, c);
        REQUIRE(ran("smt_sad_flow_run_batch", {pairs}) && a.all(pat("smt_sad_flow_run_batch", 0)) && b.all(pat("smt_sad_flow_run_batch", 1)) &&
                c.all(pat("smt_sad_flow_run_batch", 2)));
        f.run(L, R, pairs, nullptr, nullptr, nullptr);
        f.run(L, R, 0, nullptr, nullptr, nullptr);
        HB<int> v(pairs * N);
        REQUIRE(throws([&] { f.run(L, R, -1, v, v, v); }) && v.untouched());
        smt::SadFlow g(H, W, D);
        REQUIRE(ran("smt_sad_flow_create_on", {0, H, W, D, 3}));
    }
    REQUIRE(L.same() && R.same() && throws([] { smt::SadFlow f(H, W, 0); }));
    nothing_live();
    sweep("SadFlow", [&] { smt::SadFlow f(H, W, D); HB<int> a(N), b(N), c(N); f.run(L, R, 1, a, b, c); });
}

// ------------------------------------------------------------------------------------------------ NCC
void f_ncc()
{
    auto L = in<unsigned char>(N), R = in<unsigned char>(N);
    const int pairs = 3;
    auto Lb = in<unsigned char>(pairs * N), Rb = in<unsigned char>(pairs * N);
    {
        HB<int> d(N);
        stub_log_clear();
        smt::NCC_algorithem(L, R, W, H, d, 1, D);
        REQUIRE(ran("smt_ncc", {H, W, D, 1, 0}) && d.all(pat("smt_ncc")));
        sweep("NCC_algorithem", [&] { HB<int> o(N); smt::NCC_algorithem(L, R, W, H, o, 1, D); });
    }
    {
        smt::NCCFlow f(H, W, D, 2);
        REQUIRE(ran("smt_ncc_flow_create_on", {0, H, W, D, 2}));
        f.set_form(SMT_NCC_FORM_BOX);
        REQUIRE(ran("smt_ncc_flow_set_form", {SMT_NCC_FORM_BOX}) && throws([&] { f.set_form(9); }));
        HB<int> d(pairs * N);
        stub_log_clear();
        f.run(Lb, Rb, pairs, d);
        REQUIRE(ran("smt_ncc_flow_run_batch", {pairs, 0}) && d.all(pat("smt_ncc_flow_run_batch")));
        HB<int> a(pairs * N), b(pairs * N), c(pairs * N);
        HB<unsigned char> cls(pairs * N);
        stub_log_clear();
        f.runBoth(Lb, Rb, pairs, a, b, c, cls);
        REQUIRE(ran("smt_lrncc_flow_run_batch", {pairs}) && a.all(pat("smt_lrncc_flow_run_batch", 0)) && b.all(pat("smt_lrncc_flow_run_batch", 1)) &&
                c.all(pat("smt_lrncc_flow_run_batch", 2)) && cls.all(pat("smt_lrncc_flow_run_batch", 3)));
        f.runBoth(Lb, Rb, pairs, nullptr, nullptr, nullptr, nullptr);
        f.runBoth(Lb, Rb, 0, nullptr, nullptr, nullptr, nullptr);
        f.run(Lb, Rb, 0, nullptr);
        HB<int> v(pairs * N);
        REQUIRE(throws([&] { f.run(Lb, Rb, -1, v); }) && throws([&] { f.runBoth(Lb, Rb, -1, v, v, v, nullptr); }) && v.untouched());
    }
    nothing_live();
    sweep("NCCFlow", [&] { smt::NCCFlow f(H, W, D); f.set_form(0); HB<int> a(N), b(N), c(N); HB<unsigned char> k(N); f.run(L, R, 1, a); f.runBoth(L, R, 1, a, b, c, k); });
    {   // ncc(): the whole-image matcher
        HB<unsigned char> dep(N), dep2(N), dep3(N);
        HB<int> off(N);
        stub_log_clear();
        smt::ncc(L, R, H, W, "left", dep, false, 1, W);
        smt::ncc(L, R, H, W, "right", dep2, true, 2, 4, off);
        REQUIRE(ran("smt_whole_ncc", {H, W, 1, W, 0, SMT_VIEW_LEFT, 1, 0}) && ran("smt_whole_ncc", {H, W, 2, 4, 1, SMT_VIEW_RIGHT, 1, 0}, 1));
        REQUIRE(dep.all(pat("smt_whole_ncc", 0)) && dep2.all(pat("smt_whole_ncc", 0)) && off.all(pat("smt_whole_ncc", 1)) && L.same() && R.same());
        stub_log_clear();
        REQUIRE(throws([&] { smt::ncc(L, R, H, W, "both", dep3); }) && stub_log().empty());
        REQUIRE(throws([&] { smt::ncc(L, R, H, W, "left", dep3); }) && dep3.untouched());     // the default max_offset 79 > W: SMT_ERR_REF_UB
        sweep("ncc", [&] { HB<unsigned char> o(N); HB<int> f(N); smt::ncc(L, R, H, W, "left", o, false, 1, 2, f); });
        auto bgr = in<unsigned char>(3 * N);
        HB<unsigned char> grey(N);
        stub_log_clear();
        smt::bgr_to_grey(bgr, H, W, grey);
        REQUIRE(ran("smt_bgr_to_grey_batch", {1, H, W}) && grey.all(pat("smt_bgr_to_grey_batch")) && bgr.same());
        sweep("bgr_to_grey", [&] { HB<unsigned char> o(N); smt::bgr_to_grey(bgr, H, W, o); });
    }
    {
        smt::NCCWholeFlow f(H, W, 2, 4, true);
        REQUIRE(ran("smt_whole_ncc_flow_create_on", {0, H, W, 2, 4, 1}));
        f.set_form(SMT_NCC_WHOLE_FORM_LOOP);
        REQUIRE(ran("smt_whole_ncc_flow_set_form", {SMT_NCC_WHOLE_FORM_LOOP}) && throws([&] { f.set_form(7); }));
        HB<unsigned char> a(pairs * N), b(pairs * N);
        HB<int> c(pairs * N), d(pairs * N), e(pairs * N);
        stub_log_clear();
        f.run(Lb, Rb, pairs, a, b, c, d, e);
        REQUIRE(ran("smt_whole_ncc_flow_run_batch", {pairs}));
        REQUIRE(a.all(pat("smt_whole_ncc_flow_run_batch", 0)) && b.all(pat("smt_whole_ncc_flow_run_batch", 1)) && c.all(pat("smt_whole_ncc_flow_run_batch", 2)) &&
                d.all(pat("smt_whole_ncc_flow_run_batch", 3)) && e.all(pat("smt_whole_ncc_flow_run_batch", 4)));
        f.run(Lb, Rb, pairs, nullptr, nullptr, nullptr, nullptr, nullptr);
        f.run(Lb, Rb, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
        HB<int> v(pairs * N);
        REQUIRE(throws([&] { f.run(Lb, Rb, -1, nullptr, nullptr, v, v, v); }) && v.untouched());
        REQUIRE(throws([] { smt::NCCWholeFlow g(H, W); }));                                   // 79 > W
    }
    REQUIRE(Lb.same() && Rb.same());
    nothing_live();
    sweep("NCCWholeFlow", [&] { smt::NCCWholeFlow f(H, W, 1, 2); f.set_form(0); HB<unsigned char> a(N), b(N); HB<int> c(N), d(N), e(N); f.run(L, R, 1, a, b, c, d, e); });
}

// ------------------------------------------------------------------------------------------------ ASW
void f_asw()
{
    const int ws = 1, w = ws + 1, rows = H + 2 * w, cols = W + 2 * w;
    auto Lp = in<unsigned char>((size_t)rows * cols), Rp = in<unsigned char>((size_t)rows * cols);
    std::vector<double> sp, cm;
    stub_log_clear();
    smt::getMasks(sp, cm, ws, 50.0, 30.0);
    REQUIRE(ran("smt_asw_masks", {ws}) && sp.size() == 25 && cm.size() == 256);
    HB<float> d0(N), d1(N), bl(N), br(N), cl(N), cr(N);
    HB<unsigned char> last(N);
    stub_log_clear();
    smt::AdaptiveSupportWeight(d0, Lp, Rp, rows, cols, ws, D, sp, cm, 40);
    smt::AdaptiveSupportWeight(d1, Lp, Rp, rows, cols, ws, D, sp, cm, 40, false);
    smt::AdaptiveSupportWeightBoth(bl, br, last, Lp, Rp, rows, cols, ws, D, sp, cm, 40);
    smt::AdaptiveSupportWeightBoth(cl, cr, nullptr, Lp, Rp, rows, cols, ws, D, sp, cm, 40);
    REQUIRE(ran("smt_asw", {H, W, D, ws, 40, SMT_VIEW_LEFT, 0}) && ran("smt_asw", {H, W, D, ws, 40, SMT_VIEW_RIGHT, 0}, 1));
    REQUIRE(ran("smt_asw_both", {H, W, D, ws, 40, 0, 0}) && ran("smt_asw_crosscheck", {H, W}) && count("smt_asw_crosscheck") == 1);
    REQUIRE(d0.all(pat("smt_asw")) && d1.all(pat("smt_asw")) && bl.all(pat("smt_asw_both", 0)) && br.all(pat("smt_asw_both", 1)) &&
            cl.all(pat("smt_asw_both", 0)) && cr.all(pat("smt_asw_both", 1)) && last.all(pat("smt_asw_crosscheck")) && Lp.same() && Rp.same());
    // masks of another window: smt_asw would read (2 winSize + 3)^2 doubles from a device buffer that holds fewer
    std::vector<double> small(9, 1.0), col255(255, 1.0);
    HB<float> u(N);
    stub_log_clear();
    REQUIRE(throws([&] { smt::AdaptiveSupportWeight(u, Lp, Rp, rows, cols, ws, D, small, cm, 40); }));
    REQUIRE(throws([&] { smt::AdaptiveSupportWeight(u, Lp, Rp, rows, cols, ws, D, sp, col255, 40); }));
    REQUIRE(throws([&] { smt::AdaptiveSupportWeightBoth(u, u, nullptr, Lp, Rp, rows, cols, ws, D, small, cm, 40); }));
    REQUIRE(throws([&] { smt::AdaptiveSupportWeight(u, Lp, Rp, 2 * w, cols, ws, D, sp, cm, 40); }));
    REQUIRE(u.untouched() && stub_log().empty());
    sweep("getMasks", [&] { std::vector<double> a, b; smt::getMasks(a, b, 2, 1.0, 1.0); });
    sweep("AdaptiveSupportWeight", [&] { HB<float> a(N); smt::AdaptiveSupportWeight(a, Lp, Rp, rows, cols, ws, D, sp, cm, 40); });
    sweep("AdaptiveSupportWeightBoth", [&] { HB<float> a(N), b(N); HB<unsigned char> c(N); smt::AdaptiveSupportWeightBoth(a, b, c, Lp, Rp, rows, cols, ws, D, sp, cm, 40); });
}

// ------------------------------------------------------------------------------------------------ post-filters
void f_filters()
{
    {
        auto a = in<float>(N);
        HB<float> o(N);
        stub_log_clear();
        smt::MedianFilter(a, o, W, H, 3);
        REQUIRE(ran("smt_median_filter", {W, H, 3}) && o.all(pat("smt_median_filter")) && a.same());
        auto b = in<float>(N), c = in<float>(N), d = in<float>(N);
        stub_log_clear();
        smt::MedianFilter(b, b, W, H, 3);                       // in == out: the in-place recurrence, not a rejection
        smt::MedianFilterInPlace(c, W, H, 5);
        REQUIRE(count("smt_median_filter") == 0 && ran("smt_median_filter_inplace", {W, H, 3}) && ran("smt_median_filter_inplace", {W, H, 5}, 1));
        REQUIRE(b.all(pat("smt_median_filter_inplace")) && c.all(pat("smt_median_filter_inplace")));
        REQUIRE(throws([&] { smt::MedianFilter(a, d, W, H, 9); }) && d.same());
        stub_log_clear();
        smt::RemoveSpeckles(d, W, H, 1, 30u, -5);
        REQUIRE(ran("smt_remove_speckles", {W, H, 1, 30, -5}) && d.all(pat("smt_remove_speckles")));
        sweep("MedianFilter", [&] { auto i = in<float>(N); HB<float> q(N); smt::MedianFilter(i, q, W, H, 3); smt::MedianFilter(i, i, W, H, 3); smt::RemoveSpeckles(q, W, H, 1, 2u, 3); });
    }
    {
        auto m = in<unsigned char>(N), m2 = in<unsigned char>(N);
        HB<int> cnt(2);
        stub_log_clear();
        smt::FillImageNew(m, H, W);
        smt::FillImageNew(m2, H, W, SMT_ASW_FIX_FILL_ROW_END, cnt);
        REQUIRE(ran("smt_fill_image_new_batch", {1, 0, H, W, 0, 1}) && ran("smt_fill_image_new_batch", {1, 0, H, W, SMT_ASW_FIX_FILL_ROW_END, 1}, 1));
        REQUIRE(m.all(pat("smt_fill_image_new_batch")) && m2.all(pat("smt_fill_image_new_batch")) && cnt.all(pat("smt_fill_image_new_batch", 1)));
        auto m3 = in<unsigned char>(N);
        REQUIRE(throws([&] { smt::FillImageNew(m3, H, W, 0x80u); }) && m3.same());
        sweep("FillImageNew", [&] { auto i = in<unsigned char>(N); HB<int> c(2); smt::FillImageNew(i, H, W, 0, c); });
    }
    {
        auto m = in<unsigned char>(N), m2 = in<unsigned char>(N), m3 = in<unsigned char>(N);
        HB<unsigned char> am(N), af(N);
        HB<int> cnt(2);
        smt_asw_post_params post = {0, 40, 2, 5, 3, 0};
        stub_log_clear();
        smt::ASWTail(m, H, W);
        smt::ASWTail(m2, H, W, am, af, &post, cnt);
        REQUIRE(ran("smt_asw_tail_batch", {1, 0, H, W, 0, 1, 1, 1, 1}) && ran("smt_asw_tail_batch", {1, 0, H, W, 1, 1, 1, 1, 1}, 1));
        REQUIRE(m.all(pat("smt_asw_tail_batch", 0)) && m2.all(pat("smt_asw_tail_batch", 0)) && am.all(pat("smt_asw_tail_batch", 1)) &&
                af.all(pat("smt_asw_tail_batch", 2)) && cnt.all(pat("smt_asw_tail_batch", 3)));
        stub_flag("smt_asw_tail_batch");                        // a speckle kernel hit its loop cap
        REQUIRE(throws([&] { smt::ASWTail(m3, H, W); }));
        nothing_live();
        sweep("ASWTail", [&] { auto i = in<unsigned char>(N); HB<unsigned char> a(N), b(N); HB<int> c(2); smt::ASWTail(i, H, W, a, b, nullptr, c); });
    }
}

// ------------------------------------------------------------------------------------------------ images
void f_image()
{
    stub_log_clear();
    const smt::Image bgr = smt::imread("x.png");
    REQUIRE(ran("smt_image_read", {3}) && bgr.rows == 2 && bgr.cols == 3 && bgr.channels == 3 && bgr.data.size() == 18 && count("smt_image_free") == 1);
    for (unsigned char b : bgr.data) REQUIRE(b == pat("smt_image_read"));
    const smt::Image g1 = smt::imread("x.png", 1);
    REQUIRE(g1.channels == 1 && g1.data.size() == 6);
    stub_log_clear();
    const smt::Image g = smt::cvtColorBGR2GRAY(bgr);
    REQUIRE(ran("smt_bgr2gray", {2, 3}) && g.rows == 2 && g.cols == 3 && g.channels == 1 && g.data.size() == 6);
    for (unsigned char b : g.data) REQUIRE(b == pat("smt_bgr2gray"));
    stub_log_clear();
    REQUIRE(throws([&] { smt::cvtColorBGR2GRAY(g); }));
    smt::Image bad = bgr;
    bad.data.pop_back();
    REQUIRE(throws([&] { smt::cvtColorBGR2GRAY(bad); }) && stub_log().empty());
    auto px = in<unsigned char>(3 * N);
    smt::imwrite("y.png", px, H, W, 3);
    REQUIRE(ran("smt_image_write", {H, W, 3}) && px.same() && throws([&] { smt::imwrite("y.png", px, H, W, 2); }));
    nothing_live();
    sweep("images", [&] { smt::Image i = smt::imread("x.png"); smt::cvtColorBGR2GRAY(i); smt::imwrite("y.png", i.data.data(), i.rows, i.cols, 3); });
}

// ------------------------------------------------------------------------------------------------ Pipeline
void f_pipeline()
{
    auto L = in<unsigned char>(3 * N), R = in<unsigned char>(3 * N);
    {
        smt_pipeline_params pp = {10.f, 30.f, 30, 10, 150, 2};
        smt::Pipeline p(H, W, D, &pp);
        REQUIRE(ran("smt_pipeline_create", {H, W, D, 1}));
        p.setQuirks(SMT_QUIRK_FIX_ALL);
        p.setSubpixel(1.0f);
        REQUIRE(ran("smt_pipeline_set_quirks", {SMT_QUIRK_FIX_ALL}) && ran("smt_pipeline_set_subpixel", {1000}));
        p.setSubpixel(0.0f);
        REQUIRE(ran("smt_pipeline_set_subpixel", {-1}, 1) && throws([&] { p.setQuirks(0x40); }) && throws([&] { p.setSubpixel(-1.0f); }));
        for (int pairs : {2, 1, 3}) {                           // one handle, batches of different sizes
            HB<float> dl(pairs * N), dr(pairs * N);
            HB<unsigned char> cls(pairs * N);
            stub_log_clear();
            p.RunBatch(L, R, pairs, dl, dr, cls);
            REQUIRE(ran("smt_pipeline_run_batch", {pairs, 0}) && ran("smt_memcpy_h2d", {(long long)(pairs * N)}) && count("smt_pipeline_status") == 1);
            REQUIRE(dl.all(pat("smt_pipeline_run_batch", 0)) && dr.all(pat("smt_pipeline_run_batch", 1)) && cls.all(pat("smt_pipeline_run_batch", 2)));
        }
        HB<float> only(3 * N);
        p.RunBatch(L, R, 3, only, nullptr, nullptr);            // null outputs, as the sibling flows take them
        REQUIRE(only.all(pat("smt_pipeline_run_batch", 0)));
        p.RunBatch(L, R, 3, nullptr, nullptr, nullptr);
        REQUIRE(throws([&] { p.RunBatch(L, R, 0, nullptr, nullptr, nullptr); }));      // smt_pipeline_run_batch has no empty batch
        HB<float> u(3 * N);
        stub_log_clear();
        REQUIRE(throws([&] { p.RunBatch(L, R, -1, u, u, nullptr); }) && u.untouched() && stub_log().empty());
        smt::Pipeline q(H, W, D);
        REQUIRE(ran("smt_pipeline_create", {H, W, D, 0}));
    }
    REQUIRE(L.same() && R.same() && throws([] { smt::Pipeline p(0, W, D); }));
    nothing_live();
    sweep("Pipeline", [&] {
        smt::Pipeline p(H, W, D);
        p.setQuirks(0); p.setSubpixel(1.0f);
        HB<float> a(N), b(N);
        HB<unsigned char> c(N);
        p.RunBatch(L, R, 1, a, b, c);
    });
}

// ------------------------------------------------------------------------------------------------ the wrong mini-mirrors
// What the checks above must be able to see.  Each is the shape of a mirror body with one mistake.
int wrong(int which)
{
    auto vol = in<float>(V);
    if (which == 1) {           // a DevBuf one element short
        smt::DevBuf<float> v(V - 1), d(N);
        smt::check(smt_memcpy_h2d(v.get(), vol, (V - 1) * 4, nullptr), "h2d");
        smt::check(smt_wta(v.get(), H, W, D, d.get(), nullptr), "smt_wta");
    } else if (which == 2) {    // a download of n * D elements into a buffer of n
        HB<float> disp(N);
        smt::DevBuf<float> v(V), d(V);
        v.upload(vol);
        smt::check(smt_wta(v.get(), H, W, D, d.get(), nullptr), "smt_wta");
        d.download(disp);
    } else if (which == 3) {    // a throw between create and destroy without cleanup
        smt_crossarm *h = nullptr;
        smt::check(smt_crossarm_create(H, W, D, nullptr, &h), "create");
        stub_fail("smt_crossarm_reset", SMT_ERR_HIP);
        try { smt::check(smt_crossarm_reset(h), "reset"); smt_crossarm_destroy(h); } catch (const std::runtime_error &) { }
    } else return 2;
    return 0;
}

struct Case { const char *family; void (*fn)(); const char *names; };
const Case CASES[] = {
    {"devbuf", f_devbuf, "check batch_elems_ inner_size_ DevBuf::DevBuf DevBuf::resize DevBuf::upload DevBuf::download DevBuf::get DevBuf::size"},
    {"adcensus", f_adcensus, "AD_Census::AD_Census AD_Census::Initialize AD_Census::setQuirks AD_Census::ComputeADcensus AD_Census::ComputeADcensusRight "
                             "AD_Census::DevicePtrLeft AD_Census::DevicePtrRight AD_Census::GetPtrLeft AD_Census::GetPtrRight AD_Census::WTA"},
    {"multi", f_multi, "AD_Census_batch_all_devices"},
    {"crossarm", f_crossarm, "CrossArmAggregation::CrossArmAggregation CrossArmAggregation::Initialize CrossArmAggregation::setSubpixel "
                             "CrossArmAggregation::setQuirks CrossArmAggregation::ComputeArmLengths CrossArmAggregation::ComputeLeftArmLength "
                             "CrossArmAggregation::ComputeRightArmLength CrossArmAggregation::ComputeTopArmLength CrossArmAggregation::ComputeButtonArmLength "
                             "CrossArmAggregation::Aggregation CrossArmAggregation::AggregationVertical CrossArmAggregation::AggregationVerticalDevice "
                             "CrossArmAggregation::WTA"},
    {"scanline", f_scanline, "ScanlineOptimizer::ScanlineOptimizer ScanlineOptimizer::Initialize ScanlineOptimizer::setSubpixel ScanlineOptimizer::setQuirks "
                             "ScanlineOptimizer::ScanLine ScanlineOptimizer::WTA ScanlineOptimizer::DeviceProcessedVolume"},
    {"post", f_post, "LeftRightConsistency LeftAndRightConsistency FillTheHole FillTheHoleBatch"},
    {"cblsm", f_cblsm, "chooseArmLengthLeft chooseArmLengthRight chooseArmLengthUp chooseArmLengthDown ArmLengthL ArmLengthR ArmLengthUp ArmLengthDown "
                       "check_image_ ComputeAD ComputeADRight ComputeDispLeft ComputeDispRight ComputeDispV4 costAggregationV5 costAggregationV4 "
                       "ComputeDispOringin WTASubpixel CBLSMFlow::CBLSMFlow CBLSMFlow::run CBLSMFlow::runWindow"},
    {"crossagg", f_crossagg, "CrossAggregator::CrossAggregator CrossAggregator::Initialize CrossAggregator::SetData CrossAggregator::SetParams "
                             "CrossAggregator::Aggregate CrossAggregator::get_arms_ptr CrossAggregator::get_cost_ptr"},
    {"sad", f_sad, "GetPointDepth GetPointDepthLeft GetPointDepthRight GetPointDepthBoth SadFlow::SadFlow SadFlow::run"},
    {"ncc", f_ncc, "NCC_algorithem NCCFlow::NCCFlow NCCFlow::set_form NCCFlow::run NCCFlow::runBoth ncc bgr_to_grey NCCWholeFlow::NCCWholeFlow "
                   "NCCWholeFlow::set_form NCCWholeFlow::run"},
    {"asw", f_asw, "getMasks check_masks_ AdaptiveSupportWeight AdaptiveSupportWeightBoth"},
    {"filters", f_filters, "MedianFilterInPlace MedianFilter RemoveSpeckles FillImageNew ASWTail"},
    {"image", f_image, "imread imwrite cvtColorBGR2GRAY"},
    {"pipeline", f_pipeline, "Pipeline::Pipeline Pipeline::setQuirks Pipeline::setSubpixel Pipeline::RunBatch"},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (const Case &c : CASES) printf("%s %s\n", c.family, c.names);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--wrong")) return wrong(atoi(argv[2]));
    if (argc == 2)
        for (const Case &c : CASES)
            if (!strcmp(argv[1], c.family)) {
                c.fn();
                nothing_live();
                printf("%s: contract held\n", c.family);
                return 0;
            }
    fprintf(stderr, "usage: %s <family> | --list | --wrong N\n", argv[0]);
    return 2;
}
