// Every public function of host/smt_bilateral.hpp against the contract stub, with exact-size heap buffers, under
// AddressSanitizer: the entry called with the window as (height, width), the stub's byte in every output element,
// untouched inputs, the tables by value, a std::runtime_error when an entry fails -- each in turn -- and nothing left
// allocated.  A stand-alone program; no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "../../stereo_match_traditional_amd/host/smt_bilateral.hpp"
#include "bilateral_stub.hpp"

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

int masks()
{
    std::vector<double> space(3, 7.0), color(2, 9.0);
    smt::getGausssianMask(space, smt::Size(6, 4), 10);                  // Size(width, height): 4 rows of 6
    REQUIRE(space.size() == 24 && space[1 * 6 + 2] == 1.0 && space[0] == exp(-(4.0 + 1.0) / 200.0));
    smt::getColorMask(color, 30);                                       // push_back: appended behind what is there
    REQUIRE(color.size() == 258 && color[0] == 9.0 && color[2] == 1.0 && color[257] == exp(-(255 * 255) / 1800.0));
    int thrown = 0;
    try { smt::getGausssianMask(space, smt::Size(0, 3), 10); } catch (const std::runtime_error &) { thrown++; }
    try { smt::getGausssianMask(space, smt::Size(3, 65), 10); } catch (const std::runtime_error &) { thrown++; }
    REQUIRE(thrown == 2);
    return 0;
}

int filter(const char *fail)
{
    constexpr int H = 3, W = 5;
    for (int channels : {1, 3}) {
        const size_t n = (size_t)H * W * channels;
        auto src = buf<unsigned char>(n, 7), dst = buf<unsigned char>(n, 0xEE);
        auto acc = buf<double>(n, 0xEE);
        stub_log_clear();
        if (fail) stub_fail(fail);
        smt::bilateralfiter(src.get(), dst.get(), H, W, channels, smt::Size(6, 4), 10, 30, SMT_BILATERAL_NORM_DIVIDE, acc.get());
        REQUIRE(called("smt_bilateral_masks") && called("smt_bilateral_filter_batch"));
        const StubCall &c = stub_last_filter();
        REQUIRE(c.images == 1 && c.H == H && c.W == W && c.channels == channels && c.wsize_h == 4 && c.wsize_w == 6);
        REQUIRE(c.norm == SMT_BILATERAL_NORM_DIVIDE && c.acc);
        REQUIRE(all(dst.get(), n, STUB_DST) && all(acc.get(), n, STUB_ACC) && all(src.get(), n, 7));
        memset(dst.get(), 0xEE, n);
        smt::bilateralfiter(src.get(), dst.get(), H, W, channels, smt::Size(63, 64), 50, 25);       // no sums asked for
        REQUIRE(!stub_last_filter().acc && stub_last_filter().norm == SMT_BILATERAL_NORM_RECIPROCAL && stub_last_filter().wsize_h == 64);
        REQUIRE(all(dst.get(), n, STUB_DST));
        smt::Image im;
        im.rows = H; im.cols = W; im.channels = channels;
        im.data.assign(n, 9);
        const smt::Image out = smt::bilateralfiter(im, smt::Size(25, 25), 50, 25);
        REQUIRE(out.rows == H && out.cols == W && out.channels == channels && out.data.size() == n && all(out.data.data(), n, STUB_DST));
    }
    return 0;
}

// what the header rejects must come out as std::runtime_error, with nothing left behind
int rejected()
{
    auto src = buf<unsigned char>(30, 1), dst = buf<unsigned char>(30, 2);
    int thrown = 0;
    try { smt::bilateralfiter(src.get(), dst.get(), 3, 5, 2, smt::Size(3, 3), 10, 30); } catch (const std::runtime_error &) { thrown++; }
    try { smt::bilateralfiter(src.get(), dst.get(), 0, 5, 1, smt::Size(3, 3), 10, 30); } catch (const std::runtime_error &) { thrown++; }
    try { smt::bilateralfiter(src.get(), dst.get(), 3, 5, 1, smt::Size(65, 3), 10, 30); } catch (const std::runtime_error &) { thrown++; }
    try { smt::bilateralfiter(src.get(), dst.get(), 3, 5, 1, smt::Size(3, 3), 10, 30, 2); } catch (const std::runtime_error &) { thrown++; }
    try {
        smt::Image im;
        im.rows = 3; im.cols = 5; im.channels = 3;
        im.data.assign(14, 0);                                           // a vector that does not hold the image
        (void)smt::bilateralfiter(im, smt::Size(3, 3), 10, 30);
    } catch (const std::runtime_error &) { thrown++; }
    REQUIRE(thrown == 5 && all(dst.get(), 30, 2));
    return 0;
}

const char *const ENTRIES[] = {"smt_bilateral_masks", "smt_malloc", "smt_memcpy_h2d", "smt_bilateral_filter_batch", "smt_memcpy_d2h",
                               "smt_stream_sync"};
}  // namespace

int main()
{
    if (masks() || filter(nullptr) || rejected()) return 1;
    REQUIRE(stub_live_allocs() == 0);
    for (const char *e : ENTRIES) {
        bool thrown = false;
        try { (void)filter(e); } catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) { fprintf(stderr, "%s failed and nothing was thrown\n", e); return 1; }
        REQUIRE(stub_live_allocs() == 0);
    }
    printf("bilateral: contract held\n");
    return 0;
}
