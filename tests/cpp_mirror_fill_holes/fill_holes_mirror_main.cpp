// host/smt_fill_holes.hpp against the contract stub beside this file: exact-size heap buffers in and out, what reaches
// the entry, what is rejected before it, and that a failing entry leaves nothing allocated.  Built with
// -fsanitize=address,undefined by tests/test_fill_holes_cpu.py and run as its own process.
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>

#include "../../stereo_match_traditional_amd/host/smt_fill_holes.hpp"
#include "fill_holes_stub.hpp"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class F> static bool throws(F f)
{
    try { f(); } catch (const std::runtime_error &) { return true; }
    return false;
}

static bool all_bytes(const void *p, size_t n, unsigned char b)
{
    const unsigned char *q = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++)
        if (q[i] != b) return false;
    return true;
}

int main()
{
    typedef std::vector<std::pair<int, int>> List;
    const float inf = std::numeric_limits<float>::infinity();
    const int row = 5, col = 7;
    const size_t n = (size_t)row * col;
    std::unique_ptr<float[]> disp(new float[n]);
    std::unique_ptr<unsigned char[]> cls(new unsigned char[n]);
    std::unique_ptr<int[]> status(new int[4]);
    for (size_t k = 0; k < n; k++) { disp[k] = (float)k; cls[k] = (unsigned char)(k % 3); }

    // on a class map: one call of the entry, map and status downloaded whole, nothing left allocated
    smt::FillHolesInDispMap(disp.get(), cls.get(), row, col, inf, status.get());
    REQUIRE(all_bytes(disp.get(), n * 4, STUB_MAP) && all_bytes(status.get(), 16, STUB_STATUS));
    REQUIRE(stub_live_allocs() == 0);
    {
        const StubCall &c = stub_last_fill();
        REQUIRE(c.pairs == 1 && c.H == row && c.W == col && c.invalid == inf && c.status);
        REQUIRE(c.cls.size() == n && std::memcmp(c.cls.data(), cls.get(), n) == 0);
    }
    int entries = 0;
    for (const std::string &e : stub_log()) entries += e == "smt_fill_holes_batch";
    REQUIRE(entries == 1);

    // the reference's signature: width first, the lists become the class map, the invalid value is passed on
    for (size_t k = 0; k < n; k++) disp[k] = (float)k;
    const List occ = {{0, 1}, {0, 6}, {4, 0}}, mis = {{0, 0}, {2, 3}, {4, 6}};
    smt::FillHolesInDispMap(col, row, disp.get(), occ, mis, -1.0f);
    {
        const StubCall &c = stub_last_fill();
        REQUIRE(c.H == row && c.W == col && c.invalid == -1.0f);
        size_t ones = 0, twos = 0;
        for (unsigned char v : c.cls) { ones += v == 1; twos += v == 2; }
        REQUIRE(ones == 3 && twos == 3 && c.cls[1] == 1 && c.cls[6] == 1 && c.cls[4 * col] == 1);
        REQUIRE(c.cls[0] == 2 && c.cls[2 * col + 3] == 2 && c.cls[4 * col + 6] == 2);
    }
    REQUIRE(all_bytes(disp.get(), n * 4, STUB_MAP) && stub_live_allocs() == 0);
    smt::FillHolesInDispMap(col, row, disp.get(), List(), List(), inf);          // empty lists: all three passes still run
    REQUIRE(stub_last_fill().cls.size() == n && all_bytes(stub_last_fill().cls.data(), n, 0));

    // rejected before the entry
    stub_log_clear();
    REQUIRE(throws([&] { smt::FillHolesInDispMap(nullptr, cls.get(), row, col); }));
    REQUIRE(throws([&] { smt::FillHolesInDispMap(disp.get(), nullptr, row, col); }));
    REQUIRE(throws([&] { smt::FillHolesInDispMap(disp.get(), cls.get(), 0, col); }));
    REQUIRE(throws([&] { smt::FillHolesInDispMap(disp.get(), cls.get(), row, SMT_FILLHOLES_MAX_DIM + 1); }));
    REQUIRE(throws([&] { smt::FillHolesInDispMap(col, row, disp.get(), List{{5, 0}}, List(), inf); }));      // outside
    REQUIRE(throws([&] { smt::FillHolesInDispMap(col, row, disp.get(), List{{0, -1}}, List(), inf); }));
    REQUIRE(throws([&] { smt::FillHolesInDispMap(col, row, disp.get(), List{{1, 0}, {0, 3}}, List(), inf); }));   // not raster order
    REQUIRE(throws([&] { smt::FillHolesInDispMap(col, row, disp.get(), List{{1, 1}, {1, 1}}, List(), inf); }));   // twice
    REQUIRE(throws([&] { smt::FillHolesInDispMap(col, row, disp.get(), List{{1, 1}}, List{{1, 1}}, inf); }));     // in both
    REQUIRE(stub_log().empty() && stub_live_allocs() == 0);
    // rejected by the entry: a NaN invalid value
    REQUIRE(throws([&] { smt::FillHolesInDispMap(disp.get(), cls.get(), row, col, std::numeric_limits<float>::quiet_NaN()); }));
    REQUIRE(stub_live_allocs() == 0);

    // a failure of any entry is thrown and leaves nothing allocated
    for (const char *e : {"smt_malloc", "smt_memcpy_h2d", "smt_fill_holes_batch", "smt_memcpy_d2h"}) {
        stub_fail(e);
        REQUIRE(throws([&] { smt::FillHolesInDispMap(disp.get(), cls.get(), row, col, inf, status.get()); }));
        REQUIRE(stub_live_allocs() == 0);
    }
    std::printf("fill_holes: contract held\n");
    return 0;
}
