// smt::FillTheHoleBatch (smt_host.hpp) on synthetic LR-checked maps: host buffers in, host maps out, everything
// computed by libsmt_hip.so.  Prints one FNV-1a hash and the status per pair for tests/test_fill_batch_gpu.py, which
// rebuilds the same maps.   usage: fill_main pairs row col D seed
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "smt_host.hpp"

static uint64_t fnv(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char **argv)
{
    const int P = argc > 1 ? atoi(argv[1]) : 3, row = argc > 2 ? atoi(argv[2]) : 40, col = argc > 3 ? atoi(argv[3]) : 90;
    const int D = argc > 4 ? atoi(argv[4]) : 16;
    uint32_t s = argc > 5 ? (uint32_t)atoi(argv[5]) : 5;
    try {
        const size_t n = (size_t)row * col;
        std::vector<float> disp(P * n);
        std::vector<uint8_t> cls(P * n);
        // per pixel one LCG step: bits 28..31 choose the class (1 in 16 occlusion, 3 in 16 mismatch), bits 23..27 a hole
        // among the kept pixels (1 in 32), bits 16..19 the disparity
        for (size_t k = 0; k < P * n; k++) {
            s = s * 1664525u + 1013904223u;
            const unsigned c = s >> 28, h = (s >> 23) & 31u;
            cls[k] = c == 0 ? 1 : c <= 3 ? 2 : 0;
            disp[k] = cls[k] ? INFINITY : h == 0 ? 65535.0f : (float)((s >> 16) & 15u);
        }
        std::vector<std::array<int, 4>> status;
        smt::FillTheHoleBatch(P, row, col, D, disp.data(), cls.data(), status);
        for (int b = 0; b < P; b++)
            printf("pair %d %016llx %d %d %d %d\n", b, (unsigned long long)fnv(disp.data() + b * n, n * 4), status[b][0],
                   status[b][1], status[b][2], status[b][3]);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
