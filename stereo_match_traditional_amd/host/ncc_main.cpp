// Counterpart of NCC/NCC_main.cpp:8-29 with :24 enabled, the lines in the file's own order:
//   :11-12  imread(path, 0) of both images (or a synthetic pair); gray
//   :24     ncc(leftImage, rightImage, "left"), and the same call with "right", the reference's other type
// through smt::NCCWholeFlow (smt_whole_ncc_flow_*), which then runs the int-map cross-check of Sad.h:184-222 on the two
// offset maps.  :28 (imwrite) with --write; the display code (:27, :29) is app shell.  :33-57 (NCC_algorithem and its
// normalisation) is matchers_main's.  Host buffers in and out, everything computed by libsmt_hip.so through smt_host.hpp.
// Prints FNV-1a hashes for the tests.
//   usage: ncc_main H W seed [kernel_size] [max_offset] [add_constant]      synthetic pair
//          ncc_main left.png right.png [kernel_size] [max_offset] [add_constant] [--write]
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "smt_host.hpp"

static uint64_t fnv(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 1099511628211ull; }
    return h;
}
static int tri(int x, int p) { int m = x % (2 * p); int v = m < p ? m : 2 * p - m; return v - p / 2; }
static void synth(int H, int W, int D, uint32_t seed, std::vector<unsigned char> &L, std::vector<unsigned char> &R)
{
    uint32_t s = seed;
    L.resize((size_t)H * W); R.resize((size_t)H * W);
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) {
            s = s * 1664525u + 1013904223u;
            int b = (int)(s >> 24);
            int v = 128 + tri(j, 203) * 70 / 101 + tri(i, 139) * 40 / 69 + 25 * (((j / 40) + (i / 30)) & 1) + (b % 6);
            R[(size_t)i * W + j] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
    for (int i = 0; i < H; i++) {
        int g = D / 8 + ((i / 8) % 7) * (D / 16);
        for (int j = 0; j < W; j++) {
            s = s * 1664525u + 1013904223u;
            L[(size_t)i * W + j] = j >= g ? R[(size_t)i * W + j - g] : (unsigned char)(s >> 24);
        }
    }
}

int main(int argc, char **argv)
{
    try {
        using namespace smt;
        Image leftImage, rightImage;
        int kernel_size = 5, max_offset = 79, add_constant = 0;                // NCC.h:121-122, :117
        bool write = false;
        if (argc > 1 && !strcmp(argv[argc - 1], "--write")) { write = true; argc--; }
        if (argc > 2 && !isdigit((unsigned char)argv[1][0])) {
            leftImage = imread(argv[1], 1);                                     // :11-12, flag 0: gray
            rightImage = imread(argv[2], 1);
            if (argc > 3) kernel_size = atoi(argv[3]);
            if (argc > 4) max_offset = atoi(argv[4]);
            if (argc > 5) add_constant = atoi(argv[5]);
            if (leftImage.rows != rightImage.rows || leftImage.cols != rightImage.cols) throw std::runtime_error("image sizes differ");
        } else {
            const int row = argc > 1 ? atoi(argv[1]) : 375, col = argc > 2 ? atoi(argv[2]) : 450;
            const uint32_t seed = argc > 3 ? (uint32_t)atoi(argv[3]) : 6;
            if (argc > 4) kernel_size = atoi(argv[4]);
            if (argc > 5) max_offset = atoi(argv[5]);
            if (argc > 6) add_constant = atoi(argv[6]);
            leftImage.rows = rightImage.rows = row; leftImage.cols = rightImage.cols = col;
            leftImage.channels = rightImage.channels = 1;
            synth(row, col, max_offset, seed, leftImage.data, rightImage.data);
        }
        const int row = leftImage.rows, col = leftImage.cols;                  // :15-16
        const size_t n = (size_t)row * col;
        Image left_disp, right_disp;
        left_disp.rows = right_disp.rows = row; left_disp.cols = right_disp.cols = col; left_disp.channels = right_disp.channels = 1;
        left_disp.data.resize(n); right_disp.data.resize(n);
        std::vector<int> offleft(n), offright(n), lastdisp(n);
        NCCWholeFlow flow(row, col, kernel_size, max_offset, add_constant != 0);
        flow.run(leftImage.data.data(), rightImage.data.data(), 1, left_disp.data.data(), right_disp.data.data(), offleft.data(),
                 offright.data(), lastdisp.data());                            // :24, both types
        printf("left_disp %016llx\nright_disp %016llx\noffleft %016llx\noffright %016llx\nlastdisp %016llx\n",
               (unsigned long long)fnv(left_disp.data.data(), n), (unsigned long long)fnv(right_disp.data.data(), n),
               (unsigned long long)fnv(offleft.data(), n * 4), (unsigned long long)fnv(offright.data(), n * 4),
               (unsigned long long)fnv(lastdisp.data(), n * 4));
        if (write) {                                                           // :28
            imwrite("disp_left.png", left_disp.data.data(), row, col, 1);
            imwrite("disp_right.png", right_disp.data.data(), row, col, 1);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
