// Counterpart of SAD/SADmain.cpp:24-79 with :67-68 enabled, the active lines in the file's own order:
//   :27-41  imread(path, 0) of both images (or a synthetic pair); gray
//   :47-48  copyMakeBorder(img, winsize + 1, BORDER_REPLICATE)
//   :66-67  GetPointDepthLeft, GetPointDepthRight            one evaluation of the hypotheses (smt_sad_both)
//   :68     CrossCheckDiaparity
// all three through smt::SadFlow (smt_sad_flow_*).  :69 (RemoveSpeckles reading an int Mat through at<float>) and
// :71-78 (OpenCV calls, scan-order fillers) are not part of the flow; the display code (:86-96) is app shell.  Host
// buffers in and out, everything computed by libsmt_hip.so through smt_host.hpp.  Prints FNV-1a hashes for the tests.
//   usage: sad_main H W D seed [winsize]          synthetic pair, MaxDisparity D
//          sad_main left.png right.png [D] [winsize]
//   --subpixel anywhere on the line, or --subpixel min_den as its last two words: the maps keep the parabola OptimalDisparity computes and drops
//   (Sad.h:76-81) through smt::SadSubpixelFlow; float maps under the same three names, lastdisp +inf where rejected, and
//   the class map.  Without the flag the output is the integer flow's.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "smt_sad_subpixel.hpp"

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
        bool subpixel = false;
        float min_den = 1.0f;                                                   // Sad.h:80
        for (int a = 1; a < argc; a++)
            if (!strcmp(argv[a], "--subpixel")) {
                subpixel = true;
                int take = 1;
                if (a + 1 < argc && (isdigit((unsigned char)argv[a + 1][0]) || argv[a + 1][0] == '.') && a + 2 == argc) {
                    min_den = (float)atof(argv[a + 1]);                         // a value only as the line's last word
                    take = 2;
                }
                for (int b = a; b + take <= argc; b++) argv[b] = argv[b + take];   // argv[argc] is the null pointer
                argc -= take;
                break;
            }
        Image leftimg, rightimg;
        int MaxDisparity = 60;                                                  // SADmain.cpp:33
        int winsize = 3;                                                        // :34
        if (argc > 2 && !isdigit((unsigned char)argv[1][0])) {
            leftimg = imread(argv[1], 1);                                       // :27-28, flag 0: gray
            rightimg = imread(argv[2], 1);
            if (argc > 3) MaxDisparity = atoi(argv[3]);
            if (argc > 4) winsize = atoi(argv[4]);
            if (leftimg.rows != rightimg.rows || leftimg.cols != rightimg.cols) throw std::runtime_error("image sizes differ");
        } else {
            const int row = argc > 1 ? atoi(argv[1]) : 375, col = argc > 2 ? atoi(argv[2]) : 450;
            if (argc > 3) MaxDisparity = atoi(argv[3]);
            const uint32_t seed = argc > 4 ? (uint32_t)atoi(argv[4]) : 6;
            if (argc > 5) winsize = atoi(argv[5]);
            leftimg.rows = rightimg.rows = row; leftimg.cols = rightimg.cols = col; leftimg.channels = rightimg.channels = 1;
            synth(row, col, MaxDisparity, seed, leftimg.data, rightimg.data);
        }
        const int row = leftimg.rows, col = leftimg.cols;                      // :43-44
        const size_t n = (size_t)row * col;
        if (subpixel) {
            std::vector<float> depthleft(n), depthright(n), lastdisp(n);
            std::vector<unsigned char> cls(n);
            SadSubpixelFlow flow(row, col, MaxDisparity, winsize, min_den);
            flow.run(leftimg.data.data(), rightimg.data.data(), 1, depthleft.data(), depthright.data(), lastdisp.data(), cls.data());
            printf("depthleft %016llx\ndepthright %016llx\nlastdisp %016llx\ncls %016llx\n", (unsigned long long)fnv(depthleft.data(), n * 4),
                   (unsigned long long)fnv(depthright.data(), n * 4), (unsigned long long)fnv(lastdisp.data(), n * 4),
                   (unsigned long long)fnv(cls.data(), n));
            return 0;
        }
        std::vector<int> depthleft(n), depthright(n), lastdisp(n);              // :57-59
        SadFlow flow(row, col, MaxDisparity, winsize);
        flow.run(leftimg.data.data(), rightimg.data.data(), 1, depthleft.data(), depthright.data(), lastdisp.data());   // :47-48, :66-68
        printf("depthleft %016llx\ndepthright %016llx\nlastdisp %016llx\n", (unsigned long long)fnv(depthleft.data(), n * 4),
               (unsigned long long)fnv(depthright.data(), n * 4), (unsigned long long)fnv(lastdisp.data(), n * 4));
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
