// Counterpart of ASW/TeddyBilateral.cpp:7-53, the active lines in the file's own order:
//   :9      imread(path): 3-channel B, G, R
//   :39-46  winSize = 11 (the window's side is 2 * winSize + 3), spaceSigma = 50, colorSigma = 25, the two masks
//   :52     the bilateral filter of the left image -- the call names bilateralfiterWight's argument list, which does not
//           compile (BiliteralFilter.h:145-242); what runs here is bilateralfiter (:49-142) with the same window and sigmas
// through smt::bilateralfiter (host/smt_bilateral.hpp).  The Lab and gray conversions (:32-36) feed nothing.  Host buffers
// in and out, everything computed by libsmt_hip.so.  Writes the filtered image and prints its FNV-1a hash for the tests.
//   usage: bilateral_main in.{png,ppm,pgm} out.{png,ppm} [--wsize side | --wsize width height] [--sigma space color] [--divide]
//   --divide: the weights are divided by their sum (SMT_BILATERAL_NORM_DIVIDE) instead of multiplied by its reciprocal
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "smt_bilateral.hpp"

static uint64_t fnv(const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char **argv)
{
    try {
        using namespace smt;
        const int winSize = 11;                                                 // TeddyBilateral.cpp:39
        Size wsize(winSize * 2 + 3, winSize * 2 + 3);                           // :45
        double spaceSigma = 50, colorSigma = 25;                                // :41-42
        int norm = SMT_BILATERAL_NORM_RECIPROCAL;
        const char *paths[2] = {nullptr, nullptr};
        int np = 0;
        auto number = [&](int a) { return a < argc && (isdigit((unsigned char)argv[a][0]) || argv[a][0] == '.'); };
        for (int a = 1; a < argc; a++) {
            if (!strcmp(argv[a], "--divide")) {
                norm = SMT_BILATERAL_NORM_DIVIDE;
            } else if (!strcmp(argv[a], "--wsize") && number(a + 1)) {
                wsize.width = wsize.height = atoi(argv[++a]);
                if (number(a + 1)) wsize.height = atoi(argv[++a]);
            } else if (!strcmp(argv[a], "--sigma") && number(a + 1) && number(a + 2)) {
                spaceSigma = atof(argv[a + 1]);
                colorSigma = atof(argv[a + 2]);
                a += 2;
            } else if (np < 2 && argv[a][0] != '-') {
                paths[np++] = argv[a];
            } else {
                throw std::runtime_error(std::string("unexpected argument ") + argv[a]);
            }
        }
        if (np != 2) throw std::runtime_error("usage: bilateral_main in out [--wsize side | --wsize width height] [--sigma space color] [--divide]");
        const Image left = imread(paths[0]);                                    // :9
        const Image target = bilateralfiter(left, wsize, spaceSigma, colorSigma, norm);   // :52
        imwrite(paths[1], target.data.data(), target.rows, target.cols, target.channels);
        printf("target %016llx\n", (unsigned long long)fnv(target.data.data(), target.data.size()));
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
