// Counterpart of CBLSM/CBLSM.cpp:13-213 on a synthetic pair, the active lines in the file's own order:
//   :64-67   ArmLength{L,R,Up,Down}(imageL, tao = 25, ..., maxLength = 34, secLength = 17)   four by-value-tao calls
//   :101-104 the same on imageR
//   :133-134 ComputeAD / ComputeADRight (uchar)
//   :146     costAggregationV5(right volume, RIGHT arms)
//   :147     costAggregationV5(left volume, LEFT arms)
//   :149     costAggregationV5(left result again, LEFT arms)
//   :150     costAggregationV5(right result again, LEFT arms)            <- the left image's arms, as written
//   :152-153 ComputeDispOringin x 2
// (medianBlur :24-25 feeds nothing; copyMakeBorder :124-129 feeds only commented-out calls; the display conversion
// is app shell.)  Host buffers in and out, everything computed by libsmt_hip.so through smt_host.hpp.  Prints FNV-1a
// hashes for tests/test_cpp_host_gpu.py.  With --post the file's tail runs as well and the finished map is hashed:
//   :155, :160  LeftRightConsistency(col, row, gate = 5, dispLeft, dispRight, occlusion, mismatches)
//   :161        RemoveSpeckles(dispLeft, col, row, 1, 50, Invalid_Float)       int(+inf): INT_MIN on x86
//   :162        MedianFilter(dispLeft, dispLeft, col, row, 3)                  in == out
// With --window[=winSize] (default 1, :28) the flow runs once more with :132 enabled -- ComputeDispLeft, and ComputeDispRight as
// its right-view counterpart, on the images padded as :124-125 pad them, in place of ComputeAD / ComputeADRight -- through
// smt::CBLSMFlow::runWindow, and the two maps are hashed (disp_left_window, disp_right_window); the two window volumes are hashed too, computed by
// smt::ComputeDispLeft / smt::ComputeDispRight on host-padded images (window_left, window_right).
//   usage: cblsm_main H W D seed [--post] [--window[=winSize]]
#include <climits>
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
    const int row = argc > 1 ? atoi(argv[1]) : 375, col = argc > 2 ? atoi(argv[2]) : 450;
    const int dispRange = argc > 3 ? atoi(argv[3]) : 60;                       // CBLSM.cpp:29
    const uint32_t seed = argc > 4 ? (uint32_t)atoi(argv[4]) : 6;
    bool post = false;
    int window = -1;
    for (int k = 1; k < argc; k++) {
        post = post || strcmp(argv[k], "--post") == 0;
        if (strcmp(argv[k], "--window") == 0) window = 1;
        else if (strncmp(argv[k], "--window=", 9) == 0) window = atoi(argv[k] + 9);
    }
    try {
        using namespace smt;
        Image imageL, imageR;
        imageL.rows = imageR.rows = row; imageL.cols = imageR.cols = col; imageL.channels = imageR.channels = 1;
        synth(row, col, dispRange, seed, imageL.data, imageR.data);
        const int winSize = 1;                                                  // :28
        const unsigned char tao = 25;                                           // :30
        const int maxLength = 34, secLength = 17;                               // :31-32
        const size_t n = (size_t)row * col, V = n * dispRange;
        std::vector<float> dispVolumLeft(V), dispVolumRight(V), costVolumLeft(V), costVolumRight(V), costVolumLeftSec(V),
            costVolumRightSec(V), dispLeft(n), dispRight(n);
        std::vector<int> ArmLL(n), ArmLR(n), ArmLup(n), ArmLdown(n), ArmRL(n), ArmRR(n), ArmRup(n), ArmRdown(n);
        ArmLengthL(imageL, tao, ArmLL.data(), maxLength, secLength);            // :64-67
        ArmLengthR(imageL, tao, ArmLR.data(), maxLength, secLength);
        ArmLengthUp(imageL, tao, ArmLup.data(), maxLength, secLength);
        ArmLengthDown(imageL, tao, ArmLdown.data(), maxLength, secLength);
        unsigned char *leftPtr = imageL.data.data(), *rightPtr = imageR.data.data();   // :89-99
        ArmLengthL(imageR, tao, ArmRL.data(), maxLength, secLength);            // :101-104
        ArmLengthR(imageR, tao, ArmRR.data(), maxLength, secLength);
        ArmLengthUp(imageR, tao, ArmRup.data(), maxLength, secLength);
        ArmLengthDown(imageR, tao, ArmRdown.data(), maxLength, secLength);
        ComputeAD(col, row, dispRange, leftPtr, rightPtr, dispVolumLeft.data());        // :133
        ComputeADRight(col, row, dispRange, leftPtr, rightPtr, dispVolumRight.data());  // :134
        costAggregationV5(dispVolumRight.data(), costVolumRight.data(), ArmRL.data(), ArmRR.data(), ArmRup.data(), ArmRdown.data(), dispRange, row, col, winSize);   // :146
        costAggregationV5(dispVolumLeft.data(), costVolumLeft.data(), ArmLL.data(), ArmLR.data(), ArmLup.data(), ArmLdown.data(), dispRange, row, col, winSize);      // :147
        costAggregationV5(costVolumLeft.data(), costVolumLeftSec.data(), ArmLL.data(), ArmLR.data(), ArmLup.data(), ArmLdown.data(), dispRange, row, col, winSize);   // :149
        costAggregationV5(costVolumRight.data(), costVolumRightSec.data(), ArmLL.data(), ArmLR.data(), ArmLup.data(), ArmLdown.data(), dispRange, row, col, winSize); // :150
        ComputeDispOringin(costVolumLeftSec.data(), dispLeft.data(), dispRange, row, col);     // :152
        ComputeDispOringin(costVolumRightSec.data(), dispRight.data(), dispRange, row, col);   // :153
        const char *an[8] = {"arm_LL", "arm_LR", "arm_Lup", "arm_Ldown", "arm_RL", "arm_RR", "arm_Rup", "arm_Rdown"};
        const std::vector<int> *av[8] = {&ArmLL, &ArmLR, &ArmLup, &ArmLdown, &ArmRL, &ArmRR, &ArmRup, &ArmRdown};
        for (int k = 0; k < 8; k++) printf("%s %016llx\n", an[k], (unsigned long long)fnv(av[k]->data(), n * 4));
        printf("ad_left %016llx\nad_right %016llx\n", (unsigned long long)fnv(dispVolumLeft.data(), V * 4),
               (unsigned long long)fnv(dispVolumRight.data(), V * 4));
        printf("agg_left %016llx\nagg_right %016llx\n", (unsigned long long)fnv(costVolumLeft.data(), V * 4),
               (unsigned long long)fnv(costVolumRight.data(), V * 4));
        printf("agg_left_sec %016llx\nagg_right_sec %016llx\n", (unsigned long long)fnv(costVolumLeftSec.data(), V * 4),
               (unsigned long long)fnv(costVolumRightSec.data(), V * 4));
        printf("disp_left %016llx\ndisp_right %016llx\n", (unsigned long long)fnv(dispLeft.data(), n * 4),
               (unsigned long long)fnv(dispRight.data(), n * 4));
        if (post) {
            int gate = 5;                                                       // :155
            std::vector<std::pair<int, int>> occlusion, mismatches;
            LeftRightConsistency(col, row, gate, dispLeft.data(), dispRight.data(), occlusion, mismatches);   // :160
            RemoveSpeckles(dispLeft.data(), col, row, 1, 50, INT_MIN);          // :161
            MedianFilter(dispLeft.data(), dispLeft.data(), col, row, 3);        // :162
            printf("occlusion %zu\nmismatches %zu\ndisp_left_post %016llx\n", occlusion.size(), mismatches.size(),
                   (unsigned long long)fnv(dispLeft.data(), n * 4));
        }
        if (window >= 0) {
            // :124-125 copyMakeBorder(BORDER_REPLICATE) by window + 1, then :132 and its right-view counterpart on their own
            const int w = window + 1;
            Image padL, padR;
            padL.rows = padR.rows = row + 2 * w; padL.cols = padR.cols = col + 2 * w; padL.channels = padR.channels = 1;
            padL.data.resize((size_t)padL.rows * padL.cols); padR.data.resize(padL.data.size());
            for (int i = 0; i < padL.rows; i++)
                for (int j = 0; j < padL.cols; j++) {
                    const int si = i < w ? 0 : (i - w > row - 1 ? row - 1 : i - w), sj = j < w ? 0 : (j - w > col - 1 ? col - 1 : j - w);
                    padL.data[(size_t)i * padL.cols + j] = leftPtr[(size_t)si * col + sj];
                    padR.data[(size_t)i * padL.cols + j] = rightPtr[(size_t)si * col + sj];
                }
            ComputeDispLeft(dispVolumLeft.data(), padL, padR, window, dispRange, row, col);     // :132
            ComputeDispRight(dispVolumRight.data(), padL, padR, window, dispRange, row, col);
            printf("window_left %016llx\nwindow_right %016llx\n", (unsigned long long)fnv(dispVolumLeft.data(), V * 4),
                   (unsigned long long)fnv(dispVolumRight.data(), V * 4));
            std::vector<float> wl(n), wr(n);
            CBLSMFlow flow(row, col, dispRange);
            flow.runWindow(leftPtr, rightPtr, 1, window, wl.data(), wr.data());   // :132 enabled
            printf("disp_left_window %016llx\ndisp_right_window %016llx\n", (unsigned long long)fnv(wl.data(), n * 4),
                   (unsigned long long)fnv(wr.data(), n * 4));
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
