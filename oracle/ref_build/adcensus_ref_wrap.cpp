// C entry points around the REFERENCE's own AD-CensusV1 sources (AD-Census.h, CrossArm.{h,cpp},
// ScanlineOptimizer.h, PostProcessing.h), compiled unmodified from where they lie against the
// container-only stand-in oracle/ref_build/shim/opencv2/opencv.hpp -- see oracle/Makefile.
// This wrapper contains no algorithm: it drives the reference's public functions in the call
// order of main.cpp and copies results out.  It is built with -fno-access-control so that it can
// read (and, for the aggregation entry, load) the private arm maps and read the four private
// path volumes.  The reference leaks every buffer it allocates (its destructors are empty); these
// entry points leak with it.  Test infrastructure.
#include "AD-Census.h"
#include "CrossArm.h"
#include "ScanlineOptimizer.h"
#include "PostProcessing.h"

#define REF_API extern "C" __attribute__((visibility("default")))

// main.cpp:57-63
REF_API int ref_adcensus(float* left, float* right, int row, int col, int dispRange, float sigmaC, float sigmaS,
                         float* volLeft, float* volRight, float* dispLeft, float* dispRight)
{
    Mat none;
    AD_Census adc;
    adc.Initialize(left, right, dispRange, row, col, none, none, sigmaC, sigmaS);
    adc.ComputeADcensus();
    adc.ComputeADcensusRight();
    adc.WTA(dispLeft, dispRight);
    const size_t n = size_t(row) * col * dispRange;
    std::memcpy(volLeft, adc.GetPtrLeft(), n * sizeof(float));
    std::memcpy(volRight, adc.GetPtrRight(), n * sizeof(float));
    return 0;
}

static void call_arm(CrossArmAggregation& ca, int dir, const Mat& img)
{
    switch (dir) {
    case 0: ca.ComputeLeftArmLength(img); break;
    case 1: ca.ComputeRightArmLength(img); break;
    case 2: ca.ComputeTopArmLength(img); break;
    default: ca.ComputeButtonArmLength(img); break;
    }
}

// main.cpp:67-72: Initialize, then the Compute*ArmLength calls named by dirs[0..n) (0 left, 1 right,
// 2 top, 3 bottom; main.cpp's order is 0,1,2,3).  maps: the four private maps [4][row*col] as
// allocated by Initialize (zeroed) and left by the calls; *tao_after: the private sticky threshold.
REF_API int ref_arms(unsigned char* img, int row, int col, int channels, int tao, const int* dirs, int n,
                     int* maps, int* tao_after)
{
    Mat image(row, col, channels, img);
    CrossArmAggregation ca;
    ca.Initialize(row, col, nullptr, nullptr, tao, 1);
    for (int k = 0; k < n; k++) call_arm(ca, dirs[k], image);
    const size_t bytes = size_t(row) * col * sizeof(int);
    std::memcpy(maps, ca.leftLength, bytes);
    std::memcpy(maps + size_t(row) * col, ca.rightLength, bytes);
    std::memcpy(maps + 2 * size_t(row) * col, ca.topLength, bytes);
    std::memcpy(maps + 3 * size_t(row) * col, ca.buttonLenght, bytes);
    *tao_after = ca._tao;
    return 0;
}

// main.cpp:74-75 on caller-given arm maps: which 0 = AggregationVertical, 2 = Aggregation.
REF_API int ref_aggregate(const int* maps, float* vol, int row, int col, int dispRange, int which,
                          float* out, float* disp)
{
    CrossArmAggregation ca;
    ca.Initialize(row, col, nullptr, nullptr, 30, dispRange);
    const size_t bytes = size_t(row) * col * sizeof(int);
    std::memcpy(ca.leftLength, maps, bytes);
    std::memcpy(ca.rightLength, maps + size_t(row) * col, bytes);
    std::memcpy(ca.topLength, maps + 2 * size_t(row) * col, bytes);
    std::memcpy(ca.buttonLenght, maps + 3 * size_t(row) * col, bytes);
    if (which == 0) ca.AggregationVertical(vol, out);
    else ca.Aggregation(vol, out);
    ca.WTA(out, disp);
    return 0;
}

// main.cpp:86-89
REF_API int ref_scanline(float* cost, float* gray, int row, int col, int dispRange, int p1, int p2,
                         float* left, float* right, float* up, float* down, float* sum, float* disp)
{
    ScanlineOptimizer so;
    so.Initialize(row, col, dispRange, cost, p1, p2);
    so.ScanLine(cost, gray);
    so.WTA(disp);
    const size_t bytes = size_t(row) * col * dispRange * sizeof(float);
    std::memcpy(left, so.leftVolume, bytes);
    std::memcpy(right, so.rightVolume, bytes);
    std::memcpy(up, so.upVolume, bytes);
    std::memcpy(down, so.downVolume, bytes);
    std::memcpy(sum, so._ProcessedVolume, bytes);
    return 0;
}

static int copy_pairs(const vector<pair<int, int>>& v, int* out)
{
    for (size_t k = 0; k < v.size(); k++) { out[2 * k] = v[k].first; out[2 * k + 1] = v[k].second; }
    return int(v.size());
}

// main.cpp:92.  occ / mis: capacity row*col pairs each.
REF_API int ref_lrcheck(float* dispLeft, float* dispRight, int row, int col, int gate,
                        int* occ, int* n_occ, int* mis, int* n_mis)
{
    vector<pair<int, int>> o, m;
    LeftRightConsistency(col, row, gate, dispLeft, dispRight, o, m);
    *n_occ = copy_pairs(o, occ);
    *n_mis = copy_pairs(m, mis);
    return 0;
}

REF_API int ref_lrcheck_variant(float* dispLeft, float* dispRight, float* lastDisp, int row, int col, float gate,
                                int* occ, int* n_occ, int* mis, int* n_mis)
{
    vector<pair<int, int>> o, m;
    LeftAndRightConsistency(dispLeft, dispRight, lastDisp, col, row, gate, o, m);
    *n_occ = copy_pairs(o, occ);
    *n_mis = copy_pairs(m, mis);
    return 0;
}

// mis_after: the list FillTheHole leaves in `mismatch` (capacity row*col pairs).
REF_API int ref_fill_the_hole(float* disp, int row, int col, int dispRange, const int* occ, int n_occ,
                              const int* mis, int n_mis, int* mis_after, int* n_mis_after)
{
    vector<pair<int, int>> o, m;
    for (int k = 0; k < n_occ; k++) o.emplace_back(occ[2 * k], occ[2 * k + 1]);
    for (int k = 0; k < n_mis; k++) m.emplace_back(mis[2 * k], mis[2 * k + 1]);
    FillTheHole(row, col, dispRange, disp, o, m);
    *n_mis_after = copy_pairs(m, mis_after);
    return 0;
}

// main.cpp:93.  invalid_val arrives as an int ARGUMENT: `RemoveSpeckles(..., Invalid_Float)` lets the
// compiler fold int(+inf) at compile time, which g++ does not fold to the x86 run-time value INT_MIN.
REF_API int ref_remove_speckles(float* disp, int width, int height, int diff_insame, unsigned min_speckle_aera,
                                int invalid_val)
{
    RemoveSpeckles(disp, width, height, diff_insame, min_speckle_aera, invalid_val);
    return 0;
}

// main.cpp:94
REF_API int ref_median(const float* in, float* out, int width, int height, int wnd_size)
{
    MedianFilter(in, out, width, height, wnd_size);
    return 0;
}
