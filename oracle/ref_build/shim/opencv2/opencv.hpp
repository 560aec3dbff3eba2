// Stand-in for <opencv2/opencv.hpp>, used ONLY to compile the reference's AD-CensusV1 and
// CBLSM/CBLSM.h sources, unmodified and where they lie, into oracle/_ref/ (see oracle/Makefile).
// Test infrastructure; this file is our own text.
//
// It provides the pixel CONTAINER those sources use (Mat with rows / cols / data / channels() /
// at<T>() over a borrowed buffer, Vec3b) and nothing that computes.  Every OpenCV operation that
// would have to restate OpenCV arithmetic is declared so that the headers parse, and aborts when
// reached: Mat - Mat, cv::abs, cv::sum, cv::mean, absdiff, cvtColor and ROI by Range.
//
// Reference functions that reach an aborting stub, and are therefore NOT pinned by these builds:
//   CBLSM.h  sadvalue, sadvalueMean, sadvalueMeanV4                 (Mat - Mat, abs, sum, mean, absdiff)
//            ComputeDispRight, ComputeDispLeft, ComputeDispV4        (ROI by Range, sadvalueMean)
//            ComputeLocalValue, costAggregation, costAggregationNew  (ROI by Range, cv::sum)
//   (cvtColor sits behind channel tests in those same functions.)
// Everything the wrappers in this directory call uses the container only.
#pragma once
#include <algorithm>
#include <cassert>   // PostProcessing.h uses assert without including it
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

typedef unsigned char uchar;
#define CV_BGR2GRAY 6

namespace cv {

[[noreturn]] inline void shim_unpinned(const char* what)
{
    std::fprintf(stderr, "opencv shim: %s is not provided (the caller is not pinned)\n", what);
    std::abort();
}

template <typename T> struct Vec3 {
    T v[3];
    T& operator[](int k) { return v[k]; }
    const T& operator[](int k) const { return v[k]; }
};
typedef Vec3<uchar> Vec3b;
typedef Vec3<float> Vec3f;

struct Scalar {
    double v[4];
    double operator[](int k) const { return v[k]; }
};

struct Range {
    int start, end;
    Range(int s, int e) : start(s), end(e) {}
};

struct Mat {
    int rows, cols;
    uchar* data;   // borrowed, row-major, ch interleaved bytes per pixel
    int ch;
    Mat() : rows(0), cols(0), data(nullptr), ch(1) {}
    Mat(int r, int c, int channels_, uchar* borrowed) : rows(r), cols(c), data(borrowed), ch(channels_) {}
    int channels() const { return ch; }
    template <typename T> T& at(int i, int j) const
    {
        return *reinterpret_cast<T*>(data + (size_t(i) * cols + j) * ch);
    }
    Mat operator()(const Range&, const Range&) const { shim_unpinned("Mat::operator()(Range, Range)"); }
};

inline Mat operator-(const Mat&, const Mat&) { shim_unpinned("Mat - Mat"); }
inline Mat abs(const Mat&) { shim_unpinned("cv::abs"); }
inline Scalar sum(const Mat&) { shim_unpinned("cv::sum"); }
inline Scalar mean(const Mat&) { shim_unpinned("cv::mean"); }
inline void absdiff(const Mat&, const Mat&, Mat&) { shim_unpinned("cv::absdiff"); }
inline void cvtColor(const Mat&, const Mat&, int) { shim_unpinned("cv::cvtColor"); }

}  // namespace cv
