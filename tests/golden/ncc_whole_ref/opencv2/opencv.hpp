// Stand-in for <opencv2/opencv.hpp>, used ONLY by tests/golden/make_ncc_whole_golden.py to compile the reference's
// NCC/NCC.h, unmodified and where it lies, into a throw-away program that records ncc() and bgr_to_grey().
// Test infrastructure; this file is our own text.
//
// It provides the pixel CONTAINER those two functions use and nothing that computes: an owning Mat(rows, cols, type) that
// is ZERO-FILLED (OpenCV leaves it uninitialised: a pixel ncc() never writes reads as 0 here) and shares its data on copy
// as cv::Mat does, size(), at<T>, ptr<T>, Vec3b, and the Microsoft literal suffix ui8 of NCC.h:7.  What the header's other
// functions need from OpenCV -- ROI by Range, cv::mean -- and `Mat += int` (add_constant, NCC.h:129) are declared so that
// the header parses, and abort when reached: nothing recorded depends on OpenCV arithmetic.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

typedef unsigned char uchar;
#define CV_8UC1 0
#define CV_8UC3 16

// `0xffui8` (NCC.h:7): an unsigned 8-bit literal in Microsoft's dialect
constexpr unsigned char operator""ui8(unsigned long long v) { return (unsigned char)v; }

namespace cv {

[[noreturn]] inline void shim_unpinned(const char *what)
{
    std::fprintf(stderr, "opencv shim: %s is not provided\n", what);
    std::abort();
}

struct Vec3b {
    uchar v[3];
    uchar &operator[](int k) { return v[k]; }
    const uchar &operator[](int k) const { return v[k]; }
};

struct Scalar { double val[4]; };
struct Size { int width, height; };
struct Range {
    int start, end;
    Range(int s, int e) : start(s), end(e) {}
};

struct Mat {
    int rows = 0, cols = 0, esz = 1;
    std::shared_ptr<std::vector<uchar>> store;
    Mat() {}
    Mat(int r, int c, int type) : rows(r), cols(c), esz(type == CV_8UC3 ? 3 : 1),
                                  store(std::make_shared<std::vector<uchar>>((size_t)r * c * (type == CV_8UC3 ? 3 : 1), (uchar)0)) {}
    Size size() const { return Size{cols, rows}; }
    uchar *bytes() const { return store->data(); }
    template <typename T> T &at(int i, int j) const { return *reinterpret_cast<T *>(bytes() + ((size_t)i * cols + j) * esz); }
    template <typename T> T *ptr(int i) const { return reinterpret_cast<T *>(bytes() + (size_t)i * cols * esz); }
    Mat operator()(const Range &, const Range &) const { shim_unpinned("Mat::operator()(Range, Range)"); }
    Mat &operator+=(int) { shim_unpinned("Mat += int"); }
};

inline Scalar mean(const Mat &) { shim_unpinned("cv::mean"); }

}  // namespace cv
