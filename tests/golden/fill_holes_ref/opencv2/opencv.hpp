// Stand-in for <opencv2/opencv.hpp>, used ONLY by tests/golden/make_fill_holes_golden.py to compile the reference's
// SAD/Sad.h, unmodified and where it lies, into a throw-away program that records tests/golden/fill_holes_ref.npz.
// Test infrastructure; this file is our own text.
//
// It provides the pixel CONTAINER Sad.h uses and nothing that computes: Mat with rows / cols / channels() / at<T>() /
// ptr<T>() over a buffer that copies SHARE (`Mat disp_ptr = disp_left_` is how FillHolesInDispMap writes through a
// const Mat&).  Every OpenCV operation with arithmetic is declared so that the header parses, and aborts when reached:
// Mat - Mat, cv::abs, cv::sum, normalize, convertTo, cvtColor and ROI by Range.  FillHolesInDispMap reaches none of them.
//
// at<T>() reports every access to shim_on_access when the driver has set one: that is how the driver sees where the
// third pass starts (its scan reads every pixel once, in raster order) without a change to the function.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <memory>

typedef unsigned char uchar;
#define CV_BGR2GRAY 6
#define CV_8UC1 0

namespace cv {

enum { NORM_MINMAX = 32 };

[[noreturn]] inline void shim_unpinned(const char* what)
{
    std::fprintf(stderr, "opencv shim: %s is not provided (the caller is not pinned)\n", what);
    std::abort();
}

inline void (*shim_on_access)(int, int) = nullptr;

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
    size_t elem;                          // bytes per pixel
    int ch;
    std::shared_ptr<uchar> buf;           // shared by every copy
    Mat() : rows(0), cols(0), elem(1), ch(1) {}
    Mat(int r, int c, size_t elem_bytes) : rows(r), cols(c), elem(elem_bytes), ch(1),
        buf(new uchar[size_t(r) * c * elem_bytes](), std::default_delete<uchar[]>()) {}
    int channels() const { return ch; }
    uchar* data() const { return buf.get(); }
    template <typename T> T& at(int i, int j) const
    {
        if (i < 0 || i >= rows || j < 0 || j >= cols || sizeof(T) != elem) shim_unpinned("Mat::at outside the buffer");
        if (shim_on_access) shim_on_access(i, j);
        return *reinterpret_cast<T*>(buf.get() + (size_t(i) * cols + j) * elem);
    }
    template <typename T> T* ptr(int i) const { return reinterpret_cast<T*>(buf.get() + size_t(i) * cols * elem); }
    Mat operator()(const Range&, const Range&) const { shim_unpinned("Mat::operator()(Range, Range)"); }
    void convertTo(Mat&, int) const { shim_unpinned("Mat::convertTo"); }
};

inline Mat operator-(const Mat&, const Mat&) { shim_unpinned("Mat - Mat"); }
inline Mat abs(const Mat&) { shim_unpinned("cv::abs"); }
inline Scalar sum(const Mat&) { shim_unpinned("cv::sum"); }
inline void normalize(const Mat&, Mat&, double, double, int) { shim_unpinned("cv::normalize"); }
inline void cvtColor(const Mat&, const Mat&, int) { shim_unpinned("cv::cvtColor"); }

}  // namespace cv
