// smt_bilateral.hpp -- C++ host-side mirror of include/smt_bilateral.h, beside smt_host.hpp and in its manner: HOST
// pointers in and out, everything computed by libsmt_hip.so, errors thrown as std::runtime_error.  The three functions of
// ASW/BiliteralFilter.h:12-142 under their own names; bilateralfiterWight (:145-242) does not compile and has none.
#pragma once
#include "smt_host.hpp"
#include "../../include/smt_bilateral.h"

namespace smt {

// cv::Size as the reference passes it: Size(width, height)
struct Size {
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h) : width(w), height(h) {}
};

// getGausssianMask (:12-31): Mask becomes wsize.height x wsize.width, row stride wsize.width
inline void getGausssianMask(std::vector<double> &Mask, Size wsize, double spaceSigma = 10)
{
    if (wsize.height < 1 || wsize.width < 1) check(SMT_ERR_ARG, "getGausssianMask");
    Mask.assign((size_t)wsize.height * wsize.width, 0.0);
    double color[256];
    check(smt_bilateral_masks(wsize.height, wsize.width, spaceSigma, 1.0, Mask.data(), color), "smt_bilateral_masks");
}

// getColorMask (:36-43): appends the 256 entries, as the reference's push_back does
inline void getColorMask(std::vector<double> &colorMask, double colorSigma = 30)
{
    double space[1], color[256];
    check(smt_bilateral_masks(1, 1, 1.0, colorSigma, space, color), "smt_bilateral_masks");
    colorMask.insert(colorMask.end(), color, color + 256);
}

// bilateralfiter (:49-142): src, dst uchar [rows][cols][channels], channels 1 or 3; acc (may be null) double of the same
// shape, the unclamped sums; norm SMT_BILATERAL_NORM_RECIPROCAL (what OpenCV 3.1's Mat / double evaluates) or _DIVIDE
inline void bilateralfiter(const unsigned char *src, unsigned char *dst, int rows, int cols, int channels, Size wsize,
                           double spaceSigma, double colorSigma, int norm = SMT_BILATERAL_NORM_RECIPROCAL,
                           double *acc = nullptr)
{
    if (rows <= 0 || cols <= 0 || (channels != 1 && channels != 3)) check(SMT_ERR_ARG, "bilateralfiter");
    std::vector<double> space, color;
    getGausssianMask(space, wsize, spaceSigma);
    getColorMask(color, colorSigma);
    const size_t n = (size_t)rows * cols * channels;
    DevBuf<unsigned char> s(n), d(n);
    DevBuf<double> sp(space.size()), cm(color.size());
    s.upload(src); sp.upload(space.data()); cm.upload(color.data());
    if (acc) {
        DevBuf<double> a(n);
        check(smt_bilateral_filter_batch(s.get(), 1, rows, cols, channels, wsize.height, wsize.width, sp.get(), cm.get(), norm,
                                         d.get(), a.get(), nullptr), "smt_bilateral_filter_batch");
        a.download(acc);
    } else {
        check(smt_bilateral_filter_batch(s.get(), 1, rows, cols, channels, wsize.height, wsize.width, sp.get(), cm.get(), norm,
                                         d.get(), nullptr, nullptr), "smt_bilateral_filter_batch");
    }
    d.download(dst);
}

// the same on an Image (imread's B, G, R or gray)
inline Image bilateralfiter(const Image &src, Size wsize, double spaceSigma, double colorSigma,
                            int norm = SMT_BILATERAL_NORM_RECIPROCAL)
{
    check_image_(src, "bilateralfiter: image");
    Image dst;
    dst.rows = src.rows; dst.cols = src.cols; dst.channels = src.channels;
    dst.data.resize(src.data.size());
    bilateralfiter(src.data.data(), dst.data.data(), src.rows, src.cols, src.channels, wsize, spaceSigma, colorSigma, norm);
    return dst;
}

}  // namespace smt
