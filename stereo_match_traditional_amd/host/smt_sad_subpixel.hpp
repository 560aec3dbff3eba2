// smt_sad_subpixel.hpp -- C++ host-side mirror of include/smt_sad_subpixel.h, beside smt_host.hpp and in its manner:
// HOST pointers in and out, everything computed by libsmt_hip.so, errors thrown as std::runtime_error.  The sub-pixel
// counterparts of GetPointDepthLeft / Right / Both and SadFlow: the value OptimalDisparity computes at Sad.h:76-81 and
// drops.  min_den is the clamp of the parabola's denominator (the literal 1 of Sad.h:80).
#pragma once
#include "smt_host.hpp"
#include "../../include/smt_sad_subpixel.h"

namespace smt {

// GetPointDepthLeft / GetPointDepthRight with the parabola kept: disparity float [rows-2w][cols-2w], w = winsize+1;
// winner (may be null) int, exactly GetPointDepth's map
inline void GetPointDepthSubpixel(float *disparity, int *winner, const unsigned char *leftimg, const unsigned char *rightimg,
                                  int rows, int cols, int MaxDisparity, int winsize, bool left_view, float min_den = 1.0f)
{
    int H, W;
    inner_size_(rows, cols, winsize + 1, H, W);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols);
    DevBuf<float> d((size_t)H * W);
    DevBuf<int> win((size_t)H * W);
    L.upload(leftimg); R.upload(rightimg);
    const smt_subpixel_params p = {min_den};
    check(smt_sad_subpixel(L.get(), R.get(), H, W, MaxDisparity, winsize, left_view ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, &p,
                           d.get(), win.get(), nullptr), "smt_sad_subpixel");
    d.download(disparity);
    if (winner) win.download(winner);
}

// both views from one evaluation of the hypotheses (smt_sad_both_subpixel); padded host images; the winners may be null
inline void GetPointDepthBothSubpixel(float *dispLeft, float *dispRight, int *winLeft, int *winRight,
                                      const unsigned char *leftimg, const unsigned char *rightimg, int rows, int cols,
                                      int MaxDisparity, int winsize, float min_den = 1.0f)
{
    int H, W;
    inner_size_(rows, cols, winsize + 1, H, W);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols);
    DevBuf<float> dl((size_t)H * W), dr((size_t)H * W);
    DevBuf<int> wl((size_t)H * W), wr((size_t)H * W);
    L.upload(leftimg); R.upload(rightimg);
    const smt_subpixel_params p = {min_den};
    check(smt_sad_both_subpixel(L.get(), R.get(), H, W, MaxDisparity, winsize, &p, dl.get(), dr.get(), wl.get(), wr.get(),
                                nullptr, nullptr), "smt_sad_both_subpixel");
    dl.download(dispLeft); dr.download(dispRight);
    if (winLeft) wl.download(winLeft);
    if (winRight) wr.download(winRight);
}

// SadFlow with sub-pixel maps (smt_sad_flow_run_batch_subpixel): UNPADDED gray pairs, host buffers in and out
class SadSubpixelFlow {
public:
    SadSubpixelFlow(int rows, int cols, int MaxDisparity, int winsize = 3, float min_den = 1.0f, int device = 0)
        : n_((size_t)rows * cols), min_den_(min_den)
    {
        smt_sad_params p;
        smt_sad_default_params(&p);
        p.winsize = winsize;
        check(smt_sad_flow_create_on(device, rows, cols, MaxDisparity, &p, &h_), "smt_sad_flow_create_on");
    }
    ~SadSubpixelFlow() { if (h_) smt_sad_flow_destroy(h_); }
    SadSubpixelFlow(const SadSubpixelFlow &) = delete;
    SadSubpixelFlow &operator=(const SadSubpixelFlow &) = delete;
    // grayL, grayR: uchar [pairs][rows][cols]; depthleft, depthright, lastdisp: float [pairs][rows][cols], cls: uchar
    // (any may be null); lastdisp is depthleft where the cross-check accepts, +inf where it rejects
    void run(const unsigned char *grayL, const unsigned char *grayR, int pairs, float *depthleft, float *depthright,
             float *lastdisp, unsigned char *cls = nullptr)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n), c(n);
        DevBuf<float> dl(n), dr(n), last(n);
        L.upload(grayL); R.upload(grayR);
        const smt_subpixel_params p = {min_den_};
        check(smt_sad_flow_run_batch_subpixel(h_, L.get(), R.get(), pairs, &p, dl.get(), dr.get(), last.get(), c.get()),
              "smt_sad_flow_run_batch_subpixel");
        if (depthleft) dl.download(depthleft);
        if (depthright) dr.download(depthright);
        if (lastdisp) last.download(lastdisp);
        if (cls) c.download(cls);
    }
private:
    smt_sad_flow *h_ = nullptr;
    size_t n_;
    float min_den_;
};

}  // namespace smt
