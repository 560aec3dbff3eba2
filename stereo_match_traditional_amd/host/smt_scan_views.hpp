// smt_scan_views.hpp -- C++ host-side mirror of include/smt_scan_views.h, beside smt_host.hpp and in its manner: HOST
// pointers in and out, everything computed by libsmt_hip.so, errors thrown as std::runtime_error.  ScanlineOptimizer on
// two views at once (ScanLinePair), maps only (ScanLineMap), and the batched main.cpp pipeline with the right view
// scanline-optimised too (ScanViewsPipeline).
#pragma once
#include "smt_host.hpp"
#include "../../include/smt_scan_views.h"

namespace smt {

// ScanlineOptimizer.h:8-34 on two volumes of one shape.  setQuirks / setSubpixel as ScanlineOptimizer's, kept across
// Initialize and acting on both views.
class ScanlinePairOptimizer {
public:
    ScanlinePairOptimizer() = default;
    ~ScanlinePairOptimizer() { if (h_) smt_scanline_destroy(h_); }
    ScanlinePairOptimizer(const ScanlinePairOptimizer &) = delete;
    ScanlinePairOptimizer &operator=(const ScanlinePairOptimizer &) = delete;
    void Initialize(int row, int col, int dispRange, int p1, int p2)
    {
        row_ = row; col_ = col; D_ = dispRange;
        if (h_) { smt_scanline_destroy(h_); h_ = nullptr; }
        check(smt_scanline_create(row, col, dispRange, p1, p2, &h_), "smt_scanline_create");
        if (quirks_) check(smt_scanline_set_quirks(h_, quirks_), "smt_scanline_set_quirks");
        apply_subpixel();
    }
    void setSubpixel(float min_den)
    {
        sub_ = min_den;
        if (h_) apply_subpixel();
    }
    void setQuirks(unsigned quirks)
    {
        if (h_) check(smt_scanline_set_quirks(h_, quirks), "smt_scanline_set_quirks");
        quirks_ = quirks;
    }
    // costL / costR float [row][col][dispRange], ImageL / ImageR float [row][col].  outL / outR (the summed volumes) may
    // be null when the view's disp is not: that view runs the maps-only last pass.  A view needs one of the two.
    void ScanLinePair(const float *costL, const float *ImageL, const float *costR, const float *ImageR, float *outL,
                      float *dispL, float *outR, float *dispR)
    {
        const size_t n = (size_t)row_ * col_;
        DevBuf<float> inL(n * D_), inR(n * D_), gL(n), gR(n), dL, dR, oL, oR;
        inL.upload(costL); inR.upload(costR); gL.upload(ImageL); gR.upload(ImageR);
        if (outL) oL.resize(n * D_);
        if (outR) oR.resize(n * D_);
        if (dispL) dL.resize(n);
        if (dispR) dR.resize(n);
        check(smt_scanline_run_pair(h_, inL.get(), gL.get(), oL.get(), dL.get(), inR.get(), gR.get(), oR.get(), dR.get()),
              "smt_scanline_run_pair");
        if (outL) oL.download(outL);
        if (outR) oR.download(outR);
        if (dispL) dL.download(dispL);
        if (dispR) dR.download(dispR);
    }
    // one view, the map only
    void ScanLineMap(const float *costVolume, const float *Image, float *disp)
    {
        const size_t n = (size_t)row_ * col_;
        DevBuf<float> in(n * D_), g(n), d(n);
        in.upload(costVolume); g.upload(Image);
        check(smt_scanline_run_map(h_, in.get(), g.get(), d.get()), "smt_scanline_run_map");
        d.download(disp);
    }
private:
    void apply_subpixel()
    {
        const smt_subpixel_params sp{sub_};
        check(smt_scanline_set_subpixel(h_, sub_ != 0.0f ? &sp : nullptr), "smt_scanline_set_subpixel");
    }
    float sub_ = 0.0f;
    smt_scanline *h_ = nullptr;
    unsigned quirks_ = 0;
    int row_ = 0, col_ = 0, D_ = 0;
};

// smt::Pipeline with smt_pipeline_set_scan_views: host buffers in and out as Pipeline's, any output may be null.
class ScanViewsPipeline {
public:
    ScanViewsPipeline(int row, int col, int dispRange, int views = SMT_VIEW_BOTH, const smt_pipeline_params *p = nullptr)
        : row_(row), col_(col), D_(dispRange)
    {
        check(smt_pipeline_create(row, col, dispRange, p, &h_), "smt_pipeline_create");
        const int rc = smt_pipeline_set_scan_views(h_, views);
        if (rc != SMT_OK) { smt_pipeline_destroy(h_); h_ = nullptr; check(rc, "smt_pipeline_set_scan_views"); }
    }
    ~ScanViewsPipeline() { if (h_) smt_pipeline_destroy(h_); }
    ScanViewsPipeline(const ScanViewsPipeline &) = delete;
    ScanViewsPipeline &operator=(const ScanViewsPipeline &) = delete;
    void setScanViews(int views) { check(smt_pipeline_set_scan_views(h_, views), "smt_pipeline_set_scan_views"); }
    void setQuirks(unsigned quirks) { check(smt_pipeline_set_quirks(h_, quirks), "smt_pipeline_set_quirks"); }
    void setSubpixel(float min_den)
    {
        const smt_subpixel_params sp{min_den};
        check(smt_pipeline_set_subpixel(h_, min_den != 0.0f ? &sp : nullptr), "smt_pipeline_set_subpixel");
    }
    void RunBatch(const unsigned char *grayL, const unsigned char *grayR, int pairs, float *dispL, float *dispR, unsigned char *cls)
    {
        const size_t n = batch_elems_((size_t)row_ * col_, pairs);
        DevBuf<unsigned char> l(n), r(n), c(n);
        DevBuf<float> dl(n), dr(n);
        l.upload(grayL); r.upload(grayR);
        check(smt_pipeline_run_batch(h_, l.get(), r.get(), pairs, dl.get(), dr.get(), c.get(), nullptr), "smt_pipeline_run_batch");
        check(smt_pipeline_status(h_), "smt_pipeline_status");
        if (dispL) dl.download(dispL);
        if (dispR) dr.download(dispR);
        if (cls) c.download(cls);
    }
    // the right view's scanline sum of the last pair of the last BOTH RunBatch, float [row][col][dispRange]
    void ScanRightVolume(float *sum)
    {
        float *p = nullptr;
        check(smt_pipeline_scan_right_volume(h_, &p), "smt_pipeline_scan_right_volume");
        check(smt_memcpy_d2h(sum, p, (size_t)row_ * col_ * D_ * sizeof(float), nullptr), "d2h");
        check(smt_stream_sync(nullptr), "sync");
    }
private:
    smt_pipeline *h_ = nullptr;
    int row_, col_, D_;
};

}  // namespace smt
