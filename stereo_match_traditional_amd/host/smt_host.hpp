// smt_host.hpp -- C++ host-side mirror of the reference's classes over the C ABI (smt.h).
//
// Same class names, method names, argument order and HOST-pointer ownership as the
// reference (AD-CensusV1/{AD-Census.h,CrossArm.h,ScanlineOptimizer.h,PostProcessing.h},
// CBLSM/cross_aggregator.h), so that the reference's main()s compile against this header
// instead of their own after dropping the cv::Mat arguments.  Every
// method uploads / downloads through smt_memcpy_* and runs the HIP kernels of
// libsmt_hip.so; there is no CPU implementation behind it.
//
// Deviations (all forced by the missing OpenCV dependency, none changes results):
//   - cv::Mat parameters become (const unsigned char* data, int channels).
//   - Errors: the reference returns void and has UB on bad input; these methods throw
//     std::runtime_error carrying smt_strerror().  What the C entry cannot see is checked here, before any device work: a
//     negative pair count, a padded image smaller than its border, ASW masks of another window size, an Image whose
//     vector does not hold rows * cols * channels bytes, CrossAggregator::Aggregate without SetData.
//   - The classes that own a handle are not copyable.
// tests/test_cpp_mirror_cpu.py runs every function here against a contract stub of smt.h under AddressSanitizer and
// holds this file to its case table: a new function needs a case there (or a stated reason).
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/smt.h"

namespace smt {

inline void check(int rc, const char *what)
{
    if (rc != SMT_OK) throw std::runtime_error(std::string(what) + ": " + smt_strerror(rc));
}

// elements of a batch of `pairs` maps of `per` elements; a negative count must not reach a size_t product
inline size_t batch_elems_(size_t per, int pairs)
{
    if (pairs < 0) check(SMT_ERR_ARG, "pairs");
    return per * (size_t)pairs;
}
// the unpadded size of an image padded by w on every side (the window matchers' rows / cols are the padded ones)
inline void inner_size_(int rows, int cols, int w, int &H, int &W)
{
    H = rows - 2 * w; W = cols - 2 * w;
    if (w < 1 || H <= 0 || W <= 0) check(SMT_ERR_ARG, "padded image smaller than its border");
}

// RAII device buffer
template <class T> class DevBuf {
public:
    DevBuf() = default;
    explicit DevBuf(size_t n) { resize(n); }
    ~DevBuf() { if (p_) smt_free(p_); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    void resize(size_t n)
    {
        if (p_) smt_free(p_);
        p_ = nullptr; n_ = n;
        void *q = nullptr;
        check(smt_malloc(&q, n * sizeof(T)), "smt_malloc");
        p_ = static_cast<T *>(q);
    }
    void upload(const T *h) { check(smt_memcpy_h2d(p_, h, n_ * sizeof(T), nullptr), "h2d"); }
    void download(T *h) const
    {
        check(smt_memcpy_d2h(h, p_, n_ * sizeof(T), nullptr), "d2h");
        check(smt_stream_sync(nullptr), "sync");
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }
private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

// ------------------------------------------------------------------ AD-Census.h:9-43
class AD_Census {
public:
    AD_Census() = default;
    ~AD_Census() { if (h_) smt_adcensus_destroy(h_); }
    // Initialize(leftImage, rightImage, dispRange, row, col, LImage, RImage, sigmaC, sigmaS)
    void Initialize(float *leftImage, float *rightImage, int dispRange, int row, int col, float sigmaC,
                    float sigmaS)
    {
        row_ = row; col_ = col; D_ = dispRange;
        if (h_) { smt_adcensus_destroy(h_); h_ = nullptr; }
        check(smt_adcensus_create(row, col, dispRange, sigmaC, sigmaS, &h_), "smt_adcensus_create");
        if (quirks_) check(smt_adcensus_set_quirks(h_, quirks_), "smt_adcensus_set_quirks");
        L_.resize((size_t)row * col); R_.resize((size_t)row * col);
        L_.upload(leftImage); R_.upload(rightImage);
        hostL_.assign((size_t)row * col * dispRange, 0.f);
        hostR_.assign((size_t)row * col * dispRange, 0.f);
        validL_ = validR_ = false;
    }
    // SMT_QUIRK_* (SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE acts here); 0 = the reference's results.  Kept across Initialize.
    void setQuirks(unsigned quirks)
    {
        if (h_) check(smt_adcensus_set_quirks(h_, quirks), "smt_adcensus_set_quirks");
        quirks_ = quirks;
    }
    void ComputeADcensus() { check(smt_adcensus_compute(h_, L_.get(), R_.get(), SMT_VIEW_LEFT, nullptr, nullptr), "compute"); validL_ = false; }
    void ComputeADcensusRight() { check(smt_adcensus_compute(h_, L_.get(), R_.get(), SMT_VIEW_RIGHT, nullptr, nullptr), "compute"); validR_ = false; }
    // device-side volume (borrowed), for chaining into CrossArmAggregation without a round trip
    float *DevicePtrLeft() { float *p; check(smt_adcensus_volume(h_, SMT_VIEW_LEFT, &p), "volume"); return p; }
    float *DevicePtrRight() { float *p; check(smt_adcensus_volume(h_, SMT_VIEW_RIGHT, &p), "volume"); return p; }
    // GetPtrLeft/Right: host copy of the cost volume, valid for the object's life like the reference's
    // (bad input -- a pixel that is not an integer in 0..255 -- is reported here, at the first point
    // where the reference's caller would consume the volume: smt_adcensus_status)
    float *GetPtrLeft()
    {
        if (!validL_) { check(smt_adcensus_status(h_), "smt_adcensus_status"); fetch(DevicePtrLeft(), hostL_); validL_ = true; }
        return hostL_.data();
    }
    float *GetPtrRight()
    {
        if (!validR_) { check(smt_adcensus_status(h_), "smt_adcensus_status"); fetch(DevicePtrRight(), hostR_); validR_ = true; }
        return hostR_.data();
    }
    void WTA(float *leftdisp, float *rightDisp)
    {
        const size_t n = (size_t)row_ * col_;
        DevBuf<float> dl(n), dr(n);
        check(smt_wta(DevicePtrLeft(), row_, col_, D_, dl.get(), nullptr), "wta");
        check(smt_wta(DevicePtrRight(), row_, col_, D_, dr.get(), nullptr), "wta");
        dl.download(leftdisp); dr.download(rightDisp);
        check(smt_adcensus_status(h_), "smt_adcensus_status");
    }
private:
    void fetch(const float *dev, std::vector<float> &host)
    {
        check(smt_memcpy_d2h(host.data(), dev, host.size() * sizeof(float), nullptr), "d2h");
        check(smt_stream_sync(nullptr), "sync");
    }
    smt_adcensus *h_ = nullptr;
    unsigned quirks_ = 0;
    int row_ = 0, col_ = 0, D_ = 0;
    DevBuf<float> L_, R_;
    std::vector<float> hostL_, hostR_;
    bool validL_ = false, validR_ = false;
};

// ------------------------------------------------------------------ CrossArm.h:9-36
class CrossArmAggregation {
public:
    CrossArmAggregation() = default;
    CrossArmAggregation(const CrossArmAggregation &) = delete;            // one owner per handle
    CrossArmAggregation &operator=(const CrossArmAggregation &) = delete;
    ~CrossArmAggregation() { if (h_) smt_crossarm_destroy(h_); }
    void Initialize(int row, int col, float * /*leftImage*/, float * /*rightImage*/, int tao, int dispRange)
    {
        row_ = row; col_ = col; D_ = dispRange;
        if (h_) { smt_crossarm_destroy(h_); h_ = nullptr; }
        smt_crossarm_params p;
        smt_crossarm_default_params(&p);
        p.tau = tao;
        p.quirks = quirks_;
        check(smt_crossarm_create(row, col, dispRange, &p, &h_), "smt_crossarm_create");
        apply_subpixel();
        started_ = false;
    }
    // Sub-pixel switch (smt_crossarm_set_subpixel): min_den > 0 = WTA and the device map of AggregationVerticalDevice
    // are refined by the parabola rule, 0 = integer maps (the default).  Kept across Initialize.
    void setSubpixel(float min_den)
    {
        sub_ = min_den;
        if (h_) apply_subpixel();
    }
    // SMT_QUIRK_* (SMT_QUIRK_FIX_RIGHT_ARM_STRIDE and SMT_QUIRK_FIX_STICKY_TAU act here); 0 = the reference's results.
    // They are parameters of the handle: call it before Initialize, which every use of the class starts with.
    void setQuirks(unsigned quirks) { quirks_ = quirks; }
    // The four Compute*ArmLength(const Mat&) calls of main.cpp:69-72 always come together and in
    // this order (the threshold state chains through them), so they are one call here.
    void ComputeArmLengths(const unsigned char *image, int channels)
    {
        DevBuf<unsigned char> img((size_t)row_ * col_ * channels);
        img.upload(image);
        check(smt_crossarm_arms(h_, img.get(), channels), "smt_crossarm_arms");
        check(smt_stream_sync(nullptr), "sync");
    }
    // The reference's four calls one by one (CrossArm.h:15-18), for callers that run a subset or another
    // order; the sticky threshold is whatever the previous call left.  Initialize resets it.
    void ComputeLeftArmLength(const unsigned char *image, int channels) { arm_dir(image, channels, 0); }
    void ComputeRightArmLength(const unsigned char *image, int channels) { arm_dir(image, channels, 1); }
    void ComputeTopArmLength(const unsigned char *image, int channels) { arm_dir(image, channels, 2); }
    void ComputeButtonArmLength(const unsigned char *image, int channels) { arm_dir(image, channels, 3); }
    // CrossArm.cpp:104-145 (declared in CrossArm.h:19, never called): exclusive upper bounds
    void Aggregation(float *dispVolume, float *aggregatedCostVolume)
    {
        const size_t V = (size_t)row_ * col_ * D_;
        DevBuf<float> in(V), out(V);
        in.upload(dispVolume);
        check(smt_crossarm_aggregate(h_, in.get(), out.get(), 2, nullptr), "smt_crossarm_aggregate");
        out.download(aggregatedCostVolume);
        check(smt_crossarm_status(h_), "smt_crossarm_status");
    }
    void AggregationVertical(float *dispVolume, float *aggregatedCostVolume)
    {
        const size_t V = (size_t)row_ * col_ * D_;
        DevBuf<float> in(V), out(V);
        in.upload(dispVolume);
        AggregationVerticalDevice(in.get(), out.get());
        out.download(aggregatedCostVolume);
        check(smt_crossarm_status(h_), "smt_crossarm_status");
    }
    void AggregationVerticalDevice(const float *dev_in, float *dev_out, float *dev_disp = nullptr)
    {
        check(smt_crossarm_aggregate(h_, dev_in, dev_out, 0, dev_disp), "smt_crossarm_aggregate");
    }
    void WTA(float *AggredCostVolume, float *disp)
    {
        const size_t n = (size_t)row_ * col_;
        DevBuf<float> v(n * D_), d(n);
        v.upload(AggredCostVolume);
        if (sub_ != 0.0f) { const smt_subpixel_params sp{sub_}; check(smt_wta_subpixel(v.get(), row_, col_, D_, &sp, d.get(), nullptr), "wta_subpixel"); }
        else check(smt_wta(v.get(), row_, col_, D_, d.get(), nullptr), "wta");
        d.download(disp);
    }
private:
    void apply_subpixel()
    {
        const smt_subpixel_params sp{sub_};
        check(smt_crossarm_set_subpixel(h_, sub_ != 0.0f ? &sp : nullptr), "smt_crossarm_set_subpixel");
    }
    float sub_ = 0.0f;
    void arm_dir(const unsigned char *image, int channels, int dir)
    {
        DevBuf<unsigned char> img((size_t)row_ * col_ * channels);
        img.upload(image);
        if (!started_) { check(smt_crossarm_reset(h_), "smt_crossarm_reset"); started_ = true; }
        check(smt_crossarm_arm_dir(h_, img.get(), channels, dir), "smt_crossarm_arm_dir");
        check(smt_stream_sync(nullptr), "sync");
    }
    smt_crossarm *h_ = nullptr;
    unsigned quirks_ = 0;
    int row_ = 0, col_ = 0, D_ = 0;
    bool started_ = false;
};

// ------------------------------------------------------------------ ScanlineOptimizer.h:8-34
class ScanlineOptimizer {
public:
    ScanlineOptimizer() = default;
    ~ScanlineOptimizer() { if (h_) smt_scanline_destroy(h_); }
    void Initialize(int row, int col, int dispRange, float * /*costVolume*/, int p1, int p2)
    {
        row_ = row; col_ = col; D_ = dispRange;
        if (h_) { smt_scanline_destroy(h_); h_ = nullptr; }
        check(smt_scanline_create(row, col, dispRange, p1, p2, &h_), "smt_scanline_create");
        if (quirks_) check(smt_scanline_set_quirks(h_, quirks_), "smt_scanline_set_quirks");
        apply_subpixel();
        processed_.resize((size_t)row * col * dispRange);
    }
    // Sub-pixel switch (smt_scanline_set_subpixel): min_den > 0 = WTA gives the winner refined by the parabola rule,
    // 0 = the integer map (the default).  Kept across Initialize.
    void setSubpixel(float min_den)
    {
        sub_ = min_den;
        if (h_) apply_subpixel();
    }
    // SMT_QUIRK_* (SMT_QUIRK_FIX_SCAN_VERTICAL acts here); 0 = the reference's results.  Kept across Initialize.
    void setQuirks(unsigned quirks)
    {
        if (h_) check(smt_scanline_set_quirks(h_, quirks), "smt_scanline_set_quirks");
        quirks_ = quirks;
    }
    void ScanLine(float *costVolume, float *Image)
    {
        const size_t n = (size_t)row_ * col_;
        DevBuf<float> in(n * D_), g(n);
        in.upload(costVolume); g.upload(Image);
        check(smt_scanline_run(h_, in.get(), g.get(), processed_.get(), nullptr), "smt_scanline_run");
        check(smt_stream_sync(nullptr), "sync");
    }
    void WTA(float *disp)
    {
        DevBuf<float> d((size_t)row_ * col_);
        if (sub_ != 0.0f) { const smt_subpixel_params sp{sub_}; check(smt_wta_subpixel(processed_.get(), row_, col_, D_, &sp, d.get(), nullptr), "wta_subpixel"); }
        else check(smt_wta(processed_.get(), row_, col_, D_, d.get(), nullptr), "wta");
        d.download(disp);
    }
    float *DeviceProcessedVolume() { return processed_.get(); }
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
    DevBuf<float> processed_;
};

// ------------------------------------------------------------------ PostProcessing.h:72
inline void LeftRightConsistency(int col, int row, int gate, float *leftDisp, float *rightDisp,
                                 std::vector<std::pair<int, int>> &occlusion,
                                 std::vector<std::pair<int, int>> &mismatch)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> dl(n), dr(n);
    DevBuf<uint8_t> cls(n);
    dl.upload(leftDisp); dr.upload(rightDisp);
    check(smt_lrcheck(dl.get(), dr.get(), row, col, gate, cls.get(), nullptr, nullptr), "smt_lrcheck");
    dl.download(leftDisp);
    std::vector<uint8_t> h(n);
    cls.download(h.data());
    std::vector<int> o(2 * n), m(2 * n);
    int no = 0, nm = 0;
    check(smt_lrcheck_lists(h.data(), row, col, o.data(), &no, m.data(), &nm), "smt_lrcheck_lists");
    occlusion.clear(); mismatch.clear();
    for (int k = 0; k < no; k++) occlusion.emplace_back(o[2 * k], o[2 * k + 1]);
    for (int k = 0; k < nm; k++) mismatch.emplace_back(m[2 * k], m[2 * k + 1]);
}

// ------------------------------------------------------------------ PostProcessing.h:10 (no call site)
inline void LeftAndRightConsistency(float *leftDisp, float *rightDisp, float *lastDisp, int col, int row, float gate,
                                    std::vector<std::pair<int, int>> &occlusion,
                                    std::vector<std::pair<int, int>> &mismatch)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> dl(n), dr(n), last(n);
    DevBuf<uint8_t> cls(n);
    dl.upload(leftDisp); dr.upload(rightDisp);
    check(smt_lrcheck_variant(dl.get(), dr.get(), last.get(), row, col, gate, cls.get(), nullptr, nullptr), "smt_lrcheck_variant");
    last.download(lastDisp);
    std::vector<uint8_t> h(n);
    cls.download(h.data());
    std::vector<int> o(2 * n), m(2 * n);
    int no = 0, nm = 0;
    check(smt_lrcheck_lists(h.data(), row, col, o.data(), &no, m.data(), &nm), "smt_lrcheck_lists");
    for (int k = 0; k < no; k++) occlusion.emplace_back(o[2 * k], o[2 * k + 1]);     // the reference appends (:44, :47)
    for (int k = 0; k < nm; k++) mismatch.emplace_back(m[2 * k], m[2 * k + 1]);
}

// ------------------------------------------------------------------ PostProcessing.h:156
// Same signature and side effects as the reference, the replaced `mismatch` list included (:186).
inline void FillTheHole(const int row, const int col, const int dispRange, float *dispLeft,
                        std::vector<std::pair<int, int>> &occlusion, std::vector<std::pair<int, int>> &mismatch)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> d(n);
    d.upload(dispLeft);
    std::vector<int> o(2 * occlusion.size()), m(2 * mismatch.size()), third(2 * n);
    for (size_t k = 0; k < occlusion.size(); k++) { o[2 * k] = occlusion[k].first; o[2 * k + 1] = occlusion[k].second; }
    for (size_t k = 0; k < mismatch.size(); k++) { m[2 * k] = mismatch[k].first; m[2 * k + 1] = mismatch[k].second; }
    int nt = -1;
    check(smt_fill_the_hole(d.get(), row, col, dispRange, o.data(), (int)occlusion.size(), m.data(),
                            (int)mismatch.size(), third.data(), &nt, nullptr), "smt_fill_the_hole");
    d.download(dispLeft);
    if (nt >= 0) {
        mismatch.clear();
        for (int k = 0; k < nt; k++) mismatch.emplace_back(third[2 * k], third[2 * k + 1]);
    }
}

// FillTheHole on `pairs` host maps [pairs][row][col] with the lists LeftRightConsistency would have produced taken
// from the class maps (uint8, as smt_lrcheck writes them) on the device: one upload, smt_fill_the_hole_batch, one
// download.  status[b] = {n_occ, n_mis, n_third, flags} (SMT_FILL_UB_LIST / SMT_FILL_UB_THIRD: smt.h).
inline void FillTheHoleBatch(int pairs, int row, int col, int dispRange, float *disp, const uint8_t *cls,
                             std::vector<std::array<int, 4>> &status)
{
    status.assign(pairs > 0 ? (size_t)pairs : 0, std::array<int, 4>{{0, 0, -1, 0}});
    if (pairs <= 0) { check(pairs < 0 ? SMT_ERR_ARG : SMT_OK, "smt_fill_the_hole_batch"); return; }
    const size_t n = (size_t)pairs * row * col;
    DevBuf<float> d(n);
    DevBuf<uint8_t> c(n);
    DevBuf<int> st((size_t)pairs * 4);
    d.upload(disp);
    check(smt_memcpy_h2d(c.get(), cls, n, nullptr), "h2d");
    check(smt_fill_the_hole_batch(d.get(), c.get(), pairs, 0, 0, row, col, dispRange, st.get(), nullptr),
          "smt_fill_the_hole_batch");
    d.download(disp);
    st.download(&status[0][0]);
}

// ------------------------------------------------------------------ CBLSM.h:65-236
// chooseArmLength{Left,Right,Up,Down} on host arm maps (call sites commented out in CBLSM.cpp:108-111)
inline void choose_arm_length_(int dir, const int *own, const int *vert, const int *RL, const int *RR, int dispRange,
                               int *Armvolume, int row, int col)
{
    const size_t n = (size_t)row * col;
    DevBuf<int> a(n), v(n), l(n), r(n), out(n * dispRange);
    a.upload(own); l.upload(RL); r.upload(RR);
    if (vert) v.upload(vert);
    check(smt_cblsm_choose_arm_length(dir, a.get(), vert ? v.get() : nullptr, l.get(), r.get(), row, col, dispRange,
                                      out.get(), nullptr), "smt_cblsm_choose_arm_length");
    out.download(Armvolume);
}
inline void chooseArmLengthLeft(int *ArmLL, int * /*ArmLR*/, int *ArmRL, int *ArmRR, int dispRange, int *Armvolume, int row, int col)
{ choose_arm_length_(0, ArmLL, nullptr, ArmRL, ArmRR, dispRange, Armvolume, row, col); }
inline void chooseArmLengthRight(int * /*ArmLL*/, int *ArmLR, int *ArmRL, int *ArmRR, int dispRange, int *Armvolume, int row, int col)
{ choose_arm_length_(1, ArmLR, nullptr, ArmRL, ArmRR, dispRange, Armvolume, row, col); }
inline void chooseArmLengthUp(int *ArmLUp, int * /*ArmLDown*/, int *ArmRUp, int * /*ArmRDown*/, int *ArmRL, int *ArmRR, int dispRange,
                              int *Armvolume, int row, int col)
{ choose_arm_length_(2, ArmLUp, ArmRUp, ArmRL, ArmRR, dispRange, Armvolume, row, col); }
inline void chooseArmLengthDown(int * /*ArmLUp*/, int *ArmLDown, int * /*ArmRUp*/, int *ArmRDown, int *ArmRL, int *ArmRR, int dispRange,
                                int *Armvolume, int row, int col)
{ choose_arm_length_(3, ArmLDown, ArmRDown, ArmRL, ArmRR, dispRange, Armvolume, row, col); }

// ------------------------------------------------------------------ cross_aggregator.h:27-113
struct CrossArm { uint8_t left, right, top, bottom; };

class CrossAggregator {
public:
    CrossAggregator() = default;
    ~CrossAggregator() { if (h_) smt_crossagg_destroy(h_); }
    CrossAggregator(const CrossAggregator &) = delete;                    // one owner per handle
    CrossAggregator &operator=(const CrossAggregator &) = delete;
    bool Initialize(const int &width, const int &height, const int &min_disparity, const int &max_disparity)
    {
        w_ = width; hgt_ = height; D_ = max_disparity - min_disparity;
        if (h_) { smt_crossagg_destroy(h_); h_ = nullptr; }
        const int rc = smt_crossagg_create(width, height, D_, &h_);
        if (rc == SMT_ERR_ARG) return false;            // reference returns false, :28-31
        check(rc, "smt_crossagg_create");
        // :34-35 clear + resize: zeroed arms; :52 resize: the cost buffer exists from here on (get_cost_ptr is non-null)
        const size_t n = (size_t)w_ * hgt_;
        host_arms_.assign(n, CrossArm{0, 0, 0, 0});
        host_cost_.resize(n * D_);
        if (have_params_) check(smt_crossagg_set_params(h_, L1_, L2_, t1_, t2_), "smt_crossagg_set_params");
        return true;
    }
    void SetData(const uint8_t *img_left, const uint8_t * /*img_right*/, const float *cost_init)
    {
        img_ = img_left; cost_ = cost_init;
    }
    // The reference stores the four values in members that Initialize leaves alone (:67-74), so SetParams may come
    // before Initialize and holds across a second one.  Never called: the library's defaults (adcensus_types.h:69-70),
    // where the reference would run with the constructor's zeros.
    void SetParams(const int &L1, const int &L2, const int &t1, const int &t2)
    {
        if (h_) check(smt_crossagg_set_params(h_, L1, L2, t1, t2), "smt_crossagg_set_params");
        L1_ = L1; L2_ = L2; t1_ = t1; t2_ = t2; have_params_ = true;
    }
    void Aggregate(const int &num_iters)
    {
        if (!h_) return;                                 // :91-93
        if (!img_ || !cost_) check(SMT_ERR_ARG, "CrossAggregator::Aggregate before SetData");   // the reference reads through null
        const size_t n = (size_t)w_ * hgt_;
        DevBuf<uint8_t> img(n * 3);
        DevBuf<float> c(n * D_);
        img.upload(img_); c.upload(cost_);
        check(smt_crossagg_aggregate(h_, img.get(), c.get(), num_iters), "smt_crossagg_aggregate");
        host_cost_.resize(n * D_);
        host_arms_.resize(n);
        float *dc; uint8_t *da;
        check(smt_crossagg_cost(h_, &dc), "cost"); check(smt_crossagg_arms(h_, &da), "arms");
        check(smt_memcpy_d2h(host_cost_.data(), dc, n * D_ * 4, nullptr), "d2h");
        check(smt_memcpy_d2h(host_arms_.data(), da, n * 4, nullptr), "d2h");
        check(smt_stream_sync(nullptr), "sync");
    }
    CrossArm *get_arms_ptr() { return host_arms_.data(); }
    float *get_cost_ptr() { return host_cost_.empty() ? nullptr : host_cost_.data(); }
private:
    smt_crossagg *h_ = nullptr;
    int w_ = 0, hgt_ = 0, D_ = 0;
    int L1_ = 0, L2_ = 0, t1_ = 0, t2_ = 0;
    bool have_params_ = false;
    const uint8_t *img_ = nullptr;
    const float *cost_ = nullptr;
    std::vector<float> host_cost_;
    std::vector<CrossArm> host_arms_;
};

// ------------------------------------------------------------------ window matchers (host buffers)
// Images are the caller's replicate-padded uint8 buffers, exactly what the reference's drivers pass
// after copyMakeBorder (SADmain.cpp:47-48, ASWeight.cpp:54-57); rows/cols are the PADDED sizes like
// Mat::rows/cols in the reference signatures.

// GetPointDepthLeft / GetPointDepthRight (Sad.h:96-182): disparity is int32 [rows-2w][cols-2w], w = winsize+1
inline void GetPointDepth(int *disparity, const unsigned char *leftimg, const unsigned char *rightimg, int rows,
                          int cols, int MaxDisparity, int winsize, bool left_view)
{
    int H, W;
    inner_size_(rows, cols, winsize + 1, H, W);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols);
    DevBuf<int> d((size_t)H * W);
    L.upload(leftimg); R.upload(rightimg);
    check(smt_sad(L.get(), R.get(), H, W, MaxDisparity, winsize, left_view ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, d.get(),
                  nullptr), "smt_sad");
    d.download(disparity);
}
inline void GetPointDepthLeft(int *disparity, const unsigned char *l, const unsigned char *r, int rows, int cols,
                              int MaxDisparity, int winsize) { GetPointDepth(disparity, l, r, rows, cols, MaxDisparity, winsize, true); }
inline void GetPointDepthRight(int *disparity, const unsigned char *l, const unsigned char *r, int rows, int cols,
                               int MaxDisparity, int winsize) { GetPointDepth(disparity, l, r, rows, cols, MaxDisparity, winsize, false); }

// SADmain.cpp:66-67 in one call: both maps from one evaluation of the hypotheses (smt_sad_both); padded host images
inline void GetPointDepthBoth(int *dispLeft, int *dispRight, const unsigned char *leftimg, const unsigned char *rightimg,
                              int rows, int cols, int MaxDisparity, int winsize)
{
    int H, W;
    inner_size_(rows, cols, winsize + 1, H, W);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols);
    DevBuf<int> dl((size_t)H * W), dr((size_t)H * W);
    L.upload(leftimg); R.upload(rightimg);
    check(smt_sad_both(L.get(), R.get(), H, W, MaxDisparity, winsize, dl.get(), dr.get(), nullptr, nullptr), "smt_sad_both");
    dl.download(dispLeft); dr.download(dispRight);
}

// SADmain.cpp:47-48, :66-68 for batches of UNPADDED gray pairs (smt_sad_flow_*): host buffers in and out
class SadFlow {
public:
    SadFlow(int rows, int cols, int MaxDisparity, int winsize = 3, int device = 0) : n_((size_t)rows * cols)
    {
        smt_sad_params p;
        smt_sad_default_params(&p);
        p.winsize = winsize;
        check(smt_sad_flow_create_on(device, rows, cols, MaxDisparity, &p, &h_), "smt_sad_flow_create_on");
    }
    ~SadFlow() { if (h_) smt_sad_flow_destroy(h_); }
    SadFlow(const SadFlow &) = delete;
    SadFlow &operator=(const SadFlow &) = delete;
    // grayL, grayR: uchar [pairs][rows][cols]; depthleft, depthright, lastdisp: int [pairs][rows][cols] (any may be null)
    void run(const unsigned char *grayL, const unsigned char *grayR, int pairs, int *depthleft, int *depthright, int *lastdisp)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n), cls(n);
        DevBuf<int> dl(n), dr(n), last(n);
        L.upload(grayL); R.upload(grayR);
        check(smt_sad_flow_run_batch(h_, L.get(), R.get(), pairs, dl.get(), dr.get(), last.get(), cls.get()), "smt_sad_flow_run_batch");
        if (depthleft) dl.download(depthleft);
        if (depthright) dr.download(depthright);
        if (lastdisp) last.download(lastdisp);
    }
private:
    smt_sad_flow *h_ = nullptr;
    size_t n_;
};

// NCC_algorithem(leftImage, rigthImage, width, height, disp, winSize, dispRange) (NCC.h:69-95)
inline void NCC_algorithem(const unsigned char *leftImage, const unsigned char *rigthImage, int width, int height,
                           int *disp, int winSize, int dispRange)
{
    const size_t n = (size_t)width * height;
    DevBuf<unsigned char> L(n), R(n);
    DevBuf<int> d(n);
    L.upload(leftImage); R.upload(rigthImage);
    check(smt_ncc(L.get(), R.get(), height, width, dispRange, winSize, d.get(), nullptr, nullptr), "smt_ncc");
    d.download(disp);
}

// NCC_main.cpp:33 for batches of gray pairs (smt_ncc_flow_*): host buffers in and out
class NCCFlow {
public:
    NCCFlow(int rows, int cols, int dispRange, int winSize = 10, int device = 0) : n_((size_t)rows * cols)
    {
        smt_ncc_params p;
        smt_ncc_default_params(&p);
        p.winSize = winSize;
        check(smt_ncc_flow_create_on(device, rows, cols, dispRange, &p, &h_), "smt_ncc_flow_create_on");
    }
    ~NCCFlow() { if (h_) smt_ncc_flow_destroy(h_); }
    NCCFlow(const NCCFlow &) = delete;
    NCCFlow &operator=(const NCCFlow &) = delete;
    // 0 = the dispatch rule, else SMT_NCC_FORM_*
    void set_form(int form) { check(smt_ncc_flow_set_form(h_, form), "smt_ncc_flow_set_form"); }
    // leftImages, rigthImages: uchar [pairs][rows][cols]; disp: int [pairs][rows][cols]
    void run(const unsigned char *leftImages, const unsigned char *rigthImages, int pairs, int *disp)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n);
        DevBuf<int> d(n);
        L.upload(leftImages); R.upload(rigthImages);
        check(smt_ncc_flow_run_batch(h_, L.get(), R.get(), pairs, d.get(), nullptr), "smt_ncc_flow_run_batch");
        d.download(disp);
    }
    // both views and the int-map cross-check (smt_lrncc_flow_run_batch): dispLeft, dispRight, lastdisp int
    // [pairs][rows][cols], cls uchar [pairs][rows][cols] (0 kept / 1 occlusion / 2 mismatch); any may be null
    void runBoth(const unsigned char *leftImages, const unsigned char *rigthImages, int pairs, int *dispLeft, int *dispRight,
                 int *lastdisp, unsigned char *cls)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n), c(n);
        DevBuf<int> dl(n), dr(n), last(n);
        L.upload(leftImages); R.upload(rigthImages);
        check(smt_lrncc_flow_run_batch(h_, L.get(), R.get(), pairs, dl.get(), dr.get(), last.get(), c.get()), "smt_lrncc_flow_run_batch");
        if (dispLeft) dl.download(dispLeft);
        if (dispRight) dr.download(dispRight);
        if (lastdisp) last.download(lastdisp);
        if (cls) c.download(cls);
    }
private:
    smt_ncc_flow *h_ = nullptr;
    size_t n_;
};

// ncc(in1, in2, type, add_constant) (NCC.h:117-272): gray uchar [rows][cols] -> depth uchar [rows][cols] = (uchar)(3 * offset)
// of the winner; type "left" or "right".  kernel_size and max_offset are the values the reference fixes at 5 and 79.
// in2 stays as it is under add_constant (the reference adds 10 to the caller's image).
inline void ncc(const unsigned char *in1, const unsigned char *in2, int rows, int cols, const std::string &type,
                unsigned char *depth, bool add_constant = false, int kernel_size = 5, int max_offset = 79, int *offset = nullptr)
{
    if (type != "left" && type != "right") throw std::runtime_error("ncc: type must be \"left\" or \"right\"");
    const size_t n = (size_t)rows * cols;
    DevBuf<unsigned char> L(n), R(n), d(n);
    DevBuf<int> o(n);
    L.upload(in1); R.upload(in2);
    smt_whole_ncc_params p = {kernel_size, max_offset, add_constant ? 1 : 0};
    check(smt_whole_ncc(L.get(), R.get(), rows, cols, &p, type == "left" ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, d.get(), o.get(), nullptr,
                        nullptr), "smt_whole_ncc");
    d.download(depth);
    if (offset) o.download(offset);
}

// bgr_to_grey (NCC.h:97-115): B, G, R uchar [rows][cols][3] -> uchar [rows][cols], each channel uchar(0.333 v), then added
inline void bgr_to_grey(const unsigned char *bgr, int rows, int cols, unsigned char *grey)
{
    const size_t n = (size_t)rows * cols;
    DevBuf<unsigned char> b(3 * n), g(n);
    b.upload(bgr);
    check(smt_bgr_to_grey_batch(b.get(), 1, rows, cols, g.get(), nullptr), "smt_bgr_to_grey_batch");
    g.download(grey);
}

// NCC_main.cpp with :24 enabled, both types, for batches of gray pairs (smt_whole_ncc_flow_*): host buffers in and out
class NCCWholeFlow {
public:
    NCCWholeFlow(int rows, int cols, int kernel_size = 5, int max_offset = 79, bool add_constant = false, int device = 0)
        : n_((size_t)rows * cols)
    {
        smt_whole_ncc_params p = {kernel_size, max_offset, add_constant ? 1 : 0};
        check(smt_whole_ncc_flow_create_on(device, rows, cols, &p, &h_), "smt_whole_ncc_flow_create_on");
    }
    ~NCCWholeFlow() { if (h_) smt_whole_ncc_flow_destroy(h_); }
    NCCWholeFlow(const NCCWholeFlow &) = delete;
    NCCWholeFlow &operator=(const NCCWholeFlow &) = delete;
    // 0 = as ncc() chooses, else SMT_NCC_WHOLE_FORM_*
    void set_form(int form) { check(smt_whole_ncc_flow_set_form(h_, form), "smt_whole_ncc_flow_set_form"); }
    // in1, in2: uchar [pairs][rows][cols]; depthLeft, depthRight uchar, offLeft, offRight, lastdisp int [pairs][rows][cols]
    // (lastdisp: the cross-check of Sad.h:184-222 on the two offset maps); any output may be null
    void run(const unsigned char *in1, const unsigned char *in2, int pairs, unsigned char *depthLeft, unsigned char *depthRight,
             int *offLeft, int *offRight, int *lastdisp)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n), dl(n), dr(n), c(n);
        DevBuf<int> ol(n), orr(n), last(n);
        L.upload(in1); R.upload(in2);
        check(smt_whole_ncc_flow_run_batch(h_, L.get(), R.get(), pairs, dl.get(), dr.get(), ol.get(), orr.get(), last.get(), c.get()),
              "smt_whole_ncc_flow_run_batch");
        if (depthLeft) dl.download(depthLeft);
        if (depthRight) dr.download(depthRight);
        if (offLeft) ol.download(offLeft);
        if (offRight) orr.download(offRight);
        if (lastdisp) last.download(lastdisp);
    }
private:
    smt_whole_ncc_flow *h_ = nullptr;
    size_t n_;
};

// getGausssianMask + getColorMask (ASW.h:16-47)
inline void getMasks(std::vector<double> &spaceMask, std::vector<double> &colorMask, int winSize, double spaceSigma,
                     double colorSigma)
{
    const int side = 2 * winSize + 3;
    spaceMask.assign((size_t)side * side, 0.0);
    colorMask.assign(256, 0.0);
    check(smt_asw_masks(winSize, spaceSigma, colorSigma, spaceMask.data(), colorMask.data()), "smt_asw_masks");
}

// the masks smt_asw reads are (2 winSize + 3)^2 and 256 doubles whatever the vectors hold: shorter ones must not be uploaded
inline void check_masks_(const std::vector<double> &space, const std::vector<double> &color, int winSize)
{
    const size_t side = 2 * (size_t)(winSize < 0 ? 0 : winSize) + 3;
    if (winSize < 0 || space.size() != side * side || color.size() != 256) check(SMT_ERR_ARG, "ASW masks: getMasks(winSize) sizes expected");
}
// AdaptiveSupportWeight / AdaptiveSupportWeightRight (ASW.h:329-431); disp float [rows-2w][cols-2w], w = winSize+1
inline void AdaptiveSupportWeight(float *disp, const unsigned char *leftGray, const unsigned char *rightGray, int rows,
                                  int cols, int winSize, int dispRange, const std::vector<double> &space,
                                  const std::vector<double> &color, int T, bool left_view = true)
{
    int H, W;
    inner_size_(rows, cols, winSize + 1, H, W);
    check_masks_(space, color, winSize);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols);
    DevBuf<double> sp(space.size()), cm(color.size());
    DevBuf<float> d((size_t)H * W);
    L.upload(leftGray); R.upload(rightGray); sp.upload(space.data()); cm.upload(color.data());
    check(smt_asw(L.get(), R.get(), H, W, dispRange, winSize, sp.get(), cm.get(), T,
                  left_view ? SMT_VIEW_LEFT : SMT_VIEW_RIGHT, d.get(), nullptr, nullptr), "smt_asw");
    d.download(disp);
}

// ASWeight.cpp:60-66 in one call: AdaptiveSupportWeight, AdaptiveSupportWeightRight (both maps from one evaluation of the
// hypotheses, smt_asw_both) and CrossCheckDiaparity (ASW.h:108-145) into lastDisp, uchar [rows-2w][cols-2w] (may be null)
inline void AdaptiveSupportWeightBoth(float *dispL, float *dispR, unsigned char *lastDisp, const unsigned char *leftGray,
                                      const unsigned char *rightGray, int rows, int cols, int winSize, int dispRange,
                                      const std::vector<double> &space, const std::vector<double> &color, int T)
{
    int H, W;
    inner_size_(rows, cols, winSize + 1, H, W);
    check_masks_(space, color, winSize);
    DevBuf<unsigned char> L((size_t)rows * cols), R((size_t)rows * cols), last((size_t)H * W);
    DevBuf<double> sp(space.size()), cm(color.size());
    DevBuf<float> dl((size_t)H * W), dr((size_t)H * W);
    L.upload(leftGray); R.upload(rightGray); sp.upload(space.data()); cm.upload(color.data());
    check(smt_asw_both(L.get(), R.get(), H, W, dispRange, winSize, sp.get(), cm.get(), T, dl.get(), dr.get(), nullptr,
                       nullptr, nullptr), "smt_asw_both");
    dl.download(dispL); dr.download(dispR);
    if (lastDisp) {
        check(smt_asw_crosscheck(dl.get(), dr.get(), H, W, last.get(), nullptr), "smt_asw_crosscheck");
        last.download(lastDisp);
    }
}

// MedianFilter / RemoveSpeckles (PostProcessing.h:250-344) on host maps
// MedianFilter(d, d, ...) as CBLSM.cpp:162 calls it: the raster-order recurrence of the aliased call
inline void MedianFilterInPlace(float *disp, const int &width, const int &height, const int wnd_size)
{
    const size_t n = (size_t)width * height;
    DevBuf<float> a(n);
    a.upload(disp);
    check(smt_median_filter_inplace(a.get(), width, height, wnd_size, nullptr), "smt_median_filter_inplace");
    a.download(disp);
}
inline void MedianFilter(const float *in, float *out, const int &width, const int &height, const int wnd_size)
{
    if (in == out) { MedianFilterInPlace(out, width, height, wnd_size); return; }
    const size_t n = (size_t)width * height;
    DevBuf<float> a(n), b(n);
    a.upload(in);
    check(smt_median_filter(a.get(), b.get(), width, height, wnd_size, nullptr), "smt_median_filter");
    b.download(out);
}
inline void RemoveSpeckles(float *disparity_map, const int &width, const int &height, const int &diff_insame,
                           const unsigned int &min_speckle_aera, const int &invalid_val)
{
    const size_t n = (size_t)width * height;
    DevBuf<float> a(n);
    a.upload(disparity_map);
    check(smt_remove_speckles(a.get(), width, height, diff_insame, min_speckle_aera, invalid_val, nullptr),
          "smt_remove_speckles");
    a.download(disparity_map);
}

// FillImageNew(disp) (ASW/ASW.h:434-511) on a host map uchar [rows][cols], in place, with the reference's defects
// (include/smt.h: smt_fill_image_new_batch); fix = SMT_ASW_FIX_FILL_ROW_END makes column `cols` count as outside.
// counts (may be null): int[2], the holes that pushed nothing and the holes left 0 for want of a list entry.
inline void FillImageNew(unsigned char *disp, int rows, int cols, unsigned fix = 0, int *counts = nullptr)
{
    const size_t n = (size_t)rows * cols;
    DevBuf<unsigned char> a(n);
    DevBuf<int> c(2);
    a.upload(disp);
    check(smt_fill_image_new_batch(a.get(), 1, 0, rows, cols, fix, c.get(), nullptr), "smt_fill_image_new_batch");
    a.download(disp);
    if (counts) c.download(counts);
}
// ASWeight.cpp:69 + :72-78 on the host map CrossCheckDiaparity wrote (uchar [rows][cols]), in place: normalize,
// filterSpeckles, medianBlur 5, FillImageNew, medianBlur 3 (smt_asw_tail_batch).  afterMedian / afterFill (may be null):
// the states the driver writes as speckle.png and filled.png.  post == nullptr: the driver's arguments.
inline void ASWTail(unsigned char *lastDisp, int rows, int cols, unsigned char *afterMedian = nullptr,
                    unsigned char *afterFill = nullptr, const smt_asw_post_params *post = nullptr, int *fillCounts = nullptr)
{
    const size_t n = (size_t)rows * cols;
    DevBuf<unsigned char> a(n), am(n), af(n);
    DevBuf<int> c(2), err(1);
    const int zero = 0;
    a.upload(lastDisp); err.upload(&zero);
    check(smt_asw_tail_batch(a.get(), 1, 0, rows, cols, post, am.get(), af.get(), c.get(), err.get(), nullptr),
          "smt_asw_tail_batch");
    a.download(lastDisp);
    if (afterMedian) am.download(afterMedian);
    if (afterFill) af.download(afterFill);
    if (fillCounts) c.download(fillCounts);
    int e = 0;
    err.download(&e);
    if (e) throw std::runtime_error("smt_asw_tail_batch: a speckle kernel hit its loop cap");
}

// ------------------------------------------------------------------ drivers' image handling
// imread(path) (AD-CensusV1/main.cpp:16-17): 3-channel B, G, R;  cvtColor(.., CV_BGR2GRAY) (:19-20);
// imwrite(path, img) (:115-117).  Host-side decoding / encoding is libsmt_hip.so's own (PNG, PGM, PPM).
struct Image {
    int rows = 0, cols = 0, channels = 0;
    std::vector<unsigned char> data;
};
// an Image whose vector does not hold rows * cols * channels bytes must not be uploaded as if it did
inline void check_image_(const Image &im, const char *what)
{
    if (im.rows <= 0 || im.cols <= 0 || im.channels <= 0 || im.data.size() != (size_t)im.rows * im.cols * im.channels)
        check(SMT_ERR_ARG, what);
}
inline Image imread(const std::string &path, int want_channels = 3)
{
    Image im;
    uint8_t *p = nullptr;
    check(smt_image_read(path.c_str(), want_channels, &p, &im.rows, &im.cols, &im.channels), "smt_image_read");
    im.data.assign(p, p + (size_t)im.rows * im.cols * im.channels);
    smt_image_free(p);
    return im;
}
inline void imwrite(const std::string &path, const unsigned char *data, int rows, int cols, int channels)
{
    check(smt_image_write(path.c_str(), data, rows, cols, channels), "smt_image_write");
}
inline Image cvtColorBGR2GRAY(const Image &bgr)
{
    if (bgr.channels != 3) throw std::runtime_error("cvtColorBGR2GRAY: 3-channel image expected");
    check_image_(bgr, "cvtColorBGR2GRAY");
    const size_t n = (size_t)bgr.rows * bgr.cols;
    DevBuf<unsigned char> in(n * 3), out(n);
    in.upload(bgr.data.data());
    check(smt_bgr2gray(in.get(), bgr.rows, bgr.cols, out.get(), nullptr), "smt_bgr2gray");
    Image g;
    g.rows = bgr.rows; g.cols = bgr.cols; g.channels = 1; g.data.resize(n);
    out.download(g.data.data());
    return g;
}

// ------------------------------------------------------------------ CBLSM.h active path (CBLSM.cpp:64-67, 101-104, 133-153)
// ArmLength{L,R,Up,Down}(const Mat&, uchar tao, int* arm, int maxLength, int secLength) (CBLSM.h:643, 536, 753, 861):
// `tao` is BY VALUE -- every call starts from it again, the drop to 6 past secLength is local to the call.
inline void arm_length_(const Image &image, unsigned char tao, int *arm, int maxLength, int secLength, int dir)
{
    check_image_(image, "ArmLength");
    smt_crossarm_params p;
    smt_crossarm_cblsm_params(&p);
    p.tau = tao; p.max_length = maxLength; p.sec_length = secLength;
    smt_crossarm *h = nullptr;
    check(smt_crossarm_create(image.rows, image.cols, 1, &p, &h), "smt_crossarm_create");
    try {
        DevBuf<unsigned char> img(image.data.size());
        img.upload(image.data.data());
        check(smt_crossarm_reset(h), "smt_crossarm_reset");
        check(smt_crossarm_arm_dir(h, img.get(), image.channels, dir), "smt_crossarm_arm_dir");
        int *maps[4] = {nullptr, nullptr, nullptr, nullptr};
        check(smt_crossarm_arm_maps(h, &maps[0], &maps[1], &maps[2], &maps[3]), "smt_crossarm_arm_maps");
        check(smt_memcpy_d2h(arm, maps[dir], (size_t)image.rows * image.cols * sizeof(int), nullptr), "d2h");
        check(smt_stream_sync(nullptr), "sync");
    } catch (...) { smt_crossarm_destroy(h); throw; }
    smt_crossarm_destroy(h);
}
inline void ArmLengthL(const Image &image, unsigned char tao, int *LArm, int maxLength, int secLength) { arm_length_(image, tao, LArm, maxLength, secLength, 0); }
inline void ArmLengthR(const Image &image, unsigned char tao, int *RArm, int maxLength, int secLength) { arm_length_(image, tao, RArm, maxLength, secLength, 1); }
inline void ArmLengthUp(const Image &image, unsigned char tao, int *UpArm, int maxLength, int secLength) { arm_length_(image, tao, UpArm, maxLength, secLength, 2); }
inline void ArmLengthDown(const Image &image, unsigned char tao, int *DownArm, int maxLength, int secLength) { arm_length_(image, tao, DownArm, maxLength, secLength, 3); }

// ComputeAD / ComputeADRight (CBLSM.h:327-381): uchar absolute differences into a float [row][col][dispRange] volume
inline void compute_ad_(int col, int row, int dispRange, const unsigned char *leftImage, const unsigned char *rightImage,
                        float *ADcostVolum, int view)
{
    const size_t n = (size_t)row * col;
    DevBuf<unsigned char> L(n), R(n);
    DevBuf<float> vol(n * dispRange);
    L.upload(leftImage); R.upload(rightImage);
    check(smt_cblsm_ad(L.get(), R.get(), row, col, dispRange, view, vol.get(), nullptr), "smt_cblsm_ad");
    vol.download(ADcostVolum);
}
inline void ComputeAD(int col, int row, int dispRange, unsigned char *leftImage, unsigned char *rightImage, float *ADcostVolum)
{ compute_ad_(col, row, dispRange, leftImage, rightImage, ADcostVolum, SMT_VIEW_LEFT); }
inline void ComputeADRight(int col, int row, int dispRange, unsigned char *leftImage, unsigned char *rightImage, float *ADcostVolum)
{ compute_ad_(col, row, dispRange, leftImage, rightImage, ADcostVolum, SMT_VIEW_RIGHT); }

// ComputeDispLeft / ComputeDispRight / ComputeDispV4 (CBLSM.h:451-489, :409-447, :494-532), the reference's argument
// order: the images are the PADDED ones (copyMakeBorder by winsize + 1, CBLSM.cpp:124-125; three channels for V4), _row_
// and _col_ the unpadded sizes, dispVolume float [_row_][_col_][dispRange].  Throws where ComputeDispRight reads before
// its buffer (_col_ <= winsize + 1).
inline void compute_disp_(float *dispVolume, const Image &leftimg, const Image &rightimg, int winsize, int dispRange, int _row_,
                          int _col_, int form)
{
    const int w = winsize + 1, ch = form == SMT_CBLSM_COST_V4 ? 3 : 1;
    if (leftimg.rows != _row_ + 2 * w || leftimg.cols != _col_ + 2 * w || leftimg.channels != ch ||
        rightimg.rows != leftimg.rows || rightimg.cols != leftimg.cols || rightimg.channels != ch)
        check(SMT_ERR_ARG, "ComputeDisp: images must be padded by winsize + 1");
    check_image_(leftimg, "ComputeDisp");
    check_image_(rightimg, "ComputeDisp");
    if (form == SMT_CBLSM_COST_RIGHT && _col_ <= w) check(SMT_ERR_REF_UB, "ComputeDispRight");     // before any device work
    DevBuf<unsigned char> L(leftimg.data.size()), R(rightimg.data.size());
    DevBuf<float> vol((size_t)_row_ * _col_ * dispRange);
    L.upload(leftimg.data.data()); R.upload(rightimg.data.data());
    check(smt_cblsm_window_cost_batch(L.get(), R.get(), 1, 0, _row_, _col_, dispRange, winsize, form, vol.get(), 0, nullptr),
          "smt_cblsm_window_cost_batch");
    vol.download(dispVolume);
}
inline void ComputeDispLeft(float *dispVolume, const Image &leftimg, const Image &rightimg, int winsize, int dispRange, int _row_, int _col_)
{ compute_disp_(dispVolume, leftimg, rightimg, winsize, dispRange, _row_, _col_, SMT_CBLSM_COST_LEFT); }
inline void ComputeDispRight(float *dispVolume, const Image &leftimg, const Image &rightimg, int winsize, int dispRange, int _row_, int _col_)
{ compute_disp_(dispVolume, leftimg, rightimg, winsize, dispRange, _row_, _col_, SMT_CBLSM_COST_RIGHT); }
inline void ComputeDispV4(float *dispVolume, const Image &leftimg, const Image &rightimg, int winsize, int dispRange, int _row_, int _col_)
{ compute_disp_(dispVolume, leftimg, rightimg, winsize, dispRange, _row_, _col_, SMT_CBLSM_COST_V4); }

// CBLSM.cpp's flow for batches of gray pairs (smt_cblsm_flow_*): host buffers in and out
class CBLSMFlow {
public:
    CBLSMFlow(int rows, int cols, int dispRange, int device = 0) : n_((size_t)rows * cols)
    {
        check(smt_cblsm_flow_create_on(device, rows, cols, dispRange, nullptr, &h_), "smt_cblsm_flow_create_on");
    }
    ~CBLSMFlow() { if (h_) smt_cblsm_flow_destroy(h_); }
    CBLSMFlow(const CBLSMFlow &) = delete;
    CBLSMFlow &operator=(const CBLSMFlow &) = delete;
    // grayL, grayR: uchar [pairs][rows][cols]; dispLeft, dispRight: float [pairs][rows][cols].  CBLSM.cpp as it is run:
    // the first passes aggregate ComputeAD / ComputeADRight
    void run(const unsigned char *grayL, const unsigned char *grayR, int pairs, float *dispLeft, float *dispRight)
    { run_(grayL, grayR, pairs, -1, dispLeft, dispRight); }
    // the same with :132 enabled: the first passes aggregate ComputeDispLeft / ComputeDispRight of the padded images
    void runWindow(const unsigned char *grayL, const unsigned char *grayR, int pairs, int winSize, float *dispLeft, float *dispRight)
    { run_(grayL, grayR, pairs, winSize, dispLeft, dispRight); }
private:
    void run_(const unsigned char *grayL, const unsigned char *grayR, int pairs, int winSize, float *dispLeft, float *dispRight)
    {
        const size_t n = batch_elems_(n_, pairs);
        DevBuf<unsigned char> L(n), R(n);
        DevBuf<float> dl(n), dr(n);
        L.upload(grayL); R.upload(grayR);
        if (winSize < 0) check(smt_cblsm_flow_run_batch(h_, L.get(), R.get(), pairs, dl.get(), dr.get()), "smt_cblsm_flow_run_batch");
        else check(smt_cblsm_flow_run_batch_window(h_, L.get(), R.get(), pairs, winSize, dl.get(), dr.get()), "smt_cblsm_flow_run_batch_window");
        check(smt_cblsm_flow_status(h_), "smt_cblsm_flow_status");
        if (dispLeft) dl.download(dispLeft);
        if (dispRight) dr.download(dispRight);
    }
    smt_cblsm_flow *h_ = nullptr;
    size_t n_;
};

// costAggregationV5 (CBLSM.h:1179-1224): rectangle mean, rows outer / columns inner, with the four arm arrays the
// caller passes -- whichever image they were computed on (CBLSM.cpp:150 aggregates the right volume with the left
// image's arms).  winSize is unused by the reference too.
inline void costAggregationV5(float *dispvolume, float *CostVolume, int *ArmvolumeL, int *ArmvolumeR, int *ArmvolumeUp,
                              int *ArmvolumeDown, int dispRange, int row, int col, int /*winSize*/)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> in(n * dispRange), out(n * dispRange);
    DevBuf<int> aL(n), aR(n), aU(n), aD(n);
    in.upload(dispvolume);
    aL.upload(ArmvolumeL); aR.upload(ArmvolumeR); aU.upload(ArmvolumeUp); aD.upload(ArmvolumeDown);
    smt_crossarm_params p;
    smt_crossarm_cblsm_params(&p);
    smt_crossarm *h = nullptr;
    check(smt_crossarm_create(row, col, dispRange, &p, &h), "smt_crossarm_create");
    try {
        check(smt_crossarm_load_arm_maps(h, aL.get(), aR.get(), aU.get(), aD.get()), "smt_crossarm_load_arm_maps");
        check(smt_crossarm_aggregate(h, in.get(), out.get(), 1, nullptr), "smt_crossarm_aggregate");
        out.download(CostVolume);
        check(smt_crossarm_status(h), "smt_crossarm_status");
    } catch (...) { smt_crossarm_destroy(h); throw; }
    smt_crossarm_destroy(h);
}

// costAggregationV4 (CBLSM.h:1128-1176): the mean over the half-open rectangle rows [-up, down) x columns [-L, R) that
// the four [row][col][dispRange] arm volumes of chooseArmLength* give for each (pixel, d); an empty rectangle is NaN.
// Throws where a tap lies outside the plane (the reference reads out of bounds there).  winSize is unused by the
// reference too.
inline void costAggregationV4(float *dispvolume, float *CostVolume, int *ArmvolumeL, int *ArmvolumeR, int *ArmvolumeUp,
                              int *ArmvolumeDown, int dispRange, int row, int col, int /*winSize*/)
{
    const size_t n = (size_t)row * col * dispRange;
    DevBuf<float> in(n), out(n);
    DevBuf<int> aL(n), aR(n), aU(n), aD(n), ub(1);
    const int zero = 0;
    int flag = 0;
    in.upload(dispvolume);
    aL.upload(ArmvolumeL); aR.upload(ArmvolumeR); aU.upload(ArmvolumeUp); aD.upload(ArmvolumeDown); ub.upload(&zero);
    check(smt_cblsm_cost_aggregation_v4(in.get(), aL.get(), aR.get(), aU.get(), aD.get(), row, col, dispRange, out.get(),
                                        nullptr, ub.get(), nullptr), "smt_cblsm_cost_aggregation_v4");
    out.download(CostVolume);
    ub.download(&flag);
    if (flag) check(SMT_ERR_REF_UB, "costAggregationV4");
}

// ComputeDispOringin (CBLSM.h:383-407): first strict minimum over d
inline void ComputeDispOringin(float *costVolume, float *disp, int dispRange, int row, int col)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> v(n * dispRange), d(n);
    v.upload(costVolume);
    check(smt_wta(v.get(), row, col, dispRange, d.get(), nullptr), "smt_wta");
    d.download(disp);
}

// The winner of every row refined by the parabola through it and its two neighbours (smt_wta_subpixel: the value
// Sad.h:76-81 and CBLSM.h:285-290 compute and drop).  min_den = the reference's literal 1.
inline void WTASubpixel(float *costVolume, float *disp, int dispRange, int row, int col, float min_den = 1.0f)
{
    const size_t n = (size_t)row * col;
    DevBuf<float> v(n * dispRange), d(n);
    v.upload(costVolume);
    const smt_subpixel_params sp{min_den};
    check(smt_wta_subpixel(v.get(), row, col, dispRange, &sp, d.get(), nullptr), "smt_wta_subpixel");
    d.download(disp);
}

// ------------------------------------------------------------------ the batched main.cpp pipeline (smt_pipeline_*)
// Host buffers in and out: grayL / grayR uint8 [pairs][row][col]; dispL (after the LR check), dispR float and cls uint8
// [pairs][row][col], any of the three may be null.  setSubpixel(min_den): both maps refined (smt_pipeline_set_subpixel), 0 = integer maps, the default.
class Pipeline {
public:
    Pipeline(int row, int col, int dispRange, const smt_pipeline_params *p = nullptr) : row_(row), col_(col)
    {
        check(smt_pipeline_create(row, col, dispRange, p, &h_), "smt_pipeline_create");
    }
    ~Pipeline() { if (h_) smt_pipeline_destroy(h_); }
    Pipeline(const Pipeline &) = delete;
    Pipeline &operator=(const Pipeline &) = delete;
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
        if (dispL) dl.download(dispL);                   // any output may be null, as in the sibling flows
        if (dispR) dr.download(dispR);
        if (cls) c.download(cls);
    }
private:
    smt_pipeline *h_ = nullptr;
    int row_, col_;
};

// ------------------------------------------------------------------ config 5: a batch over the node's GPUs
// One host thread, one smt_adcensus handle per device (smt_adcensus_create_on); pair b goes to device
// b % G as a contiguous block per device; no data-path exchange between devices (pairs are independent,
// SURVEY 8e) -- the maps come back to the host buffers directly.  L, R: [pairs][row][col] float (integer
// valued); dispL, dispR: [pairs][row][col] float out.  Returns the number of devices used.
inline int AD_Census_batch_all_devices(const float *L, const float *R, int pairs, int dispRange, int row, int col,
                                       float sigmaC, float sigmaS, float *dispL, float *dispR, int max_devices = 0)
{
    int G = 0;
    check(smt_device_count(&G), "smt_device_count");
    if (max_devices > 0 && G > max_devices) G = max_devices;
    if (G > pairs) G = pairs;
    if (G <= 0) throw std::runtime_error("no device / empty batch");
    const size_t n = (size_t)row * col;
    struct Dev {
        smt_adcensus *h = nullptr; void *stream = nullptr; float *L = nullptr, *R = nullptr, *dl = nullptr, *dr = nullptr; int start = 0, count = 0;
        int id = -1;
        void release()      // idempotent; also what a throw half-way through the loops below runs, on every device reached
        {
            if (id < 0) return;
            smt_set_device(id);
            if (h) smt_adcensus_status(h);              // drains the device's stream before its buffers go
            smt_free(L); smt_free(R); smt_free(dl); smt_free(dr);
            if (h) smt_adcensus_destroy(h);
            if (stream) smt_stream_destroy(stream);
            h = nullptr; stream = nullptr; L = R = dl = dr = nullptr; id = -1;
        }
        ~Dev() { release(); }
    };
    struct Home { ~Home() { smt_set_device(0); } } home;       // destroyed after `dev`: the caller's device 0 again
    std::vector<Dev> dev(G);
    const int q = pairs / G, r = pairs % G;
    for (int g = 0; g < G; g++) {
        Dev &d = dev[g];
        d.count = q + (g < r ? 1 : 0);
        d.start = g * q + (g < r ? g : r);
        check(smt_set_device(g), "smt_set_device");
        d.id = g;
        check(smt_adcensus_create_on(g, row, col, dispRange, sigmaC, sigmaS, &d.h), "smt_adcensus_create_on");
        check(smt_stream_create(&d.stream), "smt_stream_create");
        check(smt_adcensus_set_stream(d.h, d.stream), "smt_adcensus_set_stream");
        const size_t bytes = (size_t)d.count * n * sizeof(float);
        check(smt_malloc((void **)&d.L, bytes), "smt_malloc"); check(smt_malloc((void **)&d.R, bytes), "smt_malloc");
        check(smt_malloc((void **)&d.dl, bytes), "smt_malloc"); check(smt_malloc((void **)&d.dr, bytes), "smt_malloc");
        check(smt_memcpy_h2d(d.L, L + (size_t)d.start * n, bytes, d.stream), "h2d");
        check(smt_memcpy_h2d(d.R, R + (size_t)d.start * n, bytes, d.stream), "h2d");
        // asynchronous on the device's own stream: all devices compute concurrently
        check(smt_adcensus_compute_batch(d.h, d.L, d.R, d.count, SMT_VIEW_BOTH, d.dl, d.dr), "smt_adcensus_compute_batch");
        check(smt_memcpy_d2h(dispL + (size_t)d.start * n, d.dl, bytes, d.stream), "d2h");
        check(smt_memcpy_d2h(dispR + (size_t)d.start * n, d.dr, bytes, d.stream), "d2h");
    }
    for (int g = 0; g < G; g++) {
        Dev &d = dev[g];
        check(smt_set_device(g), "smt_set_device");
        check(smt_adcensus_status(d.h), "smt_adcensus_status");        // synchronises the device's stream
        d.release();
    }
    check(smt_set_device(0), "smt_set_device");
    return G;
}

#ifdef SMT_HOST_WITH_RCCL
}  // namespace smt
#include <rccl/rccl.h>
namespace smt {
// ------------------------------------------------------------------ config 5 with the exchange over RCCL / xGMI
// Same sharding as AD_Census_batch_all_devices, but the disparity maps stay on the devices and are exchanged the
// way SURVEY 8e prescribes: one ncclAllGather of the (padded) per-device [count][row][col] maps -- every device
// ends up with all `pairs` maps -- and one ncclAllReduce(sum) of a float64 checksum.  Single process, one
// communicator per device (ncclCommInitAll), group calls.  Returns the all-reduced checksum; gathered maps are
// copied back from device 0.  Pairs are independent, so this is the only traffic between devices.
inline void rccl_check(ncclResult_t r, const char *what)
{
    if (r != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + ncclGetErrorString(r));
}
inline double AD_Census_batch_rccl(const float *L, const float *R, int pairs, int dispRange, int row, int col, float sigmaC,
                                   float sigmaS, float *dispL, float *dispR, int *devices_used = nullptr, int max_devices = 0)
{
    int G = 0;
    check(smt_device_count(&G), "smt_device_count");
    if (max_devices > 0 && G > max_devices) G = max_devices;
    if (G > pairs) G = pairs;
    if (G <= 0) throw std::runtime_error("no device / empty batch");
    const size_t n = (size_t)row * col;
    const int q = pairs / G, r = pairs % G, cmax = q + (r ? 1 : 0);
    struct Dev {
        smt_adcensus *h = nullptr; void *stream = nullptr;
        float *L = nullptr, *R = nullptr, *send[2] = {nullptr, nullptr}, *recv[2] = {nullptr, nullptr};
        double *sum = nullptr; int start = 0, count = 0;
    };
    std::vector<Dev> dev(G);
    std::vector<int> ids(G);
    for (int g = 0; g < G; g++) ids[g] = g;
    std::vector<ncclComm_t> comm(G);
    rccl_check(ncclCommInitAll(comm.data(), G, ids.data()), "ncclCommInitAll");
    for (int g = 0; g < G; g++) {
        Dev &d = dev[g];
        d.count = q + (g < r ? 1 : 0);
        d.start = g * q + (g < r ? g : r);
        check(smt_set_device(g), "smt_set_device");
        check(smt_adcensus_create_on(g, row, col, dispRange, sigmaC, sigmaS, &d.h), "smt_adcensus_create_on");
        check(smt_stream_create(&d.stream), "smt_stream_create");
        check(smt_adcensus_set_stream(d.h, d.stream), "smt_adcensus_set_stream");
        const size_t bytes = (size_t)d.count * n * sizeof(float), pad = (size_t)cmax * n * sizeof(float);
        check(smt_malloc((void **)&d.L, bytes), "smt_malloc"); check(smt_malloc((void **)&d.R, bytes), "smt_malloc");
        for (int v = 0; v < 2; v++) {
            check(smt_malloc((void **)&d.send[v], pad), "smt_malloc");
            check(smt_malloc((void **)&d.recv[v], pad * G), "smt_malloc");
            check(smt_memset(d.send[v], 0, pad, d.stream), "smt_memset");       // shards are padded to the largest count
        }
        check(smt_malloc((void **)&d.sum, sizeof(double)), "smt_malloc");
        check(smt_memcpy_h2d(d.L, L + (size_t)d.start * n, bytes, d.stream), "h2d");
        check(smt_memcpy_h2d(d.R, R + (size_t)d.start * n, bytes, d.stream), "h2d");
        check(smt_adcensus_compute_batch(d.h, d.L, d.R, d.count, SMT_VIEW_BOTH, d.send[0], d.send[1]), "smt_adcensus_compute_batch");
        check(smt_sum_f32(d.send[0], (size_t)d.count * n, d.sum, d.stream), "smt_sum_f32");
    }
    // the exchange: both views' maps and the checksum, one group
    rccl_check(ncclGroupStart(), "ncclGroupStart");
    for (int g = 0; g < G; g++) {
        Dev &d = dev[g];
        for (int v = 0; v < 2; v++)
            rccl_check(ncclAllGather(d.send[v], d.recv[v], (size_t)cmax * n, ncclFloat, comm[g], (hipStream_t)d.stream), "ncclAllGather");
        rccl_check(ncclAllReduce(d.sum, d.sum, 1, ncclDouble, ncclSum, comm[g], (hipStream_t)d.stream), "ncclAllReduce");
    }
    rccl_check(ncclGroupEnd(), "ncclGroupEnd");
    // device 0 holds everything: trim the padding while copying back
    double checksum = 0.0;
    check(smt_set_device(0), "smt_set_device");
    for (int g = 0; g < G; g++) {
        const size_t bytes = (size_t)dev[g].count * n * sizeof(float);
        check(smt_memcpy_d2h(dispL + (size_t)dev[g].start * n, dev[0].recv[0] + (size_t)g * cmax * n, bytes, dev[0].stream), "d2h");
        check(smt_memcpy_d2h(dispR + (size_t)dev[g].start * n, dev[0].recv[1] + (size_t)g * cmax * n, bytes, dev[0].stream), "d2h");
    }
    check(smt_memcpy_d2h(&checksum, dev[0].sum, sizeof(double), dev[0].stream), "d2h");
    for (int g = 0; g < G; g++) {
        Dev &d = dev[g];
        check(smt_set_device(g), "smt_set_device");
        check(smt_adcensus_status(d.h), "smt_adcensus_status");        // synchronises the device's stream
        smt_free(d.L); smt_free(d.R); smt_free(d.sum);
        for (int v = 0; v < 2; v++) { smt_free(d.send[v]); smt_free(d.recv[v]); }
        smt_adcensus_destroy(d.h);
        smt_stream_destroy(d.stream);
        ncclCommDestroy(comm[g]);
    }
    check(smt_set_device(0), "smt_set_device");
    if (devices_used) *devices_used = G;
    return checksum;
}
#endif  // SMT_HOST_WITH_RCCL

}  // namespace smt
