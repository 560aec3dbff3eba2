// smt_refine.hpp -- C++ host-side mirror of include/smt_refine.h, beside smt_host.hpp and in its manner: HOST pointers in
// and out, everything computed by libsmt_hip.so, errors thrown as std::runtime_error.  Region voting and outlier
// interpolation of the AD-Census method; the reference has no code for them (parity unpinned), so the names are this
// library's.
#pragma once
#include "smt_host.hpp"
#include "../../include/smt_refine.h"

namespace smt {

inline smt_refine_params RefineDefaultParams()
{
    smt_refine_params p;
    smt_refine_default_params(&p);
    return p;
}

// what a call reports besides the map: state uint8 [row][col] (may be null) and the four status words (may be null)
struct RefineOutputs {
    unsigned char *state = nullptr;
    int *status = nullptr;
};

namespace refine_detail {
inline void size_(int row, int col, int dispRange, const char *what)
{
    if (row <= 0 || col <= 0 || dispRange < 1 || dispRange > SMT_MAX_DISPARITY) check(SMT_ERR_ARG, what);
}
struct Outs {
    DevBuf<unsigned char> state;
    DevBuf<int> status;
    Outs(size_t n, const RefineOutputs &o) : state(o.state ? n : 1), status(4) {}     // never an empty allocation
    void download(const RefineOutputs &o) const
    {
        if (o.state) state.download(o.state);                   // n bytes: the buffer was sized for them
        if (o.status) status.download(o.status);
    }
};
}  // namespace refine_detail

// The four arm maps of an image, int [row][col] each, as CrossArmAggregation::Initialize + the four Compute*ArmLength
// calls of main.cpp:67-72 leave them (tao and SMT_QUIRK_* as that class takes them): what RegionVote reads
inline void ArmMaps(const unsigned char *image, int row, int col, int dispRange, int tao, unsigned quirks, int *armL, int *armR,
                    int *armT, int *armB)
{
    refine_detail::size_(row, col, dispRange, "ArmMaps");
    if (!image || !armL || !armR || !armT || !armB) check(SMT_ERR_ARG, "ArmMaps");
    const size_t n = (size_t)row * col;
    DevBuf<unsigned char> img(n);
    img.upload(image);
    smt_crossarm_params p;
    smt_crossarm_default_params(&p);
    p.tau = tao;
    p.quirks = quirks;
    struct Handle {
        smt_crossarm *h = nullptr;
        ~Handle() { if (h) smt_crossarm_destroy(h); }
    } ca;
    check(smt_crossarm_create(row, col, dispRange, &p, &ca.h), "smt_crossarm_create");
    check(smt_crossarm_arms(ca.h, img.get(), 1), "smt_crossarm_arms");
    int *dev[4] = {nullptr, nullptr, nullptr, nullptr};
    check(smt_crossarm_arm_maps(ca.h, &dev[0], &dev[1], &dev[2], &dev[3]), "smt_crossarm_arm_maps");
    int *host[4] = {armL, armR, armT, armB};
    for (int k = 0; k < 4; k++) check(smt_memcpy_d2h(host[k], dev[k], n * sizeof(int), nullptr), "d2h");
    check(smt_stream_sync(nullptr), "sync");
}

// LeftRightConsistency's two lists as the class map InterpolateOutliers reads: 1 occlusion, 2 mismatch, 0 kept
inline void ClassMap(const std::vector<std::pair<int, int>> &occlusion, const std::vector<std::pair<int, int>> &mismatch, int row,
                     int col, unsigned char *cls)
{
    if (row <= 0 || col <= 0 || !cls) check(SMT_ERR_ARG, "ClassMap");
    for (size_t k = 0; k < (size_t)row * col; k++) cls[k] = 0;
    const std::vector<std::pair<int, int>> *lists[2] = {&occlusion, &mismatch};
    for (int c = 0; c < 2; c++)
        for (const std::pair<int, int> &q : *lists[c]) {
            if (q.first < 0 || q.first >= row || q.second < 0 || q.second >= col) check(SMT_ERR_ARG, "ClassMap: pair outside the image");
            cls[(size_t)q.first * col + q.second] = (unsigned char)(c + 1);
        }
}

// smt_region_vote_batch on one map: disp float [row][col] in place; the four arm maps int [row][col] as
// CrossArmAggregation's leftLength, rightLength, topLength, buttonLenght
inline void RegionVote(float *disp, const int *armL, const int *armR, const int *armT, const int *armB, int row, int col,
                       int dispRange, const smt_refine_params &p = RefineDefaultParams(), RefineOutputs out = RefineOutputs())
{
    refine_detail::size_(row, col, dispRange, "RegionVote");
    if (!disp || !armL || !armR || !armT || !armB) check(SMT_ERR_ARG, "RegionVote");
    const size_t n = (size_t)row * col;
    DevBuf<float> d(n);
    DevBuf<int> a(4 * n);
    d.upload(disp);
    const int *arms[4] = {armL, armR, armT, armB};
    for (int k = 0; k < 4; k++) check(smt_memcpy_h2d(a.get() + k * n, arms[k], n * sizeof(int), nullptr), "h2d");
    refine_detail::Outs o(n, out);
    check(smt_region_vote_batch(d.get(), 1, 0, a.get(), a.get() + n, a.get() + 2 * n, a.get() + 3 * n, 0, row, col, dispRange, &p,
                                out.state ? o.state.get() : nullptr, 0, out.status ? o.status.get() : nullptr, nullptr),
          "smt_region_vote_batch");
    d.download(disp);
    o.download(out);
}

// smt_interpolate_outliers_batch on one map: cls as LeftRightConsistency's class map, gray the left image
inline void InterpolateOutliers(float *disp, const unsigned char *cls, const unsigned char *gray, int row, int col, int dispRange,
                                const smt_refine_params &p = RefineDefaultParams(), RefineOutputs out = RefineOutputs())
{
    refine_detail::size_(row, col, dispRange, "InterpolateOutliers");
    if (!disp || !cls || !gray) check(SMT_ERR_ARG, "InterpolateOutliers");
    const size_t n = (size_t)row * col;
    DevBuf<float> d(n);
    DevBuf<unsigned char> c(n), g(n);
    d.upload(disp); c.upload(cls); g.upload(gray);
    refine_detail::Outs o(n, out);
    check(smt_interpolate_outliers_batch(d.get(), 1, 0, c.get(), 0, g.get(), 0, row, col, dispRange, &p,
                                         out.state ? o.state.get() : nullptr, 0, out.status ? o.status.get() : nullptr, nullptr),
          "smt_interpolate_outliers_batch");
    d.download(disp);
    o.download(out);
}

// smt_refine_batch on one map: the voting, then the interpolation
inline void Refine(float *disp, const int *armL, const int *armR, const int *armT, const int *armB, const unsigned char *cls,
                   const unsigned char *gray, int row, int col, int dispRange, const smt_refine_params &p = RefineDefaultParams(),
                   RefineOutputs out = RefineOutputs())
{
    refine_detail::size_(row, col, dispRange, "Refine");
    if (!disp || !armL || !armR || !armT || !armB || !cls || !gray) check(SMT_ERR_ARG, "Refine");
    const size_t n = (size_t)row * col;
    DevBuf<float> d(n);
    DevBuf<int> a(4 * n);
    DevBuf<unsigned char> c(n), g(n);
    d.upload(disp); c.upload(cls); g.upload(gray);
    const int *arms[4] = {armL, armR, armT, armB};
    for (int k = 0; k < 4; k++) check(smt_memcpy_h2d(a.get() + k * n, arms[k], n * sizeof(int), nullptr), "h2d");
    refine_detail::Outs o(n, out);
    check(smt_refine_batch(d.get(), 1, 0, a.get(), a.get() + n, a.get() + 2 * n, a.get() + 3 * n, 0, c.get(), 0, g.get(), 0, row, col,
                           dispRange, &p, out.state ? o.state.get() : nullptr, 0, out.status ? o.status.get() : nullptr, nullptr),
          "smt_refine_batch");
    d.download(disp);
    o.download(out);
}

}  // namespace smt
