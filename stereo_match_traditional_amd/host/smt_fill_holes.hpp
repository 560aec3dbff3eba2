// smt_fill_holes.hpp -- C++ host-side mirror of include/smt_fill_holes.h, beside smt_host.hpp and in its manner: HOST
// pointers in and out, everything computed by libsmt_hip.so, errors thrown as std::runtime_error.  SAD/Sad.h's
// FillHolesInDispMap (Sad.h:317-400): the filler for the holes LeftRightConsistency marks +inf.
#pragma once
#include "smt_host.hpp"
#include "../../include/smt_fill_holes.h"

#include <limits>

namespace smt {

// the four status words of a call (may be null): {n_occ, n_mis, n_third, flags}
namespace fill_holes_detail {
inline void size_(int row, int col, const char *what)
{
    if (row <= 0 || col <= 0 || row > SMT_FILLHOLES_MAX_DIM || col > SMT_FILLHOLES_MAX_DIM) check(SMT_ERR_ARG, what);
}
}  // namespace fill_holes_detail

// On a class map as LeftRightConsistency writes it (1 occlusion, 2 mismatch): disp float [row][col] in place.  A map that
// holds a NaN is not modified; status[3] then carries SMT_FILLHOLES_UB_NAN.
inline void FillHolesInDispMap(float *disp, const unsigned char *cls, int row, int col,
                               float Invalid_Float = std::numeric_limits<float>::infinity(), int *status = nullptr)
{
    fill_holes_detail::size_(row, col, "FillHolesInDispMap");
    if (!disp || !cls) check(SMT_ERR_ARG, "FillHolesInDispMap");
    const size_t n = (size_t)row * col;
    DevBuf<float> d(n);
    DevBuf<unsigned char> c(n);
    DevBuf<int> st(4);
    d.upload(disp);
    c.upload(cls);
    check(smt_fill_holes_batch(d.get(), c.get(), 1, 0, 0, row, col, Invalid_Float, st.get(), nullptr), "smt_fill_holes_batch");
    d.download(disp);
    if (status) st.download(status);
}

// The reference's signature (Sad.h:317: width, height, the map, the two lists by value, the invalid value).  The lists
// must be what LeftRightConsistency and CrossCheckDiaparity produce: (row, col) pairs inside the image, each list in
// strictly increasing raster order, no pixel in both -- the order the device formulation reproduces.  Anything else is
// SMT_ERR_ARG.
inline void FillHolesInDispMap(const int width_, const int height_, float *disp_left_, std::vector<std::pair<int, int>> occlusion,
                               std::vector<std::pair<int, int>> mismatch, const float Invalid_Float, int *status = nullptr)
{
    fill_holes_detail::size_(height_, width_, "FillHolesInDispMap");
    if (!disp_left_) check(SMT_ERR_ARG, "FillHolesInDispMap");
    std::vector<unsigned char> cls((size_t)height_ * width_, 0);
    const std::vector<std::pair<int, int>> *lists[2] = {&occlusion, &mismatch};
    for (int c = 0; c < 2; c++) {
        long long before = -1;
        for (const std::pair<int, int> &q : *lists[c]) {
            if (q.first < 0 || q.first >= height_ || q.second < 0 || q.second >= width_)
                check(SMT_ERR_ARG, "FillHolesInDispMap: pair outside the image");
            const long long at = (long long)q.first * width_ + q.second;
            if (at <= before) check(SMT_ERR_ARG, "FillHolesInDispMap: a list is not in raster order");
            if (cls[(size_t)at]) check(SMT_ERR_ARG, "FillHolesInDispMap: a pixel is in both lists");
            cls[(size_t)at] = (unsigned char)(c + 1);
            before = at;
        }
    }
    FillHolesInDispMap(disp_left_, cls.data(), height_, width_, Invalid_Float, status);
}

}  // namespace smt
