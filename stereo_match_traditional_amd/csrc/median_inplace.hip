// MedianFilter(dispLeft, dispLeft, col, row, 3) (CBLSM/CBLSM.cpp:162; AD-CensusV1/PostProcessing.h:314-344 with
// in == out) on the device, and the tail of CBLSM.cpp it closes (:160-162).  The aliased call is a recurrence in raster
// order; csrc/median_schedule.h has the dependency argument, the step numbering and the arithmetic both kernels and the
// host twin share.  One map has one pixel per row per step, so a map belongs to one workgroup from start to end (one
// thread per row, bands of rows one after the other) and the batch is the parallel axis.
//
// Barrier rules (both kernels loop over workgroup barriers): every thread of a workgroup runs the same number of steps
// and reaches every barrier -- threads without a pixel idle inside the step, nothing returns early; every loop bound
// comes from H, W, r, pairs and the launch geometry alone; nothing waits on another workgroup.
#include "smt_common.h"
#include "median_schedule.h"
#include <climits>
#include <new>
#include <vector>

namespace {

using namespace medsched;

int g_impl = 0;                                        // smt_median_inplace_set_impl: 0 ring, 1 plain

constexpr int MAX_GRID = 1024;                         // maps beyond it stride the grid

// impl 1: per step every live row reads its window from the map, barrier, writes, barrier
__global__ void __launch_bounds__(PLAIN_BAND) k_median_inplace_plain(float *disp, int pairs, size_t stride, int W, int H,
                                                                     int r, int band)
{
    const int li = threadIdx.x, nb = band_count(band, H);
    for (int b = blockIdx.x; b < pairs; b += gridDim.x) {
        float *m = disp + (size_t)b * stride;
        for (int k = 0; k < nb; k++) {
            const int i0 = k * band, rows = band_rows(band, H, k), ns = plain_steps(rows, W, r);
            for (int s = 0; s < ns; s++) {
                const int j = col_at(s, li, r);
                const bool act = li < rows && j >= 0 && j < W;
                float o = 0.0f;
                if (act) o = plain_median(m, W, H, i0 + li, j, r);
                __syncthreads();
                if (act) m[(size_t)(i0 + li) * W + j] = o;
                __syncthreads();
            }
        }
    }
}

// impl 0: rings in LDS, sliding register window, prefetched run; one barrier per step
template <int R>
__global__ void __launch_bounds__(R >= 3 ? 512 : 1024) k_median_inplace_ring(float *disp, int pairs, size_t stride, int W,
                                                                             int H, int band)
{
    constexpr int RING = R <= 1 ? 8 : (R == 2 ? 16 : 32), NTMAX = R >= 3 ? 512 : 1024;
    __shared__ float ring[RING * NTMAX];
    const int nt = blockDim.x, tid = threadIdx.x, nb = band_count(band, H);
    for (int b = blockIdx.x; b < pairs; b += gridDim.x) {
        float *m = disp + (size_t)b * stride;
        for (int k = 0; k < nb; k++) {
            const int i0 = k * band, rows = band_rows(band, H, k);
            const int s0 = first_step(R), ns = ring_steps(rows, W, R);
            __syncthreads();                           // the band above is final and visible; the rings are free
            RingThread<R> T;
            ring_begin<R>(T, m, W, H, tid, i0, rows);
            for (int t = 0; t < ns; t += 4) {
                if (refill_point(t)) ring_refill<R>(T, m, W, s0 + t);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    ring_step<R>(T, m, W, ring, nt, tid, s0 + t + u, u);
                    __syncthreads();
                }
            }
        }
    }
}

int mip_check(const float *disp, int pairs, size_t stride, int W, int H, int wnd_size)
{
    if (!disp || pairs <= 0 || H <= 0 || W <= 0 || wnd_size < 1 || wnd_size > 7) return SMT_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) || (stride != 0 && stride < (size_t)H * W)) return SMT_ERR_ARG;
    return SMT_OK;
}

int mip_launch(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, hipStream_t st)
{
    const int r = radius(wnd_size);
    if (r == 0) return SMT_OK;                         // a 1 x 1 window: the map as it is
    if (stride == 0) stride = (size_t)H * W;
    const int impl = g_impl, cap = band_cap(impl, r), band = H < cap ? H : cap;
    const dim3 grid(pairs < MAX_GRID ? pairs : MAX_GRID);
    if (impl == 1) {
        const int nt = (band + 63) / 64 * 64;
        hipLaunchKernelGGL(k_median_inplace_plain, grid, dim3(nt), 0, st, disp, pairs, stride, W, H, r, band);
    } else {
        const int nt = (band + 2 * r + 63) / 64 * 64;  // <= ring_threads(r)
        if (r == 1) hipLaunchKernelGGL(k_median_inplace_ring<1>, grid, dim3(nt), 0, st, disp, pairs, stride, W, H, band);
        else if (r == 2) hipLaunchKernelGGL(k_median_inplace_ring<2>, grid, dim3(nt), 0, st, disp, pairs, stride, W, H, band);
        else hipLaunchKernelGGL(k_median_inplace_ring<3>, grid, dim3(nt), 0, st, disp, pairs, stride, W, H, band);
    }
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// ---- the host twin: the same schedule on host memory through median_schedule.h --------------------------------------
void host_plain(float *m, int W, int H, int r, int band)
{
    std::vector<float> o((size_t)band);
    for (int k = 0; k < band_count(band, H); k++) {
        const int i0 = k * band, rows = band_rows(band, H, k), ns = plain_steps(rows, W, r);
        for (int s = 0; s < ns; s++) {
            for (int li = 0; li < rows; li++) {                                // all reads of the step ...
                const int j = col_at(s, li, r);
                if (j >= 0 && j < W) o[li] = plain_median(m, W, H, i0 + li, j, r);
            }
            for (int li = 0; li < rows; li++) {                                // ... before its writes
                const int j = col_at(s, li, r);
                if (j >= 0 && j < W) m[(size_t)(i0 + li) * W + j] = o[li];
            }
        }
    }
}

// a thread's reads and writes of one step are not separated by a barrier on the device, so the twin runs them thread
// after thread, in ascending or descending thread order: both must give the raster result
template <int R>
void host_ring(float *m, int W, int H, int band, bool reverse)
{
    const int nt = band + 2 * R;
    std::vector<float> ring((size_t)ring_size(R) * nt, 0.0f);
    std::vector<RingThread<R>> T((size_t)nt);
    for (int k = 0; k < band_count(band, H); k++) {
        const int i0 = k * band, rows = band_rows(band, H, k);
        const int s0 = first_step(R), ns = ring_steps(rows, W, R);
        for (int tid = 0; tid < nt; tid++) ring_begin<R>(T[tid], m, W, H, tid, i0, rows);
        for (int t = 0; t < ns; t += 4) {
            if (refill_point(t))
                for (int tid = 0; tid < nt; tid++) ring_refill<R>(T[tid], m, W, s0 + t);
            for (int u = 0; u < 4; u++)
                for (int q = 0; q < nt; q++) {
                    const int tid = reverse ? nt - 1 - q : q;
                    ring_step<R>(T[tid], m, W, ring.data(), nt, tid, s0 + t + u, u);
                }
        }
    }
}

int host_run(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, int impl, int band, int reverse)
{
    const int rc = mip_check(disp, pairs, stride, W, H, wnd_size);
    if (rc != SMT_OK) return rc;
    if ((impl != 0 && impl != 1) || band < 0) return SMT_ERR_ARG;
    const int r = radius(wnd_size);
    if (r == 0) return SMT_OK;
    if (stride == 0) stride = (size_t)H * W;
    const int cap = band_cap(impl, r);
    if (band == 0) band = cap;
    if (band > cap) return SMT_ERR_ARG;
    if (band > H) band = H;
    try {
        for (int b = 0; b < pairs; b++) {
            float *m = disp + (size_t)b * stride;
            if (impl == 1) host_plain(m, W, H, r, band);
            else if (r == 1) host_ring<1>(m, W, H, band, reverse != 0);
            else if (r == 2) host_ring<2>(m, W, H, band, reverse != 0);
            else host_ring<3>(m, W, H, band, reverse != 0);
        }
    } catch (const std::bad_alloc &) {
        return SMT_ERR_ALLOC;
    }
    return SMT_OK;
}

}  // namespace

SMT_API int smt_median_inplace_set_impl(int impl)
{
    if (impl != 0 && impl != 1) return SMT_ERR_ARG;
    g_impl = impl;
    return SMT_OK;
}

SMT_API int smt_median_filter_inplace(float *disp, int W, int H, int wnd_size, void *stream)
{
    const int rc = mip_check(disp, 1, 0, W, H, wnd_size);
    return rc != SMT_OK ? rc : mip_launch(disp, 1, 0, W, H, wnd_size, smt_stream(stream));
}

SMT_API int smt_median_filter_inplace_batch(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, void *stream)
{
    const int rc = mip_check(disp, pairs, stride, W, H, wnd_size);
    return rc != SMT_OK ? rc : mip_launch(disp, pairs, stride, W, H, wnd_size, smt_stream(stream));
}

SMT_API int smt_median_filter_inplace_host(float *disp, int pairs, size_t stride, int W, int H, int wnd_size)
{
    return host_run(disp, pairs, stride, W, H, wnd_size, g_impl, 0, 0);
}

SMT_API int smt_median_filter_inplace_host_ex(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, int impl,
                                              int band, int reverse)
{
    return host_run(disp, pairs, stride, W, H, wnd_size, impl, band, reverse);
}

// ---- CBLSM.cpp:155, :160-162 ----------------------------------------------------------------------------------------
SMT_API void smt_cblsm_post_default_params(smt_cblsm_post_params *p)
{
    if (!p) return;
    p->gate = 5;                                                               // :155
    p->speckle_diff = 1; p->speckle_min_area = 50; p->speckle_invalid = INT_MIN;   // :161, int(Invalid_Float) on x86
    p->median_wnd = 3;                                                         // :162
}

SMT_API int smt_cblsm_tail_batch(float *dispL, const float *dispR, int pairs, size_t stride, int H, int W,
                                 const smt_cblsm_post_params *post, uint8_t *cls, int *counts, int *err_dev, void *stream)
{
    if (pairs < 0) return SMT_ERR_ARG;
    smt_cblsm_post_params P;
    if (post) P = *post; else smt_cblsm_post_default_params(&P);
    if (!dispL || !dispR || !cls || H <= 0 || W <= 0 || P.median_wnd < 1 || P.median_wnd > 7) return SMT_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) || (stride != 0 && stride < (size_t)H * W)) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    const size_t N = (size_t)H * W, sd = stride ? stride : N;
    for (int b = 0; b < pairs; b++) {                                          // LeftRightConsistency, :160
        const int rc = smt_lrcheck(dispL + b * sd, dispR + b * sd, H, W, P.gate, cls + b * N, counts ? counts + 2 * b : nullptr,
                                   stream);
        if (rc != SMT_OK) return rc;
    }
    int rc = smt_remove_speckles_batch(dispL, pairs, sd, W, H, P.speckle_diff, P.speckle_min_area, P.speckle_invalid, err_dev,
                                       stream);                                // :161
    if (rc == SMT_OK) rc = smt_median_filter_inplace_batch(dispL, pairs, sd, W, H, P.median_wnd, stream);   // :162
    return rc;
}
