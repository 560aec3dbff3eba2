// The reference's bilateral image filter (ASW/BiliteralFilter.h:49-142; include/smt_bilateral.h):
// two formulations that give identical bits, the host twin, and the tables.  The arithmetic is csrc/bilateral_rule.h.
//
//   k_bil_direct   the independent formulation: one thread per pixel, every tap a clamped read from global memory, both
//                  tables from global memory, the channels one after the other.
//   k_bil_staged   the hot path.  A workgroup of four waves owns a tile of 64 columns x 4 * PPT rows; the tile with its
//                  halo, clamped while loading, sits in LDS as bytes behind the 256-entry colour table.  A wave is one
//                  tile row of 64 pixels (consecutive bytes: no bank conflict on the sample reads), a thread owns PPT
//                  pixels in PPT consecutive rows, so it carries PPT * C independent chains of dependent float64 adds:
//                  3 for a colour image (PPT 1), 4 for a gray one (PPT 4).  The space weight of a tap is the same for
//                  every lane: its address is wave-uniform and the compiler reads it through the scalar cache
//                  (s_load_dwordx2; the kernel never writes either table).  Pass 2 recomputes the weight from the same
//                  two table entries; no weight is stored.
//                  LDS: 2 048 + (4 PPT + 2 hh)(64 + 2 ww) C bytes, 26 996 at 63 x 63 on three channels (five workgroups
//                  = 20 waves per CU), 11 876 on one.  The colour gather is one ds_read_b64 per sample: entry k lies on
//                  banks 2k and 2k + 1 of 64, so inside a group of 32 lanes two lanes collide when their differences
//                  are distinct and equal modulo 32; equal differences broadcast.
#include "smt_common.h"
#include "bilateral_rule.h"
#include "../../include/smt_bilateral.h"
#include <math.h>

namespace {
int g_bil_impl = 0;
int g_bil_last_form = 0;

constexpr int BIL_TW = 64;          // tile columns: one wave per tile row
constexpr int BIL_WAVES = 4;

template <int C, int divide>
__global__ void __launch_bounds__(256) k_bil_direct(const uint8_t *__restrict__ src, int images, int H, int W, int sw, int hh,
                                                    int ww, const double *__restrict__ space, const double *__restrict__ color,
                                                    uint8_t *__restrict__ dst, double *__restrict__ acc)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    for (int img = blockIdx.z; img < images; img += gridDim.z) {
        const size_t base = (size_t)img * H * W * C;
        for (int ch = 0; ch < C; ch++) {
            const size_t at = base + ((size_t)y * W + x) * C + ch;
            const int centre = src[at];
            double S = 0.0;
            for (int r = -hh; r <= hh; r++) {
                const size_t row = base + (size_t)bil_clamp(y + r, H) * W * C;
                for (int c = -ww; c <= ww; c++) {
                    const int q = src[row + (size_t)bil_clamp(x + c, W) * C + ch];
                    S = S + bil_weight(color[bil_diff(q, centre)], space[(r + hh) * sw + (c + ww)]);
                }
            }
            const double op = bil_norm_operand(S, divide);
            double a = 0.0;
            for (int r = -hh; r <= hh; r++) {
                const size_t row = base + (size_t)bil_clamp(y + r, H) * W * C;
                for (int c = -ww; c <= ww; c++) {
                    const int q = src[row + (size_t)bil_clamp(x + c, W) * C + ch];
                    const double wt = bil_weight(color[bil_diff(q, centre)], space[(r + hh) * sw + (c + ww)]);
                    a = bil_accumulate(a, q, bil_normalise(wt, op, divide));
                }
            }
            if (acc) acc[at] = a;
            dst[at] = bil_output(a);
        }
    }
}

template <int C, int PPT, int divide>
__global__ void __launch_bounds__(256) k_bil_staged(const uint8_t *__restrict__ src, int images, int H, int W, int sw, int hh,
                                                    int ww, const double *__restrict__ space, const double *__restrict__ color,
                                                    uint8_t *__restrict__ dst, double *__restrict__ acc)
{
    extern __shared__ double bil_lds[];
    double *ctab = bil_lds;                                             // [256]
    uint8_t *tile = reinterpret_cast<uint8_t *>(bil_lds + 256);         // [th][tw][C]
    constexpr int TH = BIL_WAVES * PPT, K = PPT * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * BIL_TW, y0 = blockIdx.y * TH;
    const int tw = BIL_TW + 2 * ww, th = TH + 2 * hh, rs = tw * C;
    ctab[threadIdx.x] = color[threadIdx.x];
    for (int img = blockIdx.z; img < images; img += gridDim.z) {
        const size_t base = (size_t)img * H * W * C;
        if (img != (int)blockIdx.z) __syncthreads();                    // the previous image's taps are read
        for (int i = threadIdx.x; i < th * tw; i += 256) {
            const int ty = i / tw, tx = i - ty * tw;
            const size_t from = base + ((size_t)bil_clamp(y0 + ty - hh, H) * W + bil_clamp(x0 + tx - ww, W)) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) tile[i * C + ch] = src[from + ch];
        }
        __syncthreads();
        // this thread's PPT pixels: rows wave * PPT + p of the tile, column `lane`; mine = their first sample at tap (0, 0)
        const uint8_t *mine = tile + (wave * PPT) * rs + lane * C;
        int centre[K];
        double S[K], a[K];
#pragma unroll
        for (int p = 0; p < PPT; p++)
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                centre[p * C + ch] = mine[(p + hh) * rs + ww * C + ch];
                S[p * C + ch] = 0.0;
                a[p * C + ch] = 0.0;
            }
        for (int r = 0; r <= 2 * hh; r++) {
            const double *srow = space + r * sw;
            const uint8_t *trow = mine + r * rs;
#pragma unroll 4
            for (int c = 0; c <= 2 * ww; c++) {
                const double sp = srow[c];                              // wave-uniform
#pragma unroll
                for (int p = 0; p < PPT; p++)
#pragma unroll
                    for (int ch = 0; ch < C; ch++) {
                        const int q = trow[p * rs + c * C + ch];
                        S[p * C + ch] = S[p * C + ch] + bil_weight(ctab[bil_diff(q, centre[p * C + ch])], sp);
                    }
            }
        }
        double op[K];
#pragma unroll
        for (int k = 0; k < K; k++) op[k] = bil_norm_operand(S[k], divide);
        for (int r = 0; r <= 2 * hh; r++) {
            const double *srow = space + r * sw;
            const uint8_t *trow = mine + r * rs;
#pragma unroll 4
            for (int c = 0; c <= 2 * ww; c++) {
                const double sp = srow[c];
#pragma unroll
                for (int p = 0; p < PPT; p++)
#pragma unroll
                    for (int ch = 0; ch < C; ch++) {
                        const int k = p * C + ch, q = trow[p * rs + c * C + ch];
                        const double wt = bil_weight(ctab[bil_diff(q, centre[k])], sp);
                        a[k] = bil_accumulate(a[k], q, bil_normalise(wt, op[k], divide));
                    }
            }
        }
        const int x = x0 + lane;
#pragma unroll
        for (int p = 0; p < PPT; p++) {
            const int y = y0 + wave * PPT + p;
            if (x < W && y < H) {
                const size_t at = base + ((size_t)y * W + x) * C;
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    if (acc) acc[at + ch] = a[p * C + ch];
                    dst[at + ch] = bil_output(a[p * C + ch]);
                }
            }
        }
    }
}

int bil_check(const void *src, int images, int H, int W, int channels, int wsize_h, int wsize_w, const double *space,
              const double *color, int norm, const void *dst)
{
    if (!src || !dst || !space || !color || src == dst || images < 0 || H <= 0 || W <= 0) return SMT_ERR_ARG;
    if ((channels != 1 && channels != 3) || wsize_h < 1 || wsize_h > 64 || wsize_w < 1 || wsize_w > 64) return SMT_ERR_ARG;
    if (norm != SMT_BILATERAL_NORM_RECIPROCAL && norm != SMT_BILATERAL_NORM_DIVIDE) return SMT_ERR_ARG;
    return SMT_OK;
}
}  // namespace

SMT_API int smt_bilateral_masks(int wsize_h, int wsize_w, double sigma_space, double sigma_color, double *space_host,
                                double *color_host)
{
    if (!space_host || !color_host || wsize_h < 1 || wsize_h > 64 || wsize_w < 1 || wsize_w > 64) return SMT_ERR_ARG;
    const int ch = (wsize_h - 1) / 2, cw = (wsize_w - 1) / 2;
    for (int i = 0; i < wsize_h; i++) {
        const double y = (double)((i - ch) * (i - ch));                                       // pow(i - center_h, 2), :22
        for (int j = 0; j < wsize_w; j++) {
            const double x = (double)((j - cw) * (j - cw));                                   // :25
            space_host[i * wsize_w + j] = exp(-(x + y) / (2 * sigma_space * sigma_space));    // :26
        }
    }
    for (int i = 0; i < 256; i++) color_host[i] = exp(-(i * i) / (2 * sigma_color * sigma_color));   // :39
    return SMT_OK;
}

SMT_API int smt_bilateral_set_impl(int impl)
{
    if (impl != 0 && impl != SMT_BILATERAL_FORM_DIRECT && impl != SMT_BILATERAL_FORM_STAGED) return SMT_ERR_ARG;
    g_bil_impl = impl;
    return SMT_OK;
}

SMT_API int smt_bilateral_last_form(void) { return g_bil_last_form; }

SMT_API int smt_bilateral_filter_batch(const uint8_t *src, int images, int H, int W, int channels, int wsize_h, int wsize_w,
                                       const double *space, const double *color, int norm, uint8_t *dst, double *acc,
                                       void *stream)
{
    const int rc = bil_check(src, images, H, W, channels, wsize_h, wsize_w, space, color, norm, dst);
    if (rc != SMT_OK || images == 0) return rc;
    hipStream_t st = smt_stream(stream);
    const int hh = (wsize_h - 1) / 2, ww = (wsize_w - 1) / 2, divide = norm == SMT_BILATERAL_NORM_DIVIDE;
    // the default: the staged form at every measured point
    const int form = g_bil_impl ? g_bil_impl : SMT_BILATERAL_FORM_STAGED;
    const unsigned gz = (unsigned)(images < 1024 ? images : 1024);
    if (form == SMT_BILATERAL_FORM_DIRECT) {
        const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), gz), block(64, 4);
        if (grid.y > 65535u) return SMT_ERR_ARG;
#define BIL_DIRECT(C, DIV) hipLaunchKernelGGL((k_bil_direct<C, DIV>), grid, block, 0, st, src, images, H, W, wsize_w, hh, ww, space, color, dst, acc)
        if (channels == 1) { if (divide) BIL_DIRECT(1, 1); else BIL_DIRECT(1, 0); }
        else { if (divide) BIL_DIRECT(3, 1); else BIL_DIRECT(3, 0); }
#undef BIL_DIRECT
    } else {
        const int ppt = channels == 1 ? 4 : 1, TH = BIL_WAVES * ppt;
        const dim3 grid((unsigned)((W + BIL_TW - 1) / BIL_TW), (unsigned)((H + TH - 1) / TH), gz), block(256);
        if (grid.y > 65535u) return SMT_ERR_ARG;
        const size_t lds = 256 * sizeof(double) + (size_t)(TH + 2 * hh) * (BIL_TW + 2 * ww) * channels;
#define BIL_STAGED(C, PPT, DIV) hipLaunchKernelGGL((k_bil_staged<C, PPT, DIV>), grid, block, lds, st, src, images, H, W, wsize_w, hh, ww, space, color, dst, acc)
        if (channels == 1) { if (divide) BIL_STAGED(1, 4, 1); else BIL_STAGED(1, 4, 0); }
        else { if (divide) BIL_STAGED(3, 1, 1); else BIL_STAGED(3, 1, 0); }
#undef BIL_STAGED
    }
    SMT_LAUNCH_CHECK();
    g_bil_last_form = form;
    return SMT_OK;
}

SMT_API int smt_bilateral_filter_host(const uint8_t *src, int images, int H, int W, int channels, int wsize_h, int wsize_w,
                                      const double *space, const double *color, int norm, uint8_t *dst, double *acc)
{
    const int rc = bil_check(src, images, H, W, channels, wsize_h, wsize_w, space, color, norm, dst);
    if (rc != SMT_OK) return rc;
    const int hh = (wsize_h - 1) / 2, ww = (wsize_w - 1) / 2, divide = norm == SMT_BILATERAL_NORM_DIVIDE, C = channels;
    for (int img = 0; img < images; img++) {
        const size_t base = (size_t)img * H * W * C;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int ch = 0; ch < C; ch++) {
                    const size_t at = base + ((size_t)y * W + x) * C + ch;
                    const int centre = src[at];
                    auto tap = [&](int r, int c) {
                        return (int)src[base + ((size_t)bil_clamp(y + r, H) * W + bil_clamp(x + c, W)) * C + ch];
                    };
                    double S = 0.0;
                    for (int r = -hh; r <= hh; r++)
                        for (int c = -ww; c <= ww; c++)
                            S = S + bil_weight(color[bil_diff(tap(r, c), centre)], space[(r + hh) * wsize_w + (c + ww)]);
                    const double op = bil_norm_operand(S, divide);
                    double a = 0.0;
                    for (int r = -hh; r <= hh; r++)
                        for (int c = -ww; c <= ww; c++) {
                            const int q = tap(r, c);
                            const double wt = bil_weight(color[bil_diff(q, centre)], space[(r + hh) * wsize_w + (c + ww)]);
                            a = bil_accumulate(a, q, bil_normalise(wt, op, divide));
                        }
                    if (acc) acc[at] = a;
                    dst[at] = bil_output(a);
                }
    }
    return SMT_OK;
}
