// Sub-pixel WTA over an existing volume: smt_wta's kernel with the winner refined by the parabola through it and its two
// neighbours (subpixel_rule.h; the value SAD/Sad.h:76-81 and CBLSM/CBLSM.h:285-290 compute and drop).  The fused forms
// of the same rule live where the pipeline's maps are written (csrc/scanline.hip MODE 4, csrc/crossarm.hip SUB); this
// file holds the stand-alone kernel for any [N][D] float volume, the host twin and the parameter struct.
#include "smt_common.h"

namespace {

constexpr int NT = 256;

template <int C> struct vecf { float v[C]; };          // C = 5..8 (D > 256): never loaded as a vector
template <> struct vecf<1> { float v[1]; };
template <> struct __attribute__((aligned(8))) vecf<2> { float v[2]; };
template <> struct vecf<3> { float v[3]; };
template <> struct __attribute__((aligned(16))) vecf<4> { float v[4]; };

// One wave per pixel, lane owns C consecutive d (FULL: D == 64 * C and a 16-byte aligned volume, one vector load).
// Element offsets are 64-bit: p < 2^31 pixels of up to 512 hypotheses.
template <int C, bool FULL>
__global__ void __launch_bounds__(NT) k_wta_subpixel(const float *__restrict__ vol, int N, int D, float min_den,
                                                     float *__restrict__ disp)
{
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * (NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= N) return;
    const int dl = lane * C;
    const float *c = vol + ((size_t)p * (size_t)D + (size_t)dl);
    float v[C];
    if (FULL) {
        const vecf<C> x = *reinterpret_cast<const vecf<C> *>(c);
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = x.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = (dl + k < D) ? c[k] : INFINITY;
    }
    const float r = wave_wta_subpixel<C, FULL>(v, dl, D, min_den);
    if (lane == 0) disp[(size_t)p] = r;
}

}  // namespace

SMT_API void smt_subpixel_default_params(smt_subpixel_params *p)
{
    if (!p) return;
    p->min_den = 1.0f;                                   // Sad.h:80, CBLSM.h:289
}

SMT_API int smt_wta_subpixel(const float *vol, int H, int W, int D, const smt_subpixel_params *p, float *disp, void *stream)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || (size_t)H * W >= ((size_t)1 << 31))
        return SMT_ERR_ARG;                              // as smt_wta: pixel indices are int
    const float min_den = p ? p->min_den : 1.0f;
    if (!spx_min_den_ok(min_den)) return SMT_ERR_ARG;
    const int N = H * W;
    dim3 grid((unsigned)(((long long)N + 3) / 4));
    const int C = (D + 63) / 64;
    hipStream_t st = smt_stream(stream);
    const bool full = (D == 64 * C) && C <= 4 && ((uintptr_t)vol & 15) == 0;
#define SMT_WTAS(CC)                                                                                                   \
    do {                                                                                                               \
        if (full) hipLaunchKernelGGL((k_wta_subpixel<CC, true>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp);     \
        else hipLaunchKernelGGL((k_wta_subpixel<CC, false>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp);         \
    } while (0)
    switch (C) {
    case 1: SMT_WTAS(1); break;
    case 2: SMT_WTAS(2); break;
    case 3: SMT_WTAS(3); break;
    case 4: SMT_WTAS(4); break;
    case 5: hipLaunchKernelGGL((k_wta_subpixel<5, false>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp); break;
    case 6: hipLaunchKernelGGL((k_wta_subpixel<6, false>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp); break;
    case 7: hipLaunchKernelGGL((k_wta_subpixel<7, false>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp); break;
    default: hipLaunchKernelGGL((k_wta_subpixel<8, false>), grid, dim3(NT), 0, st, vol, N, D, min_den, disp); break;
    }
#undef SMT_WTAS
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_wta_subpixel_host(const float *vol, int H, int W, int D, const smt_subpixel_params *p, float *disp)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || (size_t)H * W >= ((size_t)1 << 31))
        return SMT_ERR_ARG;
    const float min_den = p ? p->min_den : 1.0f;
    if (!spx_min_den_ok(min_den)) return SMT_ERR_ARG;
    const size_t N = (size_t)H * W;
    for (size_t q = 0; q < N; q++) {
        const float *c = vol + q * (size_t)D;
        const int w = spx_winner(c, D);
        const bool edge = (w == 0 || w == D - 1);
        disp[q] = spx_refine(w, D, edge ? 0.0f : c[w - 1], c[w], edge ? 0.0f : c[w + 1], min_den);
    }
    return SMT_OK;
}
