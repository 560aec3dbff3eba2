// The library's generic C ABI, used by every family: status strings, last HIP error, devices, memory, streams, smt_wta.
#include "smt_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;       // threads per workgroup (4 waves)

// WTA over an existing volume: one wave per pixel, lane owns C consecutive d (one vector load when
// D == 64*C), DPP argmin.
template <int C, bool FULL>
__global__ void __launch_bounds__(NT) k_wta(const float *__restrict__ vol, int N, int D,
                                            float *__restrict__ disp)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (NT / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= N) return;
    const int dl = lane * C;
    const float *c = vol + (size_t)p * D + dl;
    float v[C];
    if (FULL) {
        const vecf<C> x = *reinterpret_cast<const vecf<C> *>(c);
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = x.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) v[k] = (dl + k < D) ? c[k] : INFINITY;
    }
    const int wd = wave_wta<C, FULL>(v, dl, D);
    if (lane == 0) disp[p] = (float)wd;
}

}  // namespace

thread_local int g_smt_last_hip = 0;

SMT_API const char *smt_strerror(int s)
{
    switch (s) {
    case SMT_OK: return "ok";
    case SMT_ERR_ARG: return "invalid argument";
    case SMT_ERR_HIP: return "HIP runtime error";
    case SMT_ERR_ALLOC: return "device allocation failed";
    case SMT_ERR_DOMAIN: return "image values outside the integer 0..255 domain";
    case SMT_ERR_REF_UB: return "reference behaviour undefined for these inputs";
    case SMT_ERR_STATE: return "call order violated";
    default: return "unknown status";
    }
}
SMT_API int smt_version(void) { return SMT_VERSION; }
SMT_API int smt_last_hip_error(void) { return g_smt_last_hip; }
SMT_API int smt_device_count(int *n)
{
    if (!n) return SMT_ERR_ARG;
    SMT_HIP(hipGetDeviceCount(n));
    return SMT_OK;
}
SMT_API int smt_set_device(int d) { SMT_HIP(hipSetDevice(d)); return SMT_OK; }
SMT_API int smt_malloc(void **p, size_t n)
{
    if (!p) return SMT_ERR_ARG;
    hipError_t e = hipMalloc(p, n ? n : 1);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    return SMT_OK;
}
SMT_API int smt_free(void *p) { SMT_HIP(hipFree(p)); return SMT_OK; }
SMT_API int smt_memcpy_h2d(void *d, const void *s, size_t n, void *st)
{
    SMT_HIP(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_memcpy_d2h(void *d, const void *s, size_t n, void *st)
{
    SMT_HIP(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_memset(void *d, int b, size_t n, void *st)
{
    SMT_HIP(hipMemsetAsync(d, b, n, smt_stream(st)));
    return SMT_OK;
}
SMT_API int smt_stream_create(void **s)
{
    if (!s) return SMT_ERR_ARG;
    hipStream_t st;
    SMT_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *s = (void *)st;
    return SMT_OK;
}
SMT_API int smt_stream_destroy(void *s) { SMT_HIP(hipStreamDestroy(smt_stream(s))); return SMT_OK; }
SMT_API int smt_stream_sync(void *s) { SMT_HIP(hipStreamSynchronize(smt_stream(s))); return SMT_OK; }

SMT_API int smt_wta(const float *vol, int H, int W, int D, float *disp, void *stream)
{
    if (!vol || !disp || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || (size_t)H * W >= ((size_t)1 << 31))
        return SMT_ERR_ARG;                              // pixel indices are int; hypothesis addresses are (size_t)p * D
    const int N = H * W;
    dim3 grid((N + 3) / 4);
    const int C = (D + 63) / 64;
    hipStream_t st = smt_stream(stream);
    const bool full = (D == 64 * C) && C <= 4;
    (void)dispatch_c<SMT_MAX_DISPARITY / 64>(C, [&](auto c) {       // the vector-load form serves C <= 4 only
        constexpr int CC = decltype(c)::value;
        if constexpr (CC <= 4) {
            if (full) { hipLaunchKernelGGL((k_wta<CC, true>), grid, dim3(NT), 0, st, vol, N, D, disp); return; }
        }
        hipLaunchKernelGGL((k_wta<CC, false>), grid, dim3(NT), 0, st, vol, N, D, disp);
    });
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}
