// Shared host/device helpers for libsmt_hip.so (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdint.h>
#include <type_traits>
#include "../../include/smt.h"
#include "subpixel_rule.h"

#define SMT_API extern "C" __attribute__((visibility("default")))

extern thread_local int g_smt_last_hip;

#define SMT_HIP(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) {                            \
            g_smt_last_hip = (int)_e;                      \
            return SMT_ERR_HIP;                            \
        }                                                  \
    } while (0)

#define SMT_LAUNCH_CHECK()                                 \
    do {                                                   \
        hipError_t _e = hipGetLastError();                 \
        if (_e != hipSuccess) {                            \
            g_smt_last_hip = (int)_e;                      \
            return SMT_ERR_HIP;                            \
        }                                                  \
    } while (0)

static inline hipStream_t smt_stream(void *s) { return (hipStream_t)s; }

// Every handle remembers the device it was created on; its entry points make that device current for
// the duration of the call and restore the caller's afterwards (one host thread may drive several GPUs).
struct smt_dev_guard {
    int prev = -1;
    explicit smt_dev_guard(int dev)
    {
        int cur = -1;
        if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~smt_dev_guard() { if (prev >= 0) (void)hipSetDevice(prev); }
    smt_dev_guard(const smt_dev_guard &) = delete;
    smt_dev_guard &operator=(const smt_dev_guard &) = delete;
};
static inline int smt_current_device() { int d = -1; return hipGetDevice(&d) == hipSuccess ? d : -1; }

// Stream-ordered scratch for smt_asw and smt_ncc (tables that live for one call): csrc/scratch.hip owns the one pool
// set of the library.  Free with smt_scratch_free on the same stream.
hipError_t smt_scratch_alloc(void **p, size_t bytes, hipStream_t st);
void smt_scratch_free(void *p, hipStream_t st);
struct scratch_set {                                       // arena blocks of one call, freed in reverse order
    hipStream_t st;
    void *p[6];
    int n = 0;
    explicit scratch_set(hipStream_t s) : st(s) {}
    void *get(size_t bytes)
    {
        void *q = nullptr;
        if (n >= 6 || smt_scratch_alloc(&q, bytes, st) != hipSuccess) return nullptr;
        p[n++] = q;
        return q;
    }
    ~scratch_set() { while (n > 0) smt_scratch_free(p[--n], st); }
};

// Batched RemoveSpeckles on caller-owned scratch (csrc/speckle.hip; smt_pipeline_run_batch_post owns one for a pair):
// smt_speckle_scratch_bytes(pairs, W, H) bytes, arguments already checked.  Enqueues four launches on `st`.
size_t smt_speckle_scratch_bytes(int pairs, int W, int H);
int smt_speckle_enqueue(float *disp, int pairs, size_t stride, int W, int H, int diff_insame, unsigned min_speckle_area,
                        int invalid_val, void *scratch, int *err_dev, hipStream_t st);

// filterSpeckles on uint8 maps (csrc/speckle.hip: the same kernels for uint8 pixels, 4 neighbours, `<=`), on the same
// scratch size, arguments already checked.  Four launches on `st` (three when maxSpeckleSize < 0).
int smt_speckle_u8_enqueue(uint8_t *maps, int pairs, size_t stride, int W, int H, int newVal, int maxSpeckleSize,
                           int maxDiff, void *scratch, int *err_dev, hipStream_t st);

// The fused costAggregationV4 of smt_cblsm_flow_run_batch_v4 (csrc/cblsm_v4.hip): S = the uint32 summed-area table of
// the left view's AD volume, armL / armR = the four [H][W] arm maps (left, right, up, down) of the left / right image.
// Writes the WTA map to `disp` and, unless NULL, the aggregated volume to `vol`; ORs 1 into *err_dev when a rectangle
// had to be clipped to the plane.  Arguments already checked (D <= SMT_MAX_DISPARITY).  One launch on `st`.
int smt_cblsm_v4_box_enqueue(const uint32_t *S, int *const armL[4], int *const armR[4], int H, int W, int D, float *vol,
                             float *disp, int *err_dev, hipStream_t st);

// The three NCC cost launches over `pairs` dense pairs ([pairs][H][W] images, tables and maps, [pairs][H][W][D] costs;
// smt_ncc passes 1), arguments already checked, one launch each with the pair on a grid axis.  loop (csrc/window.hip):
// k_ncc, writes every pixel of disp.  dot4 (csrc/window.hip, side <= 31) and box (csrc/ncc_box.hip, side <= 181) write
// interior pixels only, need a non-empty interior and the tables of the statistics pass (csrc/ncc_common.h).  Each
// records its SMT_NCC_FORM_* in g_smt_ncc_last_form.
extern int g_smt_ncc_last_form;
int smt_ncc_loop_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int winSize, int32_t *disp,
                         double *cost, hipStream_t st);
// rkeys (dot4 and box): NULL, or a zeroed [pairs][H][W] map into which the launch also publishes, under an agent-scope
// maximum, the rank key (csrc/ncc_keys.h) of every real, non-NaN cost of (x, d) at right pixel x - d.
int smt_ncc_dot4_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int winSize, const int *sumL,
                         const double *rootL, const int *sumR, const double *rootR, int32_t *disp, double *cost, hipStream_t st,
                         unsigned long long *rkeys = nullptr);
int smt_ncc_box_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int winSize, const int *sumL,
                        const double *rootL, const int *sumR, const double *rootR, int32_t *disp, double *cost, hipStream_t st,
                        unsigned long long *rkeys = nullptr);
// The statistics pass of csrc/ncc_common.h as csrc/ncc_box.hip holds it, and the impl smt_ncc would run now (1, 2, 3).
bool smt_ncc_stats_ready(int winSize);
int smt_ncc_stats_enqueue(const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int winSize, int *sumL, double *rootL,
                          int *sumR, double *rootR, hipStream_t st);
int smt_ncc_current_impl(void);
// Both NCC views of `pairs` dense pairs (csrc/ncc_both.hip), arguments already checked: `form` is the SMT_NCC_FORM_* of the
// left view; the four tables hold room for the batch unless the form is the loop nest (they are filled here); dispL and
// dispR are required, costL and costR optional.  Records SMT_LRNCC_FORM_* for smt_lrncc_last_form.
int smt_lrncc_enqueue(int form, const uint8_t *L, const uint8_t *R, int pairs, int H, int W, int D, int winSize, int *sumL,
                      double *rootL, int *sumR, double *rootR, int32_t *dispL, int32_t *dispR, double *costL, double *costR,
                      hipStream_t st);

// The SMT_QUIRK_* flags of a cross-arm handle after create (csrc/crossarm.hip), for smt_pipeline_set_quirks: they take
// effect from the next arms call.  SMT_ERR_ARG for an unknown bit.
int smt_crossarm_set_quirks_internal(smt_crossarm *h, unsigned quirks);

// A launcher's ladder over its kernel instantiations: run-time hypotheses per lane C -> f(std::integral_constant<int, C>)
// for 1 <= C <= CMAX, true; false, and no call, for any other C.  What f instantiates is the whole kernel set.
template <int CMAX, class F>
static inline bool dispatch_c(int C, F &&f)
{
    if constexpr (CMAX > 0) {
        if (C == CMAX) { f(std::integral_constant<int, CMAX>{}); return true; }
        return dispatch_c<CMAX - 1>(C, f);
    }
    return false;
}

#ifdef __HIPCC__
constexpr int WAVE = 64;

template <int C> struct vecf { float v[C]; };          // C = 5..8 (D > 256): plain struct, the kernels there use the per-element paths
template <> struct vecf<1> { float v[1]; };
template <> struct __attribute__((aligned(8))) vecf<2> { float v[2]; };
template <> struct vecf<3> { float v[3]; };
template <> struct __attribute__((aligned(16))) vecf<4> { float v[4]; };

// std::min / std::max semantics of the reference (returns the FIRST argument on ties and
// for the +0/-0 pair), kept instead of fminf so that signs of zero cannot diverge.
__device__ __forceinline__ float ref_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float ref_max(float a, float b) { return (a < b) ? b : a; }

// Wave-wide minimum of non-NaN floats (all 64 lanes active).
__device__ __forceinline__ float wave_min_f32(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, WAVE));
    return v;
}
// ---- DPP wave reductions (gfx9 row_bcast forms; all 64 lanes must be active) ------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_u32(unsigned v)
{
    // old = identity of umin so the DPP combiner can fold the move into v_min_u32_dpp
    return (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xF, false);
}
// the steps of the wave minimum behind the first quad_perm step, shared by the two forms below
__device__ __forceinline__ unsigned wave_min_u32_tail(unsigned v)
{
    v = min(v, dpp_u32<0x4E, 0xF>(v));    // quad_perm [2,3,0,1]
    v = min(v, dpp_u32<0x141, 0xF>(v));   // row_half_mirror
    v = min(v, dpp_u32<0x140, 0xF>(v));   // row_mirror      -> every lane holds its row's min
    v = min(v, dpp_u32<0x142, 0xA>(v));   // row_bcast15 into rows 1,3
    v = min(v, dpp_u32<0x143, 0xC>(v));   // row_bcast31 into rows 2,3 -> lane 63 holds the min
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// minimum over the wave of unsigned keys, returned wave-uniform (SGPR).
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, dpp_u32<0xB1, 0xF>(v));    // quad_perm [1,0,3,2]
    return wave_min_u32_tail(v);
}
// wave_min_u32 for a caller that needs v again afterwards.  The compiler's DPP form ties source and destination, so the
// first step above copies such a v first; here that step is written out untied.  Every lane of a quad_perm is valid, so
// the value is the same.  The s_nops are the two wait states between a vector write and a DPP read of the same register,
// on both sides of the step.
__device__ __forceinline__ unsigned wave_min_u32_untied(unsigned v)
{
    unsigned w;
    asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 1" : "=v"(w) : "v"(v));
    return wave_min_u32_tail(w);
}
// order-preserving map float -> uint32 (handles negatives; NaNs are not ordered -- wave_wta gives them
// the reference's semantics)
__device__ __forceinline__ unsigned f32_key(float f)
{
    const unsigned b = __float_as_uint(f + 0.0f);          // -0 -> +0 so that equal zeros tie
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// WTA of one pixel held by a wave (lane l owns the C hypotheses dl = l*C .. l*C+C-1; elements at or past
// D are ignored), with the reference's exact rule (CrossArm.cpp:44-52, ScanlineOptimizer.h:51-59,
// AD-Census.h:355-373): `cost = vol[0]; for d >= 1: if (cost > vol[d]) { cost = vol[d]; best = d; }`.
// A NaN never satisfies `cost > value`, so a NaN entry never wins, and a NaN at d = 0 freezes the
// result at 0 (every later comparison against it is false).  NaN keys sort above +inf; -0 ties +0.
template <int C, bool FULL>
__device__ __forceinline__ int wave_wta(const float (&v)[C], int dl, int D)
{
    unsigned best = 0xFFFFFFFFu; int bk = 0;
#pragma unroll
    for (int k = 0; k < C; k++)
        if (FULL || dl + k < D) {
            const unsigned key = (v[k] != v[k]) ? 0xFFFFFFFFu : f32_key(v[k]);
            if (k == 0 || key < best) { best = key; bk = k; }
        }
    const unsigned m = wave_min_u32(best);
    const unsigned long long b = __ballot(best == m);
    const int first = __builtin_ctzll(b);
    const int wd = __builtin_amdgcn_readlane(dl + bk, first);
    const int nan0 = __builtin_amdgcn_readlane((int)(v[0] != v[0]), 0);   // lane 0 owns d = 0
    return nan0 ? 0 : wd;
}

// wave_wta with the winner refined by the parabola through it and its two neighbours (spx_refine, subpixel_rule.h),
// returned wave-uniform.  The neighbours d = w - 1 and w + 1 sit in lane d / C, register d % C: every register of that
// lane is read with v_readlane at the wave-uniform lane and an unrolled scalar select on the wave-uniform d % C picks
// one, so nothing goes through LDS and the row is not read again.  (Selecting the register first and reading one lane
// is the same thing to the compiler as v[d % C], and it moves such an array to LDS.)  A winner at either end of the
// range is returned as it is.
template <int C, bool FULL>
__device__ __forceinline__ float wave_wta_subpixel(const float (&v)[C], int dl, int D, float min_den)
{
    const int w = wave_wta<C, FULL>(v, dl, D);
    if (w == 0 || w == D - 1) return (float)w;
    auto at = [&](int d) {
        const int l = d / C, r = d - l * C;
        int x = __builtin_amdgcn_readlane(__float_as_int(v[0]), l);
#pragma unroll
        for (int k = 1; k < C; k++) {
            const int xk = __builtin_amdgcn_readlane(__float_as_int(v[k]), l);
            x = (r == k) ? xk : x;
        }
        return __int_as_float(x);
    };
    return spx_refine(w, D, at(w - 1), at(w), at(w + 1), min_den);
}

// Correctly rounded a[k] / b for a wave-uniform integer-valued divisor 1 <= b <= 65535 (a rectangle area, a support
// count) in 3 vector instructions per value instead of the 11 of the IEEE division sequence.  With r = v_rcp_f32(b)
// (error <= 1 ulp; 2 would do), q0 = RN(a r), rem = fma(-q0, b, a), q = fma(rem, r, q0):
//  * |q0 - a/b| < 3 ulp, so rem = a - q0 b is a multiple of ulp(q0) and fewer than 2^19 of them: exact in the fma;
//  * q0 + rem r = a/b + (a/b - q0) e1 with |e1| <= 2^-23: within 2^-21 ulp of the true quotient;
//  * a/b is never closer than 2^-17 ulp to a rounding boundary (for a midpoint m, a - b m is a non-zero multiple of half
//    an ulp of the quotient -- b m has 25 significant bits or more, a has 24 -- and b < 2^16),
// so the final rounding is the rounding of a/b.  That holds while nothing leaves the normal range: every value the wave
// holds for the pixel must lie in [2^-60, 2^61) (zeros, denormals, infinities, NaNs and larger divisors take the
// division), checked with one ballot.  Elements at or past D do not count.  All 64 lanes must be active.
template <int C, bool FULL>
__device__ __forceinline__ void wave_quotient(const float (&a)[C], float b, int dl, int D, float (&q)[C])
{
    bool fast = false;
    if (b >= 1.0f && b <= 65535.0f) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < C; k++) {
            const unsigned t = (__float_as_uint(a[k]) << 1) - (67u << 24);       // biased exponent - 67, sign dropped
            ok = ok && ((!FULL && dl + k >= D) || t < (121u << 24));
        }
        fast = __ballot(!ok) == 0;
    }
    if (fast) {
        float r = __builtin_amdgcn_rcpf(b), bv = b;
        asm volatile("" : "+v"(r), "+v"(bv));              // vector operands: an SGPR multiplier halves the FMA rate
#pragma unroll
        for (int k = 0; k < C; k++) {
            const float q0 = a[k] * r;
            const float rem = __builtin_fmaf(-q0, bv, a[k]);
            q[k] = __builtin_fmaf(rem, r, q0);
        }
    } else {
#pragma unroll
        for (int k = 0; k < C; k++) q[k] = a[k] / b;
    }
}

// First-strict-minimum WTA across a wave whose lanes hold candidates in increasing-d
// order: (v, d) = this lane's first local minimum (v = +inf for lanes with no candidate).
// Returns the winning d, wave-uniform.  All 64 lanes must be active.
__device__ __forceinline__ int wave_argmin_first(float v, int d)
{
    const unsigned key = f32_key(v);
    const unsigned m = wave_min_u32(key);
    const unsigned long long b = __ballot(key == m);
    const int first = __builtin_ctzll(b);
    return __builtin_amdgcn_readlane(d, first);
}
#endif
