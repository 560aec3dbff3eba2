// The tail of ASW/ASWeight.cpp (:67-78) for a batch of maps on the device:
//   :67-72  normalize(.., 0, 255, NORM_MINMAX) + convertTo(CV_8UC1)     smt_minmax_normalize_[f32_]u8_batch   3 launches
//   :73     filterSpeckles(lastDisp, 0, 40, 2)                           smt_filter_speckles_u8_batch (speckle.hip)  4
//   :74,:78 medianBlur(lastDisp, lastDisp, 5 / 3)                        smt_median_blur_u8_batch               1
//   :76     FillImageNew(lastDisp) (ASW.h:434-511)                       smt_fill_image_new_batch               3
// Every launch count is fixed whatever the data and the pair count; nothing synchronises; scratch comes from the arena.
// The OpenCV steps are the library's restatement of OpenCV 3.1 (include/smt.h, "parity unpinned").
#include "smt_common.h"
#include "fill_image_rules.h"
#include "median_net.h"
#include <float.h>
#include <new>
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int MAX_GRID_Y = 65535;

int tail_check(const void *a, const void *b, int pairs, size_t stride, int H, int W)
{
    if (!a || !b || pairs <= 0 || H <= 0 || W <= 0) return SMT_ERR_ARG;
    if ((long long)H * W >= (1ll << 28)) return SMT_ERR_ARG;
    if (stride != 0 && stride < (size_t)H * W) return SMT_ERR_ARG;
    return SMT_OK;
}
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- normalize(src, dst, 0, 255, NORM_MINMAX) --------------------------------------------------------------------
constexpr int MM_PER_THREAD = 16, MM_CHUNK = NT * MM_PER_THREAD;

__device__ __forceinline__ unsigned mm_key(uint8_t v) { return v; }
__device__ __forceinline__ unsigned mm_key(float v) { return f32_key(v); }
__device__ __forceinline__ float mm_unkey_f32(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__global__ void k_mm_init(unsigned *mm, int pairs)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < pairs) { mm[2 * b] = 0xFFFFFFFFu; mm[2 * b + 1] = 0u; }
}

// one agent-scope atomic min and max per wave into the map's slot pair
template <class T>
__global__ void __launch_bounds__(NT) k_mm_reduce(const T *__restrict__ in, int pairs, size_t stride, size_t n, unsigned *mm)
{
    const size_t i0 = (size_t)blockIdx.x * MM_CHUNK;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const T *p = in + (size_t)b * stride;
        unsigned lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll 4
        for (int k = 0; k < MM_PER_THREAD; k++) {
            const size_t i = i0 + (size_t)k * NT + threadIdx.x;
            if (i < n) { const unsigned key = mm_key(p[i]); lo = min(lo, key); hi = max(hi, key); }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, off, WAVE));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, off, WAVE));
        }
        if ((threadIdx.x & (WAVE - 1)) == 0 && lo <= hi) {
            atomicMin(mm + 2 * b, lo);
            atomicMax(mm + 2 * b + 1, hi);
        }
    }
}

// scale and shift in double, convertTo's multiply and add in float, each rounded on its own (no fused multiply-add),
// then saturate_cast<uchar>: round half to even, clamp.
__device__ __forceinline__ void mm_scale_shift(double smin, double smax, float &scale_f, float &shift_f)
{
    const double d = smax - smin;
    const double scale = 255.0 * (d > DBL_EPSILON ? __ddiv_rn(1.0, d) : 0.0);
    const double shift = 0.0 - __dmul_rn(smin, scale);
    scale_f = (float)scale;
    shift_f = (float)shift;
}
__device__ __forceinline__ uint8_t mm_sat_u8(float t)
{
    float r = rintf(t);                                        // round to nearest, ties to even
    r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    return (uint8_t)(int)r;
}

template <class T>
__global__ void __launch_bounds__(NT) k_mm_apply(const T *in, uint8_t *out, int pairs, size_t stride, size_t n,
                                                 const unsigned *__restrict__ mm)
{
    const size_t i0 = (size_t)blockIdx.x * MM_CHUNK;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const unsigned klo = mm[2 * b], khi = mm[2 * b + 1];
        float scale_f, shift_f;
        if (sizeof(T) == 1) mm_scale_shift((double)klo, (double)khi, scale_f, shift_f);
        else mm_scale_shift((double)mm_unkey_f32(klo), (double)mm_unkey_f32(khi), scale_f, shift_f);
        const T *p = in + (size_t)b * stride;
        uint8_t *q = out + (size_t)b * stride;
#pragma unroll 4
        for (int k = 0; k < MM_PER_THREAD; k++) {
            const size_t i = i0 + (size_t)k * NT + threadIdx.x;
            if (i >= n) continue;
            float t = __fmul_rn((float)p[i], scale_f);
            t = __fadd_rn(t, shift_f);                             // float maps: :67-68's float result, :70-71 round it
            q[i] = mm_sat_u8(t);
        }
    }
}

template <class T>
int normalize_enqueue(const T *in, uint8_t *out, int pairs, size_t stride, int H, int W, void *scratch, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    if (stride == 0) stride = n;
    unsigned *mm = (unsigned *)scratch;
    const dim3 grid((unsigned)((n + MM_CHUNK - 1) / MM_CHUNK), pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    hipLaunchKernelGGL(k_mm_init, dim3((pairs + NT - 1) / NT), dim3(NT), 0, st, mm, pairs);
    hipLaunchKernelGGL(k_mm_reduce<T>, grid, dim3(NT), 0, st, in, pairs, stride, n, mm);
    hipLaunchKernelGGL(k_mm_apply<T>, grid, dim3(NT), 0, st, in, out, pairs, stride, n, (const unsigned *)mm);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}
size_t normalize_scratch_bytes(int pairs) { return up256((size_t)pairs * 8); }

// ---- medianBlur(src, dst, k), k = 3 or 5, BORDER_REPLICATE --------------------------------------------------------
// A workgroup owns MB_TH rows x MB_TW columns of outputs: the tile and its replicate halo are staged in LDS (coordinates
// clamped into the image, so a window wider than the image is all border), a thread selects four adjacent outputs of
// one row as two packed pairs of 16-bit lanes (v_pk_min_u16 / v_pk_max_u16: one instruction, two pixels).
constexpr int MB_TW = 64, MB_TH = 16, MB_R = 2, MB_PITCH = 72;     // pitch: a multiple of 4 >= MB_TW + 2 * MB_R
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

template <int K>
__global__ void __launch_bounds__(NT) k_median_blur(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int pairs,
                                                    size_t in_stride, size_t out_stride, int W, int H, int ntx)
{
    constexpr int R = K / 2, LW = MB_TW + 2 * R, LH = MB_TH + 2 * R;
    __shared__ __attribute__((aligned(8))) uint8_t tile[(MB_TH + 2 * MB_R) * MB_PITCH + 8];
    const int ty0 = blockIdx.x / ntx, tx0 = blockIdx.x - ty0 * ntx;
    const int y0 = ty0 * MB_TH, x0 = tx0 * MB_TW;
    const int tx = threadIdx.x % (MB_TW / 4), ty = threadIdx.x / (MB_TW / 4);
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const uint8_t *src = in + (size_t)b * in_stride;
        for (int i = threadIdx.x; i < LW * LH; i += NT) {
            const int ry = i / LW, rx = i - ry * LW;
            const int gy = min(max(y0 + ry - R, 0), H - 1), gx = min(max(x0 + rx - R, 0), W - 1);
            tile[ry * MB_PITCH + rx] = src[(size_t)gy * W + gx];
        }
        __syncthreads();
        const int y = y0 + ty, x = x0 + 4 * tx;
        if (y < H && x < W) {
            u16x2 pa[K * K], pb[K * K];
#pragma unroll
            for (int dy = 0; dy < K; dy++) {
                // the K + 3 bytes of this row under the four windows, from two aligned dwords
                const unsigned *wp = (const unsigned *)(tile + (ty + dy) * MB_PITCH + 4 * tx);
                const unsigned w0 = wp[0], w1 = wp[1];
                unsigned short c[8];
#pragma unroll
                for (int j = 0; j < 4; j++) { c[j] = (w0 >> (8 * j)) & 0xFF; c[4 + j] = (w1 >> (8 * j)) & 0xFF; }
#pragma unroll
                for (int dx = 0; dx < K; dx++) {
                    pa[dy * K + dx] = u16x2{c[dx], c[dx + 1]};
                    pb[dy * K + dx] = u16x2{c[dx + 2], c[dx + 3]};
                }
            }
            auto mn = [](u16x2 p, u16x2 q) { return __builtin_elementwise_min(p, q); };
            auto mx = [](u16x2 p, u16x2 q) { return __builtin_elementwise_max(p, q); };
            mednet_run<K * K>(pa, mn, mx);
            mednet_run<K * K>(pb, mn, mx);
            uint8_t *dst = out + (size_t)b * out_stride + (size_t)y * W + x;
            const u16x2 ma = pa[K * K / 2], mb = pb[K * K / 2];
            dst[0] = (uint8_t)ma.x;
            if (x + 1 < W) dst[1] = (uint8_t)ma.y;
            if (x + 2 < W) dst[2] = (uint8_t)mb.x;
            if (x + 3 < W) dst[3] = (uint8_t)mb.y;
        }
        __syncthreads();                                          // tile reused by the next pair
    }
}

int median_blur_enqueue(const uint8_t *in, uint8_t *out, int pairs, size_t in_stride, size_t out_stride, int W, int H,
                        int ksize, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    if (in_stride == 0) in_stride = n;
    if (out_stride == 0) out_stride = n;
    const int ntx = (W + MB_TW - 1) / MB_TW, nty = (H + MB_TH - 1) / MB_TH;
    const dim3 grid((unsigned)ntx * nty, pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    if (ksize == 3)
        hipLaunchKernelGGL(k_median_blur<3>, grid, dim3(NT), 0, st, in, out, pairs, in_stride, out_stride, W, H, ntx);
    else
        hipLaunchKernelGGL(k_median_blur<5>, grid, dim3(NT), 0, st, in, out, pairs, in_stride, out_stride, W, H, ntx);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// the optional copies of the tail's intermediate states: dense maps -> maps `out_stride` apart
__global__ void __launch_bounds__(NT) k_copy_maps(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int pairs,
                                                  size_t out_stride, size_t n)
{
    const size_t i0 = (size_t)blockIdx.x * MM_CHUNK;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y)
        for (int k = 0; k < MM_PER_THREAD; k++) {
            const size_t i = i0 + (size_t)k * NT + threadIdx.x;
            if (i < n) out[(size_t)b * out_stride + i] = in[(size_t)b * n + i];
        }
}
int copy_maps_enqueue(const uint8_t *in, uint8_t *out, int pairs, size_t out_stride, size_t n, hipStream_t st)
{
    const dim3 grid((unsigned)((n + MM_CHUNK - 1) / MM_CHUNK), pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    hipLaunchKernelGGL(k_copy_maps, grid, dim3(NT), 0, st, in, out, pairs, out_stride, n);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// ---- FillImageNew ------------------------------------------------------------------------------------------------
// k_fin_search  one workgroup per row: the row (W <= FIN_LDS_W; longer rows are probed in global memory) and the next
//               row's first byte; per hole fin_search; the pushed values of the row compacted in hole order into
//               pv[r * W ..]; the row's hole and push counts
// k_fin_scan    one workgroup per map: exclusive scans of both counts over the H rows (H + 1 entries each), counts
// k_fin_gather  one workgroup per row: hole number i of the map takes push number i -- its own where no push is missing
//               in front of the row or inside it, else found by fin_find_row and the offset inside that row
constexpr int FIN_LDS_W = 16384;

// ranks of the set flags below this thread in the workgroup and the workgroup's totals, for two flags at once
__device__ __forceinline__ void fin_block_ranks(bool f0, bool f1, int (*ws)[NT / WAVE], int &r0, int &r1, int &t0, int &t1)
{
    const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) { ws[0][wave] = __popcll(b0); ws[1][wave] = __popcll(b1); }
    __syncthreads();
    r0 = __popcll(b0 & below); r1 = __popcll(b1 & below); t0 = 0; t1 = 0;
#pragma unroll
    for (int w = 0; w < NT / WAVE; w++) {
        const int c0 = ws[0][w], c1 = ws[1][w];
        if (w < wave) { r0 += c0; r1 += c1; }
        t0 += c0; t1 += c1;
    }
    __syncthreads();                                              // ws reused by the next chunk
}

__global__ void __launch_bounds__(NT) k_fin_search(const uint8_t *__restrict__ maps, int pairs, size_t stride, int H, int W,
                                                   int fix, uint8_t *__restrict__ pv, int *__restrict__ rowcnt)
{
    __shared__ uint8_t srow[FIN_LDS_W];
    __shared__ int ws[2][NT / WAVE];
    const int r = blockIdx.x;
    const size_t n = (size_t)H * W;
    const bool lds = W <= FIN_LDS_W;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const uint8_t *g = maps + (size_t)b * stride + (size_t)r * W;
        if (lds) {
            for (int i = threadIdx.x; i < W; i += NT) srow[i] = g[i];
            __syncthreads();
        }
        const int row_end = r + 1 < H ? g[W] : 0;                 // (H - 1, W) reads as 0
        uint8_t *pr = pv + (size_t)b * n + (size_t)r * W;
        int hbase = 0, pbase = 0;
        for (int c0 = 0; c0 < W; c0 += NT) {
            const int c = c0 + threadIdx.x;
            int val = 0;
            bool hole = false, pushed = false;
            if (c < W) {
                if (lds) { hole = srow[c] == 0; if (hole) pushed = fin_search(srow, W, c, row_end, fix, &val) != 0; }
                else { hole = g[c] == 0; if (hole) pushed = fin_search(g, W, c, row_end, fix, &val) != 0; }
            }
            int rh, rp, th, tp;
            fin_block_ranks(hole, pushed, ws, rh, rp, th, tp);
            if (pushed) pr[pbase + rp] = (uint8_t)val;
            hbase += th; pbase += tp;
        }
        if (threadIdx.x == 0) {
            rowcnt[2 * ((size_t)b * H + r)] = hbase;
            rowcnt[2 * ((size_t)b * H + r) + 1] = pbase;
        }
        __syncthreads();                                          // srow reused by the next pair
    }
}

__global__ void __launch_bounds__(NT) k_fin_scan(const int *__restrict__ rowcnt, int H, int *__restrict__ hp,
                                                 int *__restrict__ pp, int *__restrict__ counts)
{
    __shared__ int ws[2][NT / WAVE];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int *rc = rowcnt + 2 * (size_t)b * H;
    int *hb = hp + (size_t)b * (H + 1), *pb = pp + (size_t)b * (H + 1);
    int hcar = 0, pcar = 0;
    for (int r0 = 0; r0 < H; r0 += NT) {
        const int r = r0 + threadIdx.x;
        const int h = r < H ? rc[2 * r] : 0, p = r < H ? rc[2 * r + 1] : 0;
        int hs = h, ps = p;                                       // inclusive scans inside the wave
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int hy = __shfl_up(hs, off, WAVE), py = __shfl_up(ps, off, WAVE);
            if (lane >= off) { hs += hy; ps += py; }
        }
        if (lane == WAVE - 1) { ws[0][wave] = hs; ws[1][wave] = ps; }
        __syncthreads();
        int hw = 0, pw = 0, ht = 0, pt = 0;
#pragma unroll
        for (int w = 0; w < NT / WAVE; w++) {
            if (w < wave) { hw += ws[0][w]; pw += ws[1][w]; }
            ht += ws[0][w]; pt += ws[1][w];
        }
        if (r < H) { hb[r] = hcar + hw + hs - h; pb[r] = pcar + pw + ps - p; }
        hcar += ht; pcar += pt;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hb[H] = hcar; pb[H] = pcar;
        if (counts) { counts[2 * b] = hcar - pcar; counts[2 * b + 1] = hcar - pcar; }
    }
}

__global__ void __launch_bounds__(NT) k_fin_gather(uint8_t *maps, int pairs, size_t stride, int H, int W,
                                                   const uint8_t *__restrict__ pv, const int *__restrict__ hp,
                                                   const int *__restrict__ pp)
{
    __shared__ int ws[2][NT / WAVE];
    const int r = blockIdx.x;
    const size_t n = (size_t)H * W;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const int *hb = hp + (size_t)b * (H + 1), *pb = pp + (size_t)b * (H + 1);
        const int h0 = hb[r], nh = hb[r + 1] - h0, p0 = pb[r], np = pb[r + 1] - p0, total = pb[H];
        if (nh == 0) continue;                                    // uniform over the workgroup
        const bool own = h0 == p0 && nh == np;                    // no push missing in front of the row or inside it
        uint8_t *g = maps + (size_t)b * stride + (size_t)r * W;
        const uint8_t *pvb = pv + (size_t)b * n;
        int hbase = 0;
        for (int c0 = 0; c0 < W; c0 += NT) {
            const int c = c0 + threadIdx.x;
            const bool hole = c < W && g[c] == 0;
            int rh, r1, th, t1;
            fin_block_ranks(hole, false, ws, rh, r1, th, t1);
            if (hole) {
                const int i = h0 + hbase + rh;                    // the hole's number in raster order
                if (own) g[c] = pvb[(size_t)r * W + hbase + rh];
                else if (i < total) {                             // at or past the list's length: keeps 0
                    const int r2 = fin_find_row(pb, H, i);
                    g[c] = pvb[(size_t)r2 * W + (i - pb[r2])];
                }
            }
            hbase += th;
        }
    }
}

size_t fill_scratch_bytes(int pairs, int H, int W)
{
    return up256((size_t)pairs * H * W) + up256((size_t)pairs * H * 8) + 2 * up256((size_t)pairs * (H + 1) * 4);
}
int fill_enqueue(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts, void *scratch, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    if (stride == 0) stride = n;
    uint8_t *pv = (uint8_t *)scratch;
    int *rowcnt = (int *)(pv + up256((size_t)pairs * n));
    int *hp = (int *)((uint8_t *)rowcnt + up256((size_t)pairs * H * 8));
    int *pp = (int *)((uint8_t *)hp + up256((size_t)pairs * (H + 1) * 4));
    const dim3 grid((unsigned)H, pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    hipLaunchKernelGGL(k_fin_search, grid, dim3(NT), 0, st, (const uint8_t *)maps, pairs, stride, H, W,
                       (int)(fix & SMT_ASW_FIX_FILL_ROW_END), pv, rowcnt);
    hipLaunchKernelGGL(k_fin_scan, dim3(pairs), dim3(NT), 0, st, (const int *)rowcnt, H, hp, pp, counts);
    hipLaunchKernelGGL(k_fin_gather, grid, dim3(NT), 0, st, maps, pairs, stride, H, W, (const uint8_t *)pv, (const int *)hp,
                       (const int *)pp);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

int post_check(const smt_asw_post_params &P)
{
    if ((P.median_first != 3 && P.median_first != 5) || (P.median_last != 3 && P.median_last != 5)) return SMT_ERR_ARG;
    if (P.fix & ~(unsigned)SMT_ASW_FIX_FILL_ROW_END) return SMT_ERR_ARG;
    return SMT_OK;
}

// scratch of one call, handed back to the arena in stream order when the call returns
struct scratch_block {
    void *p = nullptr;
    hipStream_t st;
    explicit scratch_block(hipStream_t s) : st(s) {}
    int get(size_t bytes)
    {
        const hipError_t e = smt_scratch_alloc(&p, bytes, st);
        if (e != hipSuccess) { g_smt_last_hip = (int)e; p = nullptr; return SMT_ERR_ALLOC; }
        return SMT_OK;
    }
    ~scratch_block() { if (p) smt_scratch_free(p, st); }
};

}  // namespace

SMT_API void smt_asw_post_default_params(smt_asw_post_params *p)
{
    if (!p) return;
    p->speckle_newval = 0; p->speckle_max_size = 40; p->speckle_max_diff = 2;      // ASWeight.cpp:73
    p->median_first = 5; p->median_last = 3;                                       // :74, :78
    p->fix = 0;
}

SMT_API int smt_minmax_normalize_u8_batch(const uint8_t *in, uint8_t *out, int pairs, size_t stride, int H, int W, void *stream)
{
    int rc = tail_check(in, out, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    hipStream_t st = smt_stream(stream);
    scratch_block s(st);
    if ((rc = s.get(normalize_scratch_bytes(pairs))) != SMT_OK) return rc;
    return normalize_enqueue<uint8_t>(in, out, pairs, stride, H, W, s.p, st);
}

SMT_API int smt_minmax_normalize_f32_u8_batch(const float *in, uint8_t *out, int pairs, size_t stride, int H, int W,
                                              void *stream)
{
    int rc = tail_check(in, out, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    hipStream_t st = smt_stream(stream);
    scratch_block s(st);
    if ((rc = s.get(normalize_scratch_bytes(pairs))) != SMT_OK) return rc;
    return normalize_enqueue<float>(in, out, pairs, stride, H, W, s.p, st);
}

SMT_API int smt_median_blur_u8_batch(const uint8_t *in, uint8_t *out, int pairs, size_t stride, int W, int H, int ksize,
                                     void *stream)
{
    int rc = tail_check(in, out, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    if (in == out || (ksize != 3 && ksize != 5)) return SMT_ERR_ARG;
    return median_blur_enqueue(in, out, pairs, stride, stride, W, H, ksize, smt_stream(stream));
}

SMT_API int smt_fill_image_new_batch(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts,
                                     void *stream)
{
    int rc = tail_check(maps, maps, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    if (W > 65535 || (fix & ~(unsigned)SMT_ASW_FIX_FILL_ROW_END)) return SMT_ERR_ARG;
    hipStream_t st = smt_stream(stream);
    scratch_block s(st);
    if ((rc = s.get(fill_scratch_bytes(pairs, H, W))) != SMT_OK) return rc;
    return fill_enqueue(maps, pairs, stride, H, W, fix, counts, s.p, st);
}

// The same three steps on host memory through fill_image_rules.h.  No read outside a map: the byte at (H - 1, W) is 0.
SMT_API int smt_fill_image_new_host(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts)
{
    int rc = tail_check(maps, maps, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    if (W > 65535 || (fix & ~(unsigned)SMT_ASW_FIX_FILL_ROW_END)) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    if (stride == 0) stride = n;
    try {
        std::vector<uint8_t> pv(n);
        std::vector<int> hp((size_t)H + 1), pp((size_t)H + 1);
        for (int b = 0; b < pairs; b++) {
            uint8_t *m = maps + (size_t)b * stride;
            hp[0] = pp[0] = 0;
            for (int r = 0; r < H; r++) {                                            // k_fin_search, k_fin_scan
                const uint8_t *row = m + (size_t)r * W;
                const int row_end = r + 1 < H ? row[W] : 0;
                int nh = 0, np = 0;
                for (int c = 0; c < W; c++) {
                    if (row[c]) continue;
                    int val = 0;
                    nh++;
                    if (fin_search(row, W, c, row_end, (int)(fix & SMT_ASW_FIX_FILL_ROW_END), &val))
                        pv[(size_t)r * W + np++] = (uint8_t)val;
                }
                hp[r + 1] = hp[r] + nh; pp[r + 1] = pp[r] + np;
            }
            const int total = pp[H];
            for (int r = 0; r < H; r++) {                                            // k_fin_gather
                uint8_t *row = m + (size_t)r * W;
                const bool own = hp[r] == pp[r] && hp[r + 1] - hp[r] == pp[r + 1] - pp[r];
                int rank = 0;
                for (int c = 0; c < W; c++) {
                    if (row[c]) continue;
                    const int i = hp[r] + rank;
                    if (own) row[c] = pv[(size_t)r * W + rank];
                    else if (i < total) {
                        const int r2 = fin_find_row(pp.data(), H, i);
                        row[c] = pv[(size_t)r2 * W + (i - pp[r2])];
                    }
                    rank++;
                }
            }
            if (counts) { counts[2 * b] = hp[H] - pp[H]; counts[2 * b + 1] = hp[H] - pp[H]; }
        }
    } catch (const std::bad_alloc &) {
        return SMT_ERR_ALLOC;
    }
    return SMT_OK;
}

SMT_API int smt_asw_tail_batch(uint8_t *lastDisp, int pairs, size_t stride, int H, int W, const smt_asw_post_params *post,
                               uint8_t *after_median, uint8_t *after_fill, int *fill_counts, int *err_dev, void *stream)
{
    if (pairs == 0 && lastDisp) return SMT_OK;
    int rc = tail_check(lastDisp, lastDisp, pairs, stride, H, W);
    if (rc != SMT_OK) return rc;
    smt_asw_post_params P;
    if (post) P = *post; else smt_asw_post_default_params(&P);
    if ((rc = post_check(P)) != SMT_OK || W > 65535) return SMT_ERR_ARG;
    const size_t n = (size_t)H * W;
    hipStream_t st = smt_stream(stream);
    // tmp: the dense maps between the two medians; behind it the stage scratch, one stage at a time in stream order
    size_t stage = normalize_scratch_bytes(pairs);
    if (smt_speckle_scratch_bytes(pairs, W, H) > stage) stage = smt_speckle_scratch_bytes(pairs, W, H);
    if (fill_scratch_bytes(pairs, H, W) > stage) stage = fill_scratch_bytes(pairs, H, W);
    scratch_block s(st);
    if ((rc = s.get(up256((size_t)pairs * n) + stage)) != SMT_OK) return rc;
    uint8_t *tmp = (uint8_t *)s.p;
    void *sc = tmp + up256((size_t)pairs * n);
    const size_t pitch = stride ? stride : n;
    rc = normalize_enqueue<uint8_t>(lastDisp, lastDisp, pairs, stride, H, W, sc, st);                        // :69, :72
    if (rc == SMT_OK) rc = smt_speckle_u8_enqueue(lastDisp, pairs, stride, W, H, P.speckle_newval, P.speckle_max_size,
                                                  P.speckle_max_diff, sc, err_dev, st);                      // :73
    if (rc == SMT_OK) rc = median_blur_enqueue(lastDisp, tmp, pairs, stride, 0, W, H, P.median_first, st);   // :74
    if (rc == SMT_OK && after_median) rc = copy_maps_enqueue(tmp, after_median, pairs, pitch, n, st);        // speckle.png
    if (rc == SMT_OK) rc = fill_enqueue(tmp, pairs, 0, H, W, P.fix, fill_counts, sc, st);                    // :76
    if (rc == SMT_OK && after_fill) rc = copy_maps_enqueue(tmp, after_fill, pairs, pitch, n, st);            // filled.png
    if (rc == SMT_OK) rc = median_blur_enqueue(tmp, lastDisp, pairs, 0, stride, W, H, P.median_last, st);    // :78
    return rc;
}

// Host only: both selection networks of csrc/median_net.h on every input of zeros and ones (min = and, max = or, 64
// inputs per word).
SMT_API int smt_median_blur_selftest_nets(void)
{
    struct ops {
        static unsigned long long mn(unsigned long long a, unsigned long long b) { return a & b; }
        static unsigned long long mx(unsigned long long a, unsigned long long b) { return a | b; }
    };
    const unsigned long long low[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                       0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    for (int N = 9; N <= 25; N += 16) {
        for (unsigned hi = 0; hi < (1u << (N - 6)); hi++) {
            unsigned long long p[25], in[25];
            for (int i = 0; i < N; i++) in[i] = p[i] = i < 6 ? low[i] : (((hi >> (i - 6)) & 1) ? ~0ull : 0ull);
            if (N == 9) mednet_run<9>(p, ops::mn, ops::mx); else mednet_run<25>(p, ops::mn, ops::mx);
            // the median of zeros and ones is 1 iff more than half are ones: a bit-sliced counter of the ones
            unsigned long long cnt[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < N; i++) {
                unsigned long long carry = in[i];
                for (int k = 0; k < 5; k++) { const unsigned long long t = cnt[k] & carry; cnt[k] ^= carry; carry = t; }
            }
            unsigned long long ge = 0;                             // count >= N / 2 + 1, per bit position
            for (int bit = 0; bit < 64; bit++) {
                int c = 0;
                for (int k = 0; k < 5; k++) c |= (int)((cnt[k] >> bit) & 1) << k;
                if (c >= N / 2 + 1) ge |= 1ull << bit;
            }
            if (ge != p[N / 2]) return SMT_ERR_STATE;
        }
    }
    return SMT_OK;
}
