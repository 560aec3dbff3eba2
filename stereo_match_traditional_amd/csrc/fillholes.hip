// SAD/Sad.h's in-place FillHolesInDispMap, batched (include/smt_fill_holes.h, csrc/fillholes_rule.h, DESIGN.md section
// 5.21).
//
// The reference writes into the map it reads: a target sees the fills of every target before it in raster order.  On
// the device that recurrence runs as a wavefront.  Pixel (i, j) of a pass has step 2 i + j; a step first reads (every
// target of the step walks its eight rays and chooses), then synchronises, then writes.  That is the sequential result
// because of what a ray can touch: every pixel on a ray of (i, j) that comes EARLIER in raster order has a strictly
// smaller step, so its fill has been written, and every LATER one has an equal or larger step, so it still holds the
// value the sequential loop would read.  (An up-right ray climbs at least as many rows as it crosses columns and a
// down-left ray descends at least one row for every two columns once it has left its row; tests/test_fill_holes_cpu.py
// checks the property through this library's own probe function.  With step i + j it fails.)
//
// One workgroup owns one map and runs the three passes on it, so the only synchronisation is the workgroup barrier, and
// a call is one launch with the pairs on the grid.  The rows that have a pixel at step s are lo..hi, at most
// ceil(W / 2) + 1 of them, one per thread; where that is more than the workgroup they run in ascending groups of
// blockDim.x rows, each group reading, synchronising and writing before the next (a group's rays touch rows above
// it only at smaller steps, so ascending order keeps the property).  Pass 2 needs no list: a pixel is its target iff it
// is == invalid when its step comes (fillholes_rule.h, is_target).
//
// A thread whose pixel is not a target does nothing; a step on which no thread of the workgroup has a target costs one
// barrier (__syncthreads_or) instead of two.  The eight ray states are registers (fhrule::collect is unrolled over the
// rays, which advance together so that their loads are in flight side by side).  No LDS staging: see DESIGN.md.
#include "smt_common.h"
#include "../../include/smt_fill_holes.h"
#include "fillholes_rule.h"
#include <stdlib.h>
#include <string.h>

namespace fh = fhrule;

namespace {

constexpr int FH_MAX_THREADS = 1024;

__global__ __launch_bounds__(FH_MAX_THREADS) void k_fill_holes(float *maps, size_t mstride, const uint8_t *clsmaps,
                                                               size_t cstride, int H, int W, float invalid, int *status)
{
    __shared__ int s_cnt[4];                                     // n_occ, n_mis, n_third, NaN seen
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    float *M = maps + blockIdx.x * mstride;
    const uint8_t *cls = clsmaps + blockIdx.x * cstride;
    const int N = H * W;
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    {
        int c1 = 0, c2 = 0, nan = 0;
        for (int idx = tid; idx < N; idx += T) {
            const float v = M[idx];
            const uint8_t c = cls[idx];
            nan |= v != v;
            c1 += c == 1;
            c2 += c == 2;
        }
        if (c1) atomicAdd(&s_cnt[0], c1);
        if (c2) atomicAdd(&s_cnt[1], c2);
        if (nan) atomicOr(&s_cnt[3], 1);
    }
    __syncthreads();
    const bool ub = s_cnt[3] != 0;                               // workgroup-uniform
    int third = 0;
    if (!ub) {
        const int S = (int)fh::steps(H, W);
        for (int pass = 0; pass < 3; pass++) {
            for (int s = 0; s < S; s++) {
                // rows with a pixel at this step: 0 <= s - 2 i <= W - 1
                const int lo = s - W + 1 > 0 ? (s - W + 2) >> 1 : 0;
                const int hi = min(H - 1, s >> 1);
                for (int base = lo; base <= hi; base += T) {
                    const int i = base + tid;
                    bool fill = false;
                    float value = 0.0f;
                    int at = 0;
                    if (i <= hi) {
                        const int j = s - fh::SKEW * i;
                        at = i * W + j;
                        const bool target = pass == 2 ? fh::is_target(2, 0, M[at], invalid)
                                                      : fh::is_target(pass, cls[at], 0.0f, invalid);
                        if (target) {
                            third += pass == 2;
                            float v[fh::RAYS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                            const unsigned has = fh::collect(M, H, W, i, j, invalid, v);
                            if (has) {
                                fill = true;
                                value = fh::choose(v, has, pass);
                            }
                        }
                    }
                    if (__syncthreads_or(fill)) {                // every read of the group is done
                        if (fill) M[at] = value;
                        __syncthreads();                         // every write is visible to the next group's reads
                    }
                }
            }
            __syncthreads();
        }
        if (third) atomicAdd(&s_cnt[2], third);
        __syncthreads();
    }
    if (status && tid == 0) {
        int *st = status + 4 * (size_t)blockIdx.x;
        st[0] = s_cnt[0];
        st[1] = s_cnt[1];
        st[2] = s_cnt[2];
        st[3] = ub ? SMT_FILLHOLES_UB_NAN : 0;
    }
}

// arguments -> SMT_ERR_ARG or SMT_OK, strides resolved (0 -> H*W)
int fill_holes_check(const float *maps, const uint8_t *cls, int pairs, size_t &map_stride, size_t &cls_stride, int H, int W,
                     float invalid)
{
    if (!maps || !cls || pairs < 0) return SMT_ERR_ARG;
    if (H <= 0 || W <= 0 || H > SMT_FILLHOLES_MAX_DIM || W > SMT_FILLHOLES_MAX_DIM) return SMT_ERR_ARG;
    if (invalid != invalid) return SMT_ERR_ARG;
    const size_t N = (size_t)H * W;
    for (size_t *s : {&map_stride, &cls_stride}) {
        if (*s == 0) *s = N;
        if (*s < N) return SMT_ERR_ARG;
    }
    return SMT_OK;
}

// ---- host twin: the raster-order loops of Sad.h:333-399 through fillholes_rule.h ------------------------------------
void fill_holes_host_one(float *M, const uint8_t *cls, int H, int W, float invalid, int *st, int passes = 3)
{
    const size_t N = (size_t)H * W;
    st[0] = st[1] = st[2] = st[3] = 0;
    for (size_t x = 0; x < N; x++) {
        st[0] += cls[x] == 1;
        st[1] += cls[x] == 2;
        if (M[x] != M[x]) st[3] = SMT_FILLHOLES_UB_NAN;
    }
    if (st[3]) return;
    for (int pass = 0; pass < passes; pass++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t at = (size_t)y * W + x;
                if (!fh::is_target(pass, cls[at], M[at], invalid)) continue;
                st[2] += pass == 2;
                float v[fh::RAYS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                const unsigned has = fh::collect(M, H, W, y, x, invalid, v);
                if (has) M[at] = fh::choose(v, has, pass);
            }
}

}  // namespace

SMT_API int smt_fill_holes_batch(float *maps, const uint8_t *cls, int pairs, size_t map_stride, size_t cls_stride, int H,
                                 int W, float invalid, int *status, void *stream)
{
    const int rc = fill_holes_check(maps, cls, pairs, map_stride, cls_stride, H, W, invalid);
    if (rc != SMT_OK || pairs == 0) return rc;
    // one thread per row that can have a pixel at a step, in whole waves
    int T = (((W + 1) / 2 + 1 + WAVE - 1) / WAVE) * WAVE;
    if (T > H) T = ((H + WAVE - 1) / WAVE) * WAVE;
    if (T > FH_MAX_THREADS) T = FH_MAX_THREADS;
    hipLaunchKernelGGL(k_fill_holes, dim3((unsigned)pairs), dim3((unsigned)T), 0, smt_stream(stream), maps, map_stride, cls,
                       cls_stride, H, W, invalid, status);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_fill_holes_batch_host(float *maps, const uint8_t *cls, int pairs, size_t map_stride, size_t cls_stride,
                                      int H, int W, float invalid, int *status)
{
    const int rc = fill_holes_check(maps, cls, pairs, map_stride, cls_stride, H, W, invalid);
    if (rc != SMT_OK) return rc;
    for (int p = 0; p < pairs; p++) {
        int st[4];
        fill_holes_host_one(maps + p * map_stride, cls + p * cls_stride, H, W, invalid, st);
        if (status) memcpy(status + 4 * (size_t)p, st, sizeof(st));
    }
    return SMT_OK;
}

SMT_API void smt_fill_holes_constants(float *out16)
{
    if (!out16) return;
    for (int r = 0; r < fh::RAYS; r++) {
        out16[r] = fh::sina(r);
        out16[fh::RAYS + r] = fh::cosa(r);
    }
}

SMT_API int smt_fill_holes_probe(int y, int x, int ray, int n, int *yy, int *xx)
{
    if (ray < 0 || ray >= fh::RAYS || n < 1 || !yy || !xx) return SMT_ERR_ARG;
    *yy = fh::probe(y, n, fh::sina(ray));
    *xx = fh::probe(x, n, fh::cosa(ray));
    return SMT_OK;
}

SMT_API int smt_fill_holes_walk(int H, int W, int y, int x, int ray, int *yy, int *xx, int cap)
{
    if (H <= 0 || W <= 0 || ray < 0 || ray >= fh::RAYS || cap < 0 || (cap > 0 && (!yy || !xx))) return SMT_ERR_ARG;
    int count = 0;
    for (int n = 1;; n++) {
        const int py = fh::probe(y, n, fh::sina(ray)), px = fh::probe(x, n, fh::cosa(ray));
        if (fh::outside(py, px, H, W)) return count;
        if (count >= cap) return SMT_ERR_ARG;
        yy[count] = py;
        xx[count] = px;
        count++;
    }
}

SMT_API int smt_fill_holes_host_passes(float *map, const uint8_t *cls, int H, int W, float invalid, int passes)
{
    size_t ms = 0, cs = 0;
    const int rc = fill_holes_check(map, cls, 1, ms, cs, H, W, invalid);
    if (rc != SMT_OK || passes < 0 || passes > 3) return SMT_ERR_ARG;
    int st[4];
    fill_holes_host_one(map, cls, H, W, invalid, st, passes);
    return SMT_OK;
}
