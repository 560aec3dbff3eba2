// RemoveSpeckles (AD-CensusV1/PostProcessing.h:250-311) for a batch of maps, asynchronous, in four launches whatever
// the data and the pair count.  The relation `a != inv && b != inv && fabsf(b - a) <= diff` is
// symmetric, so the reference's scan-order BFS computes the connected components of an 8-connected graph; this is
// connected-component labelling by union-find over 32 x 32 tiles:
//   k_sp_tile   one workgroup per tile: union-find in LDS over the tile's own 8-neighbour links; every pixel gets the
//               tile-local index of its local root (loc), every pixel's forest slot points to itself (par), counts 0
//   k_sp_merge  one thread per tile-border pixel: the links whose other end lies in another tile (right, below and the
//               two diagonals, corners included) unite the two local roots in the global forest par
//   k_sp_count  per tile: pixels counted per local root in LDS, one global atomic add per local root into its global
//               root; every local root's forest slot is left pointing at its global root
//   k_sp_apply  a pixel whose global root has fewer than min_area pixels becomes inv
// Cross-workgroup visibility: inside k_sp_merge and k_sp_count the forest is written by other workgroups, possibly on
// other XCDs, whose L2s are not coherent with each other: every read of par there is an agent-scope atomic load, every
// write an agent-scope atomic min.  Between launches plain loads see everything.
// Loop caps: a parent is never larger than its child, so a find walks at most n slots and every round of a union
// lowers the larger of its two roots; caps of n + 1 are above both.  A cap reached sets *err (never expected).
#include "smt_common.h"
#include <new>

namespace {

constexpr int TS = 32, TN = TS * TS;  // tile side; tile-local index k = r * TS + c
constexpr int NT_TILE = 256;          // 4 pixels per thread
constexpr int NT_MERGE = 128;         // >= 3 * TS - 2 border slots
constexpr int MAX_GRID_Y = 65535;

__device__ __forceinline__ bool sp_linked(float a, float b, float inv, float diff)
{
    return a != inv && b != inv && fabsf(b - a) <= diff;                  // :290-292
}
// filterSpeckles on CV_8UC1 (smt_filter_speckles_u8_batch): the pixels, newVal and maxDiff as ints
__device__ __forceinline__ bool sp_linked(int a, int b, int inv, int diff)
{
    return a != inv && b != inv && abs(b - a) <= diff;
}

// Union-find on `lab` with parent <= child.  SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for the LDS forest,
// __HIP_MEMORY_SCOPE_AGENT for the global one.  find halves the path it walks (atomic min: a slot only ever goes
// down, to an ancestor); union hooks the larger root under the smaller and, when the larger one was hooked
// elsewhere in the meantime, goes on with the slot it now has (Playne & Hawick 2018).
template <int SCOPE>
__device__ __forceinline__ int uf_find(int *lab, int x, unsigned cap, bool &bad)
{
    for (unsigned it = 0; it < cap; it++) {
        const int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        const int g = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, SCOPE);
        if (g == p) return p;
        __hip_atomic_fetch_min(lab + x, g, __ATOMIC_RELAXED, SCOPE);
        x = g;
    }
    bad = true;
    return x;
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(int *lab, int a, int b, unsigned cap, bool &bad)
{
    for (unsigned it = 0; it < cap; it++) {
        a = uf_find<SCOPE>(lab, a, cap, bad);
        b = uf_find<SCOPE>(lab, b, cap, bad);
        if (bad || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
    bad = true;
}

}  // namespace

// Border slot s of a th x tw tile -> the tile-local pixel (r, c) whose forward neighbours (right, below-left, below,
// below-right) it examines: the last column (th slots), the last row but its last pixel (tw - 1), the first column but
// its last pixel when it is not also the last column (th - 1).  Every other pixel's forward neighbours lie in its own
// tile.  Shared by k_sp_merge and smt_speckle_selftest_tiles.
__host__ __device__ static inline bool sp_border_slot(int s, int th, int tw, int &r, int &c)
{
    if (s < 0) return false;
    if (s < th) { r = s; c = tw - 1; return true; }
    s -= th;
    if (s < tw - 1) { r = th - 1; c = s; return true; }
    s -= tw - 1;
    if (tw > 1 && s < th - 1) { r = s; c = 0; return true; }
    return false;
}
__host__ __device__ static inline int sp_fwd_dy(int k) { return k == 0 ? 0 : 1; }   // right, below-left, below, below-right
__host__ __device__ static inline int sp_fwd_dx(int k) { return k == 0 ? 1 : k - 2; }

namespace {

// T = the pixel type, V = the type it is compared in (float / float for RemoveSpeckles, uint8_t / int for filterSpeckles),
// NB = 8 or 4 neighbours.
template <class T, class V, int NB>
__global__ void __launch_bounds__(NT_TILE) k_sp_tile(const T *__restrict__ d, int pairs, size_t stride, int W, int H,
                                                     int ntx, V inv, V diff, int *__restrict__ par,
                                                     int *__restrict__ cnt, short *__restrict__ loc, int *err)
{
    __shared__ V v[TN];
    __shared__ int lab[TN];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    const size_t n = (size_t)H * W;
    bool bad = false;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const T *db = d + (size_t)b * stride;
        bool valid[TN / NT_TILE];
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            const int k = threadIdx.x + i * NT_TILE, r = k / TS, c = k % TS;
            const bool in = r < th && c < tw;
            const V x = in ? (V)db[(size_t)(y0 + r) * W + x0 + c] : (V)0;
            valid[i] = in && x != inv;
            v[k] = x;
            lab[k] = valid[i] ? k : -1;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            if (!valid[i]) continue;
            const int k = threadIdx.x + i * NT_TILE, r = k / TS, c = k % TS;
            const V x = v[k];
            // backward neighbours: left, above-left, above, above-right (each in-tile link once; NB == 4: no diagonals)
            if (c > 0 && sp_linked(x, v[k - 1], inv, diff)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, k, k - 1, TN + 1, bad);
            if (r > 0) {
                if (NB == 8 && c > 0 && sp_linked(x, v[k - TS - 1], inv, diff)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, k, k - TS - 1, TN + 1, bad);
                if (sp_linked(x, v[k - TS], inv, diff)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, k, k - TS, TN + 1, bad);
                if (NB == 8 && c + 1 < tw && sp_linked(x, v[k - TS + 1], inv, diff)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, k, k - TS + 1, TN + 1, bad);
            }
        }
        __syncthreads();
        int *pb = par + (size_t)b * n, *cb = cnt + (size_t)b * n;
        short *lb = loc + (size_t)b * n;
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            const int k = threadIdx.x + i * NT_TILE, r = k / TS, c = k % TS;
            if (r >= th || c >= tw) continue;
            const int g = (y0 + r) * W + x0 + c;
            lb[g] = valid[i] ? (short)uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, k, TN + 1, bad) : (short)-1;
            pb[g] = g;
            cb[g] = 0;
        }
        __syncthreads();                                                    // LDS reused by the next pair
    }
    if (bad && err) *err = 1;
}

template <class T, class V, int NB>
__global__ void __launch_bounds__(NT_MERGE) k_sp_merge(const T *__restrict__ d, int pairs, size_t stride, int W,
                                                       int H, int ntx, V inv, V diff, int *par,
                                                       const short *__restrict__ loc, int *err)
{
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    int r, c;
    if (!sp_border_slot(threadIdx.x, th, tw, r, c)) return;
    const size_t n = (size_t)H * W;
    const unsigned cap = (unsigned)n + 1u;
    const int y = y0 + r, x = x0 + c, p = y * W + x;
    bool bad = false;
    for (int b = blockIdx.y; b < pairs && !bad; b += gridDim.y) {
        const T *db = d + (size_t)b * stride;
        const short *lb = loc + (size_t)b * n;
        int *pb = par + (size_t)b * n;
        const V dp = (V)db[p];
        if (dp == inv) continue;
        const int rp = (y0 + lb[p] / TS) * W + x0 + lb[p] % TS;             // p's local root
        for (int k = 0; k < 4; k++) {
            if (NB == 4 && (k & 1)) continue;                               // the two diagonals
            const int rr = r + sp_fwd_dy(k), cc = c + sp_fwd_dx(k);
            if (rr < th && cc >= 0 && cc < tw) continue;                    // same tile: k_sp_tile's link
            const int yy = y + sp_fwd_dy(k), xx = x + sp_fwd_dx(k);
            if (yy >= H || xx < 0 || xx >= W) continue;
            const int q = yy * W + xx;
            if (!sp_linked(dp, (V)db[q], inv, diff)) continue;
            const int lq = lb[q];
            const int qy0 = yy & ~(TS - 1), qx0 = xx & ~(TS - 1);
            uf_union<__HIP_MEMORY_SCOPE_AGENT>(pb, rp, (qy0 + lq / TS) * W + qx0 + lq % TS, cap, bad);
        }
    }
    if (bad && err) *err = 1;
}

__global__ void __launch_bounds__(NT_TILE) k_sp_count(int pairs, int W, int H, int ntx, int *par, int *cnt,
                                                      const short *__restrict__ loc, int *err)
{
    __shared__ int lc[TN];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    const size_t n = (size_t)H * W;
    const unsigned cap = (unsigned)n + 1u;
    bool bad = false;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        const short *lb = loc + (size_t)b * n;
        int *pb = par + (size_t)b * n, *cb = cnt + (size_t)b * n;
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) lc[threadIdx.x + i * NT_TILE] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            const int k = threadIdx.x + i * NT_TILE, r = k / TS, c = k % TS;
            if (r >= th || c >= tw) continue;
            const int l = lb[(y0 + r) * W + x0 + c];
            if (l >= 0) atomicAdd(&lc[l], 1);
        }
        __syncthreads();
        // one global add per local root (its pixel count); the add never overflows: a map has fewer than 2^31 pixels
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            const int k = threadIdx.x + i * NT_TILE, m = lc[k];
            if (m == 0) continue;
            const int g = (y0 + k / TS) * W + x0 + k % TS;
            const int root = uf_find<__HIP_MEMORY_SCOPE_AGENT>(pb, g, cap, bad);
            __hip_atomic_fetch_min(pb + g, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(cb + root, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                                                    // lc reused by the next pair
    }
    if (bad && err) *err = 1;
}

// LE: a component of at most min_area pixels goes (filterSpeckles' maxSpeckleSize), not one of fewer than min_area
template <class T, bool LE>
__global__ void __launch_bounds__(NT_TILE) k_sp_apply(T *d, int pairs, size_t stride, int W, int H, int ntx,
                                                      T inv, unsigned min_area, const int *__restrict__ par,
                                                      const int *__restrict__ cnt, const short *__restrict__ loc)
{
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * TS, x0 = tx * TS;
    const int th = min(TS, H - y0), tw = min(TS, W - x0);
    const size_t n = (size_t)H * W;
    for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
        T *db = d + (size_t)b * stride;
        const short *lb = loc + (size_t)b * n;
        const int *pb = par + (size_t)b * n, *cb = cnt + (size_t)b * n;
#pragma unroll
        for (int i = 0; i < TN / NT_TILE; i++) {
            const int k = threadIdx.x + i * NT_TILE, r = k / TS, c = k % TS;
            if (r >= th || c >= tw) continue;
            const int g = (y0 + r) * W + x0 + c, l = lb[g];
            if (l < 0) continue;
            const int root = pb[(y0 + l / TS) * W + x0 + l % TS];
            if (LE ? (unsigned)cb[root] <= min_area : (unsigned)cb[root] < min_area) db[g] = inv;   // :304-308
        }
    }
}

int speckle_check(const void *disp, int pairs, size_t stride, int W, int H)
{
    if (!disp || pairs <= 0 || W <= 0 || H <= 0) return SMT_ERR_ARG;
    if ((long long)H * W >= (1ll << 31)) return SMT_ERR_ARG;
    if (stride != 0 && stride < (size_t)H * W) return SMT_ERR_ARG;
    return SMT_OK;
}

}  // namespace

size_t smt_speckle_scratch_bytes(int pairs, int W, int H)
{
    return (size_t)pairs * H * W * (4 + 4 + 2);
}

int smt_speckle_enqueue(float *disp, int pairs, size_t stride, int W, int H, int diff_insame, unsigned min_speckle_area,
                        int invalid_val, void *scratch, int *err_dev, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    if (stride == 0) stride = n;
    int *par = (int *)scratch, *cnt = par + (size_t)pairs * n;
    short *loc = (short *)(cnt + (size_t)pairs * n);
    const float inv = (float)invalid_val, diff = (float)diff_insame;
    const int ntx = (W + TS - 1) / TS, nty = (H + TS - 1) / TS;
    const dim3 grid((unsigned)ntx * nty, pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    hipLaunchKernelGGL((k_sp_tile<float, float, 8>), grid, dim3(NT_TILE), 0, st, (const float *)disp, pairs, stride, W, H, ntx,
                       inv, diff, par, cnt, loc, err_dev);
    hipLaunchKernelGGL((k_sp_merge<float, float, 8>), grid, dim3(NT_MERGE), 0, st, (const float *)disp, pairs, stride, W, H,
                       ntx, inv, diff, par, loc, err_dev);
    hipLaunchKernelGGL(k_sp_count, grid, dim3(NT_TILE), 0, st, pairs, W, H, ntx, par, cnt, loc, err_dev);
    hipLaunchKernelGGL((k_sp_apply<float, false>), grid, dim3(NT_TILE), 0, st, disp, pairs, stride, W, H, ntx, inv,
                       min_speckle_area, par, cnt, loc);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on CV_8UC1 maps: the same four launches over the 4-neighbour
// graph, `<=` as the size test.  A newVal outside 0..255 equals no pixel; the pixels that go receive its low byte.
// A negative maxDiff links nothing, a negative maxSpeckleSize removes nothing.
int smt_speckle_u8_enqueue(uint8_t *maps, int pairs, size_t stride, int W, int H, int newVal, int maxSpeckleSize,
                           int maxDiff, void *scratch, int *err_dev, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    if (stride == 0) stride = n;
    int *par = (int *)scratch, *cnt = par + (size_t)pairs * n;
    short *loc = (short *)(cnt + (size_t)pairs * n);
    const int ntx = (W + TS - 1) / TS, nty = (H + TS - 1) / TS;
    const dim3 grid((unsigned)ntx * nty, pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y);
    hipLaunchKernelGGL((k_sp_tile<uint8_t, int, 4>), grid, dim3(NT_TILE), 0, st, (const uint8_t *)maps, pairs, stride, W, H,
                       ntx, newVal, maxDiff, par, cnt, loc, err_dev);
    hipLaunchKernelGGL((k_sp_merge<uint8_t, int, 4>), grid, dim3(NT_MERGE), 0, st, (const uint8_t *)maps, pairs, stride, W, H,
                       ntx, newVal, maxDiff, par, loc, err_dev);
    hipLaunchKernelGGL(k_sp_count, grid, dim3(NT_TILE), 0, st, pairs, W, H, ntx, par, cnt, loc, err_dev);
    if (maxSpeckleSize >= 0)
        hipLaunchKernelGGL((k_sp_apply<uint8_t, true>), grid, dim3(NT_TILE), 0, st, maps, pairs, stride, W, H, ntx,
                           (uint8_t)newVal, (unsigned)maxSpeckleSize, par, cnt, loc);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_filter_speckles_u8_batch(uint8_t *maps, int pairs, size_t stride, int W, int H, int newVal,
                                         int maxSpeckleSize, int maxDiff, int *err_dev, void *stream)
{
    int rc = speckle_check(maps, pairs, stride, W, H);
    if (rc != SMT_OK) return rc;
    if ((long long)H * W >= (1ll << 28)) return SMT_ERR_ARG;
    hipStream_t st = smt_stream(stream);
    void *scratch = nullptr;
    const hipError_t e = smt_scratch_alloc(&scratch, smt_speckle_scratch_bytes(pairs, W, H), st);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    rc = smt_speckle_u8_enqueue(maps, pairs, stride, W, H, newVal, maxSpeckleSize, maxDiff, scratch, err_dev, st);
    smt_scratch_free(scratch, st);
    return rc;
}

SMT_API int smt_remove_speckles_batch(float *disp, int pairs, size_t disp_stride, int W, int H, int diff_insame,
                                      unsigned min_speckle_area, int invalid_val, int *err_dev, void *stream)
{
    int rc = speckle_check(disp, pairs, disp_stride, W, H);
    if (rc != SMT_OK) return rc;
    hipStream_t st = smt_stream(stream);
    void *scratch = nullptr;
    const hipError_t e = smt_scratch_alloc(&scratch, smt_speckle_scratch_bytes(pairs, W, H), st);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    rc = smt_speckle_enqueue(disp, pairs, disp_stride, W, H, diff_insame, min_speckle_area, invalid_val, scratch, err_dev, st);
    smt_scratch_free(scratch, st);
    return rc;
}

// Host only: every 8-adjacent pixel pair of an H x W map whose two pixels lie in different tiles is examined by exactly
// one (tile, border slot, forward direction) of k_sp_merge, and no slot examines a pair inside one tile.
SMT_API int smt_speckle_selftest_tiles(int H, int W)
{
    if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 28)) return SMT_ERR_ARG;
    const int ntx = (W + TS - 1) / TS, nty = (H + TS - 1) / TS;
    // hits[p * 4 + k]: pair (p, forward neighbour k of p)
    unsigned char *hits = new (std::nothrow) unsigned char[(size_t)H * W * 4]();
    if (!hits) return SMT_ERR_ALLOC;
    int rc = SMT_OK;
    for (int t = 0; t < ntx * nty && rc == SMT_OK; t++) {
        const int ty = t / ntx, tx = t - ty * ntx, y0 = ty * TS, x0 = tx * TS;
        const int th = H - y0 < TS ? H - y0 : TS, tw = W - x0 < TS ? W - x0 : TS;
        for (int s = 0; s < NT_MERGE && rc == SMT_OK; s++) {
            int r, c;
            if (!sp_border_slot(s, th, tw, r, c)) continue;
            if (r < 0 || r >= th || c < 0 || c >= tw) { rc = SMT_ERR_STATE; break; }
            for (int k = 0; k < 4; k++) {
                const int rr = r + sp_fwd_dy(k), cc = c + sp_fwd_dx(k);
                if (rr < th && cc >= 0 && cc < tw) continue;
                const int yy = y0 + rr, xx = x0 + cc;
                if (yy >= H || xx < 0 || xx >= W) continue;
                unsigned char &h = hits[((size_t)(y0 + r) * W + x0 + c) * 4 + k];
                if (h) { rc = SMT_ERR_STATE; break; }
                h = 1;
            }
        }
    }
    for (int y = 0; y < H && rc == SMT_OK; y++)
        for (int x = 0; x < W && rc == SMT_OK; x++)
            for (int k = 0; k < 4; k++) {
                const int yy = y + sp_fwd_dy(k), xx = x + sp_fwd_dx(k);
                const bool exists = yy < H && xx >= 0 && xx < W;
                const bool cross = exists && (yy / TS != y / TS || xx / TS != x / TS);
                if (cross != (hits[((size_t)y * W + x) * 4 + k] != 0)) { rc = SMT_ERR_STATE; break; }
            }
    delete[] hits;
    return rc;
}
