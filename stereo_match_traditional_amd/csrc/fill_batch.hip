// FillTheHole (AD-CensusV1/PostProcessing.h:156-248) for a batch of maps, with the lists LeftRightConsistency would
// have produced taken from the class maps on the device.  Asynchronous: one memset of the
// per-pair state and EIGHT kernel launches whatever the data and the pair count, no host synchronisation, scratch
// from the library's arena.  The pair is a grid axis; every launch reads the per-pair state and leaves flagged pairs
// and skipped passes alone.
//
//   k_fb_count      cls -> n_occ, n_mis, mid_0, mid_1 (a class-(k+1) pixel in image row col/2), out-of-buffer flag
//   k_fb_collect 0  one thread per ADDRESS a: the winner among the class-1 pixels (i, j) with i*row + j == a (largest
//   k_fb_apply   0  i; csrc/fill_rules.h) casts its 8 rays, the pick goes to fill[a]; apply writes fill[a] to disp[a]
//   k_fb_collect 1  the same for class 2 with the median rule
//   k_fb_apply   1
//   k_fb_holes      n_third = entries equal to 65535 after pass 1, mid_2 = one of them on line col/2
//   k_fb_collect 2  every hole, median rule, out of place into fill[]
//   k_fb_writeback  fill[a] -> disp[a] at the hole addresses only; writes the status
//
// Aliased targets (856 k of 2.0 M list entries on a 1080p LR map) are resolved before any ray is cast: the gather
// over addresses finds the one entry whose value survives, so a loser costs two byte loads and no atomics are needed.
// All writes of a pass come after all its reads (:241-246): collect only reads disp, apply only writes it.
//
// A collect workgroup looks at 256 addresses, one per thread.  Each wave ballots its targets, compacts them with one
// ds_permute and serves them eight at a time: 8 lanes per target, lane & 7 = ray, the pick by 8-wide shuffles.  On an
// LR map a few percent of the addresses are targets and most rays end at m = 1 (+inf is not a hole).
#include "smt_common.h"
#include "fill_rules.h"
#include <new>
#include <vector>

using namespace fillrule;

namespace {

constexpr int NT = 256;
constexpr int MAX_GRID_Y = 65535;
constexpr int CNT_BLOCKS = 1024;                      // grid-stride cap of the two counting kernels

// per-pair state, int32[8]
enum { S_NOCC = 0, S_NMIS = 1, S_MID0 = 2, S_MID1 = 3, S_OOB = 4, S_NTHIRD = 5, S_MID2 = 6, S_WORDS = 8 };

struct Shape {
    int pairs, row, col;
    size_t disp_stride, cls_stride;
};

// whether pass k (0, 1: list passes; 2: holes) has anything to do for a pair with this state
__host__ __device__ __forceinline__ bool pass_runs(const int *st, int k)
{
    if (st[S_OOB]) return false;
    if (k < 2) return st[k] > 0;                                              // :175
    return third_pass_tested(st[S_NMIS]) && !third_pass_overruns(st[S_NMIS], st[S_NTHIRD]) && st[S_NTHIRD] > 0;
}

__host__ __device__ __forceinline__ void status_of(const int *st, int *out)
{
    const bool tested = !st[S_OOB] && third_pass_tested(st[S_NMIS]);
    out[0] = st[S_NOCC];
    out[1] = st[S_NMIS];
    out[2] = tested ? st[S_NTHIRD] : -1;
    out[3] = st[S_OOB] ? SMT_FILL_UB_LIST : (tested && third_pass_overruns(st[S_NMIS], st[S_NTHIRD]) ? SMT_FILL_UB_THIRD : 0);
}

__global__ void __launch_bounds__(NT) k_fb_count(const uint8_t *__restrict__ cls, Shape sh, int *__restrict__ state)
{
    __shared__ int s_acc[5];
    const long n = (long)sh.row * sh.col;
    for (int b = blockIdx.y; b < sh.pairs; b += gridDim.y) {
        const uint8_t *cb = cls + (size_t)b * sh.cls_stride;
        if (threadIdx.x < 5) s_acc[threadIdx.x] = 0;
        __syncthreads();
        int cnt[2] = {0, 0}, mid[2] = {0, 0}, oob = 0;
        for (long p = (long)blockIdx.x * NT + threadIdx.x; p < n; p += (long)gridDim.x * NT) {
            const int c = cb[p];
            if (c != 1 && c != 2) continue;
            const int i = (int)(p / sh.col), j = (int)(p - (long)i * sh.col);
            cnt[c - 1]++;
            if (i == sh.col / 2) mid[c - 1] = 1;
            if (out_of_buffer(sh.row, sh.col, i, j)) oob = 1;
        }
        if (cnt[0]) atomicAdd(&s_acc[S_NOCC], cnt[0]);
        if (cnt[1]) atomicAdd(&s_acc[S_NMIS], cnt[1]);
        if (mid[0]) atomicOr(&s_acc[S_MID0], 1);
        if (mid[1]) atomicOr(&s_acc[S_MID1], 1);
        if (oob) atomicOr(&s_acc[S_OOB], 1);
        __syncthreads();
        int *st = state + (size_t)b * S_WORDS;
        if (threadIdx.x < 2 && s_acc[threadIdx.x]) atomicAdd(&st[threadIdx.x], s_acc[threadIdx.x]);
        if (threadIdx.x >= 2 && threadIdx.x < 5 && s_acc[threadIdx.x]) atomicOr(&st[threadIdx.x], 1);
        __syncthreads();                                                    // s_acc reused by the next pair
    }
}

__global__ void __launch_bounds__(NT) k_fb_holes(const float *__restrict__ disp, Shape sh, int *__restrict__ state)
{
    __shared__ int s_cnt, s_mid;
    const long n = (long)sh.row * sh.col;
    for (int b = blockIdx.y; b < sh.pairs; b += gridDim.y) {
        int *st = state + (size_t)b * S_WORDS;
        if (st[S_OOB] || !third_pass_tested(st[S_NMIS])) continue;          // uniform over the workgroup
        const float *db = disp + (size_t)b * sh.disp_stride;
        if (threadIdx.x == 0) { s_cnt = 0; s_mid = 0; }
        __syncthreads();
        int mine = 0, mid = 0;
        for (long p = (long)blockIdx.x * NT + threadIdx.x; p < n; p += (long)gridDim.x * NT)
            if (db[p] == HOLE) { mine++; if (p / sh.row == sh.col / 2) mid = 1; }
        if (mine) atomicAdd(&s_cnt, mine);
        if (mid) atomicOr(&s_mid, 1);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (s_cnt) atomicAdd(&st[S_NTHIRD], s_cnt);
            if (s_mid) atomicOr(&st[S_MID2], 1);
        }
        __syncthreads();
    }
}

// pass k: the fill value of every address that has a target, into fill[pair][address]
__global__ void __launch_bounds__(NT) k_fb_collect(const float *__restrict__ disp, const uint8_t *__restrict__ cls,
                                                   Shape sh, FillCfg c, int k, const int *__restrict__ state,
                                                   float *__restrict__ fill)
{
    const long n = (long)sh.row * sh.col;
    const long a = (long)blockIdx.x * NT + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    for (int b = blockIdx.y; b < sh.pairs; b += gridDim.y) {
        const int *st = state + (size_t)b * S_WORDS;
        if (!pass_runs(st, k)) continue;
        const float *db = disp + (size_t)b * sh.disp_stride;
        const uint8_t *cb = cls + (size_t)b * sh.cls_stride;
        float *fb = fill + (size_t)b * n;
        bool tgt = false;
        int y = 0, x = 0, set = 0;
        if (a < n) {
            if (k < 2) {
                if (winner(cb, sh.row, sh.col, a, k + 1, y, x)) {
                    tgt = true;
                    set = set_of_list_target(k == 1 && st[S_MID0], st[S_MID0 + k], y, sh.col);
                }
            } else if (db[a] == HOLE) {
                tgt = true;
                y = (int)(a / sh.row); x = (int)(a - (long)y * sh.row);
                set = set_of_hole(st[S_MID0] || st[S_MID1], st[S_MID2], y, sh.col);
            }
        }
        const unsigned long long mask = __ballot(tgt);
        if (mask == 0) continue;                                            // uniform over the wave
        // compact: target number t of the wave moves to lane t (the others fill the lanes behind; a bijection)
        const int cnt = __popcll(mask);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        const int dest = tgt ? before : cnt + lane - before;
        const int py = __builtin_amdgcn_ds_permute(dest * 4, y);
        const int px = __builtin_amdgcn_ds_permute(dest * 4, (int)((unsigned)x | ((unsigned)set << 31)));
        const int s = lane & 7;
        for (int r = 0; r * 8 < cnt; r++) {                                 // all 64 lanes stay in the loop
            const int slot = r * 8 + (lane >> 3);
            const bool live = slot < cnt;                                   // whole groups are live or not
            const int src = live ? slot : 0;
            const int ty = __shfl(py, src, WAVE);
            const unsigned tp = (unsigned)__shfl(px, src, WAVE);
            const int tx = (int)(tp & 0x7fffffffu), tset = (int)(tp >> 31);
            float val = 0.0f;
            const bool found = live && ray(db, c, ty, tx, tset, s, val);
            const float v = pick_group(found, val, k == 0 ? 0 : 1);
            if (live && s == 0) fb[(long)ty * sh.row + tx] = v;             // = the target's address, < n
        }
    }
}

__global__ void __launch_bounds__(NT) k_fb_apply(float *__restrict__ disp, const uint8_t *__restrict__ cls, Shape sh,
                                                 int k, const int *__restrict__ state, const float *__restrict__ fill)
{
    const long n = (long)sh.row * sh.col;
    const long a = (long)blockIdx.x * NT + threadIdx.x;
    if (a >= n) return;
    for (int b = blockIdx.y; b < sh.pairs; b += gridDim.y) {
        if (!pass_runs(state + (size_t)b * S_WORDS, k)) continue;
        int i, j;
        if (winner(cls + (size_t)b * sh.cls_stride, sh.row, sh.col, a, k + 1, i, j))
            disp[(size_t)b * sh.disp_stride + a] = fill[(size_t)b * n + a];
    }
}

__global__ void __launch_bounds__(NT) k_fb_writeback(float *__restrict__ disp, Shape sh, const int *__restrict__ state,
                                                     const float *__restrict__ fill, int *__restrict__ status)
{
    const long n = (long)sh.row * sh.col;
    const long a = (long)blockIdx.x * NT + threadIdx.x;
    for (int b = blockIdx.y; b < sh.pairs; b += gridDim.y) {
        const int *st = state + (size_t)b * S_WORDS;
        if (status && a == 0) status_of(st, status + (size_t)b * 4);
        if (a >= n || !pass_runs(st, 2)) continue;
        float *dp = disp + (size_t)b * sh.disp_stride + a;
        if (*dp == HOLE) *dp = fill[(size_t)b * n + a];
    }
}

int batch_check(const float *disp, const uint8_t *cls, int pairs, size_t disp_stride, size_t cls_stride, int row, int col,
                int dispRange)
{
    if (!disp || !cls || pairs < 0 || row <= 0 || col <= 0 || dispRange < 0) return SMT_ERR_ARG;
    if ((long long)row * col >= (1ll << 31)) return SMT_ERR_ARG;
    const size_t n = (size_t)row * col;
    if ((disp_stride != 0 && disp_stride < n) || (cls_stride != 0 && cls_stride < n)) return SMT_ERR_ARG;
    return SMT_OK;
}

}  // namespace

SMT_API int smt_fill_the_hole_batch(float *disp, const uint8_t *cls, int pairs, size_t disp_stride, size_t cls_stride,
                                    int row, int col, int dispRange, int *status, void *stream)
{
    const int rc = batch_check(disp, cls, pairs, disp_stride, cls_stride, row, col, dispRange);
    if (rc != SMT_OK) return rc;
    if (pairs == 0) return SMT_OK;
    hipStream_t st = smt_stream(stream);
    const size_t n = (size_t)row * col;
    Shape sh = {pairs, row, col, disp_stride ? disp_stride : n, cls_stride ? cls_stride : n};
    FillCfg c;
    cfg_init(c, row, col, dispRange);
    const size_t fill_bytes = (size_t)pairs * n * sizeof(float), state_bytes = (size_t)pairs * S_WORDS * sizeof(int);
    void *scratch = nullptr;
    const hipError_t e = smt_scratch_alloc(&scratch, fill_bytes + state_bytes, st);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    float *fill = (float *)scratch;
    int *state = (int *)((char *)scratch + fill_bytes);
    const unsigned gy = pairs < MAX_GRID_Y ? pairs : MAX_GRID_Y;
    const unsigned nb = (unsigned)((n + NT - 1) / NT);
    const dim3 per_addr(nb, gy), counting(nb < CNT_BLOCKS ? nb : CNT_BLOCKS, gy);
    int ret = SMT_OK;
    if (hipMemsetAsync(state, 0, state_bytes, st) != hipSuccess) ret = SMT_ERR_HIP;
    if (ret == SMT_OK) {
        hipLaunchKernelGGL(k_fb_count, counting, dim3(NT), 0, st, cls, sh, state);
        for (int k = 0; k < 2; k++) {
            hipLaunchKernelGGL(k_fb_collect, per_addr, dim3(NT), 0, st, (const float *)disp, cls, sh, c, k,
                               (const int *)state, fill);
            hipLaunchKernelGGL(k_fb_apply, per_addr, dim3(NT), 0, st, disp, cls, sh, k, (const int *)state,
                               (const float *)fill);
        }
        hipLaunchKernelGGL(k_fb_holes, counting, dim3(NT), 0, st, (const float *)disp, sh, state);
        hipLaunchKernelGGL(k_fb_collect, per_addr, dim3(NT), 0, st, (const float *)disp, cls, sh, c, 2,
                           (const int *)state, fill);
        hipLaunchKernelGGL(k_fb_writeback, per_addr, dim3(NT), 0, st, disp, sh, (const int *)state, (const float *)fill,
                           status);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { g_smt_last_hip = (int)le; ret = SMT_ERR_HIP; }
    }
    smt_scratch_free(scratch, st);
    return ret;
}

// Host twin (test hook, no GPU, no HIP call): the same passes over host memory, one address after the other, through
// the same inline functions -- target derivation (winner), set choice, pick, pass gating (pass_runs) and status.
SMT_API int smt_fill_the_hole_batch_host(float *disp, const uint8_t *cls, int pairs, size_t disp_stride,
                                         size_t cls_stride, int row, int col, int dispRange, int *status)
{
    const int rc = batch_check(disp, cls, pairs, disp_stride, cls_stride, row, col, dispRange);
    if (rc != SMT_OK) return rc;
    if (pairs == 0) return SMT_OK;
    const long n = (long)row * col;
    if (disp_stride == 0) disp_stride = (size_t)n;
    if (cls_stride == 0) cls_stride = (size_t)n;
    FillCfg c;
    cfg_init(c, row, col, dispRange);
    std::vector<float> fill;
    std::vector<unsigned char> hit;
    try { fill.resize((size_t)n); hit.resize((size_t)n); } catch (const std::bad_alloc &) { return SMT_ERR_ALLOC; }
    for (int b = 0; b < pairs; b++) {
        float *db = disp + (size_t)b * disp_stride;
        const uint8_t *cb = cls + (size_t)b * cls_stride;
        int st[S_WORDS] = {0};
        for (long p = 0; p < n; p++) {                                      // k_fb_count
            const int cc = cb[p];
            if (cc != 1 && cc != 2) continue;
            const int i = (int)(p / col), j = (int)(p - (long)i * col);
            st[cc - 1]++;
            if (i == col / 2) st[S_MID0 + cc - 1] = 1;
            if (out_of_buffer(row, col, i, j)) st[S_OOB] = 1;
        }
        for (int k = 0; k < 3; k++) {
            if (k == 2 && !st[S_OOB] && third_pass_tested(st[S_NMIS]))      // k_fb_holes
                for (long p = 0; p < n; p++)
                    if (db[p] == HOLE) { st[S_NTHIRD]++; if (p / row == col / 2) st[S_MID2] = 1; }
            if (!pass_runs(st, k)) continue;
            for (long a = 0; a < n; a++) {                                  // k_fb_collect
                int y = 0, x = 0, set = 0;
                hit[(size_t)a] = 0;
                if (k < 2) {
                    if (!winner(cb, row, col, a, k + 1, y, x)) continue;
                    set = set_of_list_target(k == 1 && st[S_MID0], st[S_MID0 + k], y, col);
                } else {
                    if (db[a] != HOLE) continue;
                    y = (int)(a / row); x = (int)(a - (long)y * row);
                    set = set_of_hole(st[S_MID0] || st[S_MID1], st[S_MID2], y, col);
                }
                float vals[8] = {0};
                unsigned fm = 0;
                for (int s = 0; s < 8; s++)
                    if (ray(db, c, y, x, set, s, vals[s])) fm |= 1u << s;
                hit[(size_t)a] = 1;
                fill[(size_t)((long)y * row + x)] = pick(vals, fm, k == 0 ? 0 : 1);
            }
            for (long a = 0; a < n; a++)                                    // k_fb_apply / k_fb_writeback
                if (hit[(size_t)a]) db[a] = fill[(size_t)a];
        }
        if (status) status_of(st, status + (size_t)b * 4);
    }
    return SMT_OK;
}
