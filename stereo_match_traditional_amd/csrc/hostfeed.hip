// Host-fed AD-Census batches (smt_adcensus_host_*): uint8 images in host memory in, both views' WTA maps in host
// memory out, with the copies overlapped with the compute.  What AD-CensusV1/main.cpp does around the hot path --
// imread (:16-17), cvtColor(BGR2GRAY) (:19-20), the uchar -> float staging (:46-55), and the maps back to the host for
// imwrite (:115-117) -- for a whole batch, in chunks of `chunk` pairs on three streams:
//   H2D      uint8 images of chunk k+1 into input slot (k+1) % 2
//   compute  k_stage_pairs (uint8 -> float32, BGR -> gray fused), the batch machinery of adcensus.hip
//            (adcensus_batch_pairs) with the tables of chunk k+1's first pair built inside chunk k's last launch, and
//            k_pack_maps (float32 maps -> uint8, SMT_MAP_U8)
//   D2H      both maps of chunk k out of output slot k % 2
// The enqueue order is one list of operations (hf_schedule) that the run executes and smt_adcensus_host_selftest_schedule
// simulates: every wait is enqueued after its record and no slot is overwritten before its last reader is done.
#include "smt_common.h"
#include "adcensus_internal.h"
#include <string.h>
#include <new>
#include <vector>

namespace {

constexpr int HNT = 256;

__device__ __forceinline__ float gray_of(uint32_t b, uint32_t g, uint32_t r)
{
    return (float)((1868u * b + 9617u * g + 4899u * r + (1u << 13)) >> 14);      // k_bgr2gray (staging.hip)
}

// uint8 [n][CH] -> float32 [n], n = 2 * pairs * H * W: the L and R images of a chunk are adjacent in both buffers, so
// the chunk is one flat array.  16 pixels per thread and step: one (CH = 1) or three (CH = 3) 16-byte loads, four
// 16-byte stores; the n % 16 pixels past the last full group go one by one.  Ordinary stores: the table workgroups
// read the result right away.
template <int CH>
__global__ void __launch_bounds__(HNT) k_stage_pairs(const uint8_t *__restrict__ in, float *__restrict__ out, size_t n)
{
    const size_t n16 = n >> 4, step = (size_t)gridDim.x * HNT;
    const size_t t = (size_t)blockIdx.x * HNT + threadIdx.x;
    for (size_t g = t; g < n16; g += step) {
        float v[16];
        if (CH == 1) {
            const uint4 q = *reinterpret_cast<const uint4 *>(in + g * 16);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
        } else {
            const uint4 *src = reinterpret_cast<const uint4 *>(in + g * 48);
            const uint4 a = src[0], b = src[1], c = src[2];
            const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
            auto byte = [&](int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; };
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = gray_of(byte(3 * k), byte(3 * k + 1), byte(3 * k + 2));
        }
        float4 *dst = reinterpret_cast<float4 *>(out + g * 16);
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
    for (size_t p = (n16 << 4) + t; p < n; p += step)
        out[p] = CH == 1 ? (float)in[p] : gray_of(in[3 * p], in[3 * p + 1], in[3 * p + 2]);
}

// float32 maps -> uint8, n = 2 * pairs * H * W (both views, adjacent).  The WTA writes integers in [0, D) and D <= 256,
// so the conversion is exact.  Four 16-byte loads and one 16-byte store per 16 pixels; the n % 16 rest one by one.
__global__ void __launch_bounds__(HNT) k_pack_maps(const float *__restrict__ in, uint8_t *__restrict__ out, size_t n)
{
    const size_t n16 = n >> 4, step = (size_t)gridDim.x * HNT;
    const size_t t = (size_t)blockIdx.x * HNT + threadIdx.x;
    for (size_t g = t; g < n16; g += step) {
        const float4 *src = reinterpret_cast<const float4 *>(in + g * 16);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 f = src[k];
            w[k] = (uint32_t)f.x | ((uint32_t)f.y << 8) | ((uint32_t)f.z << 16) | ((uint32_t)f.w << 24);
        }
        *reinterpret_cast<uint4 *>(out + g * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (size_t p = (n16 << 4) + t; p < n; p += step) out[p] = (uint8_t)(uint32_t)in[p];
}

// ---- the enqueue schedule ----------------------------------------------------------------------------------------
enum { S_H2D, S_COMP, S_D2H, NSTREAMS };
enum { OP_H2D, OP_STAGE, OP_PAIRS, OP_PACK, OP_D2H, OP_RECORD, OP_WAIT };
// events per chunk k, index k * NEV + e
enum { E_H2D_START, E_H2D_DONE, E_STAGE_START, E_STAGED, E_COMP_START, E_COMPUTED, E_D2H_START, E_D2H_DONE, NEV };

struct HfOp {
    int kind, stream, chunk;
    int first, count;    // OP_PAIRS: pairs [first, first + count) of the chunk
    bool prepped;        // OP_PAIRS: the first pair's tables were built by an earlier launch
    bool next;           // OP_PAIRS: the last pair's launch builds the tables of the pair after it (fused)
    int event;           // OP_RECORD / OP_WAIT
};

// The op list of a run of `pairs` pairs in chunks of `chunk`.  fused: adcensus_batch_pairs with sched 2 across chunk
// boundaries (adcensus_fused_both_views); else every chunk is a plain batch.  pack: SMT_MAP_U8.
static void hf_schedule(int pairs, int chunk, bool fused, bool pack, std::vector<HfOp> &ops)
{
    ops.clear();
    const int nch = (pairs + chunk - 1) / chunk;
    auto add = [&](int kind, int s, int k) { ops.push_back(HfOp{kind, s, k, 0, 0, false, false, -1}); };
    auto rec = [&](int s, int k, int e) { ops.push_back(HfOp{OP_RECORD, s, k, 0, 0, false, false, k * NEV + e}); };
    auto wait = [&](int s, int k, int e) { ops.push_back(HfOp{OP_WAIT, s, k, 0, 0, false, false, k * NEV + e}); };
    auto run = [&](int k, int first, int count, bool prepped, bool next) {
        ops.push_back(HfOp{OP_PAIRS, S_COMP, k, first, count, prepped, next, -1});
    };
    auto stage = [&](int k) {
        wait(S_COMP, k, E_H2D_DONE);
        add(OP_STAGE, S_COMP, k);
        rec(S_COMP, k, E_STAGED);
    };
    if (nch <= 0) return;
    // chunk 0 is copied and staged before the loop
    rec(S_H2D, 0, E_H2D_START);
    add(OP_H2D, S_H2D, 0);
    rec(S_H2D, 0, E_H2D_DONE);
    wait(S_COMP, 0, E_H2D_DONE);
    rec(S_COMP, 0, E_STAGE_START);
    add(OP_STAGE, S_COMP, 0);
    rec(S_COMP, 0, E_STAGED);
    for (int k = 0; k < nch; k++) {
        const int c = pairs - k * chunk < chunk ? pairs - k * chunk : chunk;
        const bool more = k + 1 < nch;
        // 1. H2D of chunk k+1 into input slot (k+1) % 2, whose last reader was the staging of chunk k-1
        if (more) {
            if (k >= 1) wait(S_H2D, k - 1, E_STAGED);
            rec(S_H2D, k + 1, E_H2D_START);
            add(OP_H2D, S_H2D, k + 1);
            rec(S_H2D, k + 1, E_H2D_DONE);
        }
        // 2. compute of chunk k; its output slot k % 2 was last read by the D2H of chunk k-2
        if (k >= 2) wait(S_COMP, k - 2, E_D2H_DONE);
        rec(S_COMP, k, E_COMP_START);
        if (fused) {
            if (c > 1) run(k, 0, c - 1, k > 0, true);       // the last of these builds the tables of pair c-1
            if (more) stage(k + 1);
            run(k, c - 1, 1, k > 0 || c > 1, more);        // ... and pair c-1 those of chunk k+1's pair 0
        } else {
            run(k, 0, c, false, false);
            if (more) stage(k + 1);
        }
        if (pack) add(OP_PACK, S_COMP, k);
        rec(S_COMP, k, E_COMPUTED);
        // 3. D2H of chunk k
        wait(S_D2H, k, E_COMPUTED);
        rec(S_D2H, k, E_D2H_START);
        add(OP_D2H, S_D2H, k);
        rec(S_D2H, k, E_D2H_DONE);
    }
}

// Simulates an op list: happens-before through stream order and record -> wait edges (vector clocks over the three
// streams), and checks every rule of the schedule.  SMT_OK or SMT_ERR_STATE.
static int hf_check(const std::vector<HfOp> &ops, int pairs, int chunk, bool fused, bool pack)
{
    const int nch = (pairs + chunk - 1) / chunk;
    struct VC { long t[NSTREAMS]; };
    struct Access { int stream; long seq; };
    struct Slot { int content = -1; Access writer{-1, 0}; std::vector<Access> readers; };
    // slots: input (u8) 0-1, staging 2-3, float maps 4-5, packed maps 6-7
    Slot slot[8];
    std::vector<VC> ev((size_t)nch * NEV);
    std::vector<char> recorded((size_t)nch * NEV, 0);
    std::vector<int> in_count(pairs, 0), out_count(pairs, 0), tables((size_t)pairs, 0);
    VC cur[NSTREAMS] = {};
    long seq[NSTREAMS] = {};
    auto hb = [&](const Access &a, const VC &b) { return a.stream < 0 || b.t[a.stream] >= a.seq; };
    bool ok = true;
    auto chunk_size = [&](int k) { return pairs - k * chunk < chunk ? pairs - k * chunk : chunk; };
    auto write = [&](int s, int k, const Access &me, const VC &vc) {
        Slot &sl = slot[s];
        if (!hb(sl.writer, vc)) ok = false;
        for (const Access &r : sl.readers) if (!hb(r, vc)) ok = false;
        sl.content = k; sl.writer = me; sl.readers.clear();
    };
    auto read = [&](int s, int k, const Access &me, const VC &vc) {
        Slot &sl = slot[s];
        if (sl.content != k || !hb(sl.writer, vc)) ok = false;
        sl.readers.push_back(me);
    };
    auto build = [&](int k, int p) { if (k < nch && p < chunk_size(k)) tables[(size_t)k * chunk + p]++; else ok = false; };
    for (const HfOp &o : ops) {
        const int s = o.stream, k = o.chunk;
        if (s < 0 || s >= NSTREAMS || k < 0 || k >= nch) return SMT_ERR_STATE;
        cur[s].t[s] = ++seq[s];
        const VC vc = cur[s];
        const Access me{s, seq[s]};
        const int c = chunk_size(k), base = k * chunk;
        switch (o.kind) {
        case OP_RECORD:
            if (o.event < 0 || o.event >= nch * NEV || recorded[o.event]) return SMT_ERR_STATE;
            recorded[o.event] = 1;
            ev[o.event] = vc;
            break;
        case OP_WAIT:
            if (o.event < 0 || o.event >= nch * NEV || !recorded[o.event]) return SMT_ERR_STATE;   // wait before record
            for (int j = 0; j < NSTREAMS; j++) if (ev[o.event].t[j] > cur[s].t[j]) cur[s].t[j] = ev[o.event].t[j];
            break;
        case OP_H2D:
            if (s != S_H2D) return SMT_ERR_STATE;
            for (int p = 0; p < c; p++) in_count[base + p]++;
            write(0 + k % 2, k, me, vc);
            break;
        case OP_STAGE:
            if (s != S_COMP) return SMT_ERR_STATE;
            read(0 + k % 2, k, me, vc);
            write(2 + k % 2, k, me, vc);
            break;
        case OP_PAIRS: {
            if (s != S_COMP || o.count < 1 || o.first < 0 || o.first + o.count > c) return SMT_ERR_STATE;
            read(2 + k % 2, k, me, vc);
            for (int p = o.first; p < o.first + o.count; p++) {
                if (p == o.first ? !o.prepped : !fused) build(k, p);
                if (tables[(size_t)base + p] != 1) return SMT_ERR_STATE;      // built once, before its cost launch
                if (fused && p + 1 < o.first + o.count) build(k, p + 1);      // inside this pair's launch
            }
            if (o.next) {
                if (!fused) return SMT_ERR_STATE;
                if (o.first + o.count < c) build(k, o.first + o.count);
                else { read(2 + (k + 1) % 2, k + 1, me, vc); build(k + 1, 0); }
            }
            write(pack ? 4 : 4 + k % 2, k, me, vc);
            break;
        }
        case OP_PACK:
            if (s != S_COMP || !pack) return SMT_ERR_STATE;
            read(4, k, me, vc);
            write(6 + k % 2, k, me, vc);
            break;
        case OP_D2H:
            if (s != S_D2H) return SMT_ERR_STATE;
            read(pack ? 6 + k % 2 : 4 + k % 2, k, me, vc);
            for (int p = 0; p < c; p++) out_count[base + p]++;
            break;
        default:
            return SMT_ERR_STATE;
        }
        if (!ok) return SMT_ERR_STATE;
    }
    for (int p = 0; p < pairs; p++)
        if (in_count[p] != 1 || out_count[p] != 1 || tables[p] != 1) return SMT_ERR_STATE;
    // the run synchronises the D2H stream only: everything must be ordered before its last operation
    for (int s = 0; s < NSTREAMS; s++) if (seq[s] > cur[S_D2H].t[s]) return SMT_ERR_STATE;
    return SMT_OK;
}

}  // namespace

struct smt_adcensus_host {
    int device, H, W, D, channels, format, chunk, blocks;
    smt_adcensus *adc;
    bool fused;
    hipStream_t st[NSTREAMS];
    uint8_t *in[2];      // [2][chunk][H][W][channels]: L of the chunk's c pairs, then R
    float *stg[2];       // [2][chunk][H][W], same layout
    float *fmap[2];      // float32 maps (L then R): both slots with SMT_MAP_F32; slot 0 alone (the pack's input) with U8
    uint8_t *u8map[2];   // SMT_MAP_U8: packed maps
    std::vector<hipEvent_t> ev;   // NEV per chunk, grown to the largest run
    std::vector<HfOp> ops;
    smt_host_stats stats;
};

SMT_API int smt_host_malloc(void **p, size_t bytes)
{
    if (!p) return SMT_ERR_ARG;
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { g_smt_last_hip = (int)e; return SMT_ERR_ALLOC; }
    return SMT_OK;
}

SMT_API int smt_host_free(void *p) { SMT_HIP(hipHostFree(p)); return SMT_OK; }

SMT_API int smt_adcensus_host_destroy(smt_adcensus_host *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    for (int s = 0; s < NSTREAMS; s++)
        if (h->st[s]) (void)hipStreamSynchronize(h->st[s]);
    if (h->adc) smt_adcensus_destroy(h->adc);
    for (int s = 0; s < NSTREAMS; s++)
        if (h->st[s]) (void)hipStreamDestroy(h->st[s]);
    for (int t = 0; t < 2; t++) {
        (void)hipFree(h->in[t]); (void)hipFree(h->stg[t]); (void)hipFree(h->fmap[t]); (void)hipFree(h->u8map[t]);
    }
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    delete h;
    return SMT_OK;
}

static int host_create(int H, int W, int D, float sigmaC, float sigmaS, int channels, int format, int chunk,
                       smt_adcensus_host **out)
{
    smt_adcensus_host *h = new (std::nothrow) smt_adcensus_host();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->channels = channels; h->format = format; h->chunk = chunk;
    int rc = smt_adcensus_create_ex(-1, H, W, D, sigmaC, sigmaS,
                                    SMT_ADCENSUS_NO_PLACEMENT_SEARCH | SMT_ADCENSUS_NO_STORE_CALIBRATION, &h->adc);
    if (rc != SMT_OK) { h->adc = nullptr; smt_adcensus_host_destroy(h); return rc; }
    h->fused = adcensus_fused_both_views(h->adc);
    for (int s = 0; s < NSTREAMS && rc == SMT_OK; s++)
        if (hipStreamCreateWithFlags(&h->st[s], hipStreamNonBlocking) != hipSuccess) { h->st[s] = nullptr; rc = SMT_ERR_HIP; }
    if (rc == SMT_OK) rc = smt_adcensus_set_stream(h->adc, h->st[S_COMP]);
    int ncu = 0;
    if (rc == SMT_OK && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess)
        rc = SMT_ERR_HIP;
    h->blocks = (ncu > 0 ? ncu : 1) * 8;                   // streaming kernels: 8 workgroups per CU, grid-stride beyond
    const size_t n = (size_t)2 * chunk * H * W;            // pixels of a full chunk, both views
    auto alloc = [&](void **p, size_t bytes) { if (rc == SMT_OK) rc = smt_malloc(p, bytes); };
    for (int t = 0; t < 2; t++) {
        alloc((void **)&h->in[t], n * channels);
        alloc((void **)&h->stg[t], n * 4);
        if (format == SMT_MAP_F32 || t == 0) alloc((void **)&h->fmap[t], n * 4);
        if (format == SMT_MAP_U8) alloc((void **)&h->u8map[t], n);
    }
    if (rc != SMT_OK) { smt_adcensus_host_destroy(h); return rc; }
    *out = h;
    return SMT_OK;
}

SMT_API int smt_adcensus_host_create(int device, int H, int W, int D, float sigmaC, float sigmaS, int channels,
                                     int map_format, int chunk, smt_adcensus_host **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || !(sigmaC > 0.0f) || !(sigmaS > 0.0f) ||
        (channels != 1 && channels != 3) || (map_format != SMT_MAP_F32 && map_format != SMT_MAP_U8) ||
        (map_format == SMT_MAP_U8 && D > 256) || chunk < 1 || (double)2 * chunk * H * W * 4 > (double)SIZE_MAX / 2)
        return SMT_ERR_ARG;
    if (device < 0) return host_create(H, W, D, sigmaC, sigmaS, channels, map_format, chunk, out);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return host_create(H, W, D, sigmaC, sigmaS, channels, map_format, chunk, out);
}

// hipPointerGetAttributes on memory HIP does not know fails; that is "pageable", not an error of the run
static int is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return a.type == hipMemoryTypeHost ? 1 : 0;
}

// Executes the op list; on a HIP error the caller drains the streams.
static int host_enqueue(smt_adcensus_host *h, const uint8_t *L, const uint8_t *R, int pairs, void *dispL, void *dispR)
{
    const size_t N = (size_t)h->H * h->W, ch = (size_t)h->channels;
    const size_t esz = h->format == SMT_MAP_U8 ? 1 : 4;
    const bool pack = h->format == SMT_MAP_U8;
    auto csize = [&](int k) { return pairs - k * h->chunk < h->chunk ? pairs - k * h->chunk : h->chunk; };
    for (const HfOp &o : h->ops) {
        const int k = o.chunk, c = csize(k);
        const size_t base = (size_t)k * h->chunk;
        hipStream_t st = h->st[o.stream];
        float *fm = pack ? h->fmap[0] : h->fmap[k % 2];
        switch (o.kind) {
        case OP_RECORD: SMT_HIP(hipEventRecord(h->ev[o.event], st)); break;
        case OP_WAIT: SMT_HIP(hipStreamWaitEvent(st, h->ev[o.event], 0)); break;
        case OP_H2D: {
            const size_t bytes = c * N * ch;
            SMT_HIP(hipMemcpyAsync(h->in[k % 2], L + base * N * ch, bytes, hipMemcpyHostToDevice, st));
            SMT_HIP(hipMemcpyAsync(h->in[k % 2] + bytes, R + base * N * ch, bytes, hipMemcpyHostToDevice, st));
            h->stats.h2d_bytes += 2 * bytes;
            break;
        }
        case OP_STAGE: {
            const size_t n = 2 * (size_t)c * N, groups = (n / 16 + HNT - 1) / HNT;
            const unsigned grid = (unsigned)(groups < 1 ? 1 : groups < (size_t)h->blocks ? groups : h->blocks);
            if (h->channels == 3)
                hipLaunchKernelGGL(k_stage_pairs<3>, dim3(grid), dim3(HNT), 0, st, h->in[k % 2], h->stg[k % 2], n);
            else
                hipLaunchKernelGGL(k_stage_pairs<1>, dim3(grid), dim3(HNT), 0, st, h->in[k % 2], h->stg[k % 2], n);
            SMT_LAUNCH_CHECK();
            break;
        }
        case OP_PAIRS: {
            const float *sl = h->stg[k % 2], *sr = sl + c * N;
            if (!h->fused) {
                const int rc = smt_adcensus_compute_batch(h->adc, sl, sr, c, SMT_VIEW_BOTH, fm, fm + c * N);
                if (rc != SMT_OK) return rc;
                break;
            }
            const float *nl = nullptr, *nr = nullptr;
            if (o.next) {
                const int e = o.first + o.count;
                if (e < c) { nl = sl + e * N; nr = sr + e * N; }
                else { nl = h->stg[(k + 1) % 2]; nr = nl + csize(k + 1) * N; }
            }
            const int rc = adcensus_batch_pairs(h->adc, sl + o.first * N, sr + o.first * N, o.count, SMT_VIEW_BOTH,
                                                fm + o.first * N, fm + (c + o.first) * N, 2, o.prepped, nl, nr, true,
                                                false);
            if (rc != SMT_OK) return rc;
            break;
        }
        case OP_PACK: {
            const size_t n = 2 * (size_t)c * N, groups = (n / 16 + HNT - 1) / HNT;
            const unsigned grid = (unsigned)(groups < 1 ? 1 : groups < (size_t)h->blocks ? groups : h->blocks);
            hipLaunchKernelGGL(k_pack_maps, dim3(grid), dim3(HNT), 0, st, h->fmap[0], h->u8map[k % 2], n);
            SMT_LAUNCH_CHECK();
            break;
        }
        case OP_D2H: {
            const size_t bytes = c * N * esz;
            const uint8_t *src = pack ? h->u8map[k % 2] : (const uint8_t *)h->fmap[k % 2];
            SMT_HIP(hipMemcpyAsync((uint8_t *)dispL + base * N * esz, src, bytes, hipMemcpyDeviceToHost, st));
            SMT_HIP(hipMemcpyAsync((uint8_t *)dispR + base * N * esz, src + bytes, bytes, hipMemcpyDeviceToHost, st));
            h->stats.d2h_bytes += 2 * bytes;
            break;
        }
        default: return SMT_ERR_STATE;
        }
    }
    return SMT_OK;
}

SMT_API int smt_adcensus_host_run(smt_adcensus_host *h, const uint8_t *L, const uint8_t *R, int pairs, void *dispL,
                                  void *dispR)
{
    if (!h || pairs < 0) return SMT_ERR_ARG;
    if (pairs == 0) return SMT_OK;
    if (!L || !R || !dispL || !dispR) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int nch = (pairs + h->chunk - 1) / h->chunk;
    while (h->ev.size() < (size_t)nch * NEV) {
        hipEvent_t e;
        SMT_HIP(hipEventCreate(&e));
        h->ev.push_back(e);
    }
    hf_schedule(pairs, h->chunk, h->fused, h->format == SMT_MAP_U8, h->ops);
    h->stats = smt_host_stats{};
    h->stats.chunks = nch;
    h->stats.pinned_in = is_pinned(L) && is_pinned(R);
    h->stats.pinned_out = is_pinned(dispL) && is_pinned(dispR);
    int rc = host_enqueue(h, L, R, pairs, dispL, dispR);
    if (rc != SMT_OK) {
        // the host buffers may still be in use by what was enqueued
        for (int s = 0; s < NSTREAMS; s++) (void)hipStreamSynchronize(h->st[s]);
        return rc;
    }
    // everything is ordered before the last D2H (hf_check): one synchronisation, then the events are complete
    SMT_HIP(hipStreamSynchronize(h->st[S_D2H]));
    smt_host_stats &s = h->stats;
    auto ms = [&](int k0, int e0, int k1, int e1, double &acc) -> int {
        float t = 0.0f;
        SMT_HIP(hipEventElapsedTime(&t, h->ev[k0 * NEV + e0], h->ev[k1 * NEV + e1]));
        acc += t;
        return SMT_OK;
    };
    rc = ms(0, E_H2D_START, nch - 1, E_D2H_DONE, s.wall_ms);
    if (rc == SMT_OK) rc = ms(0, E_STAGE_START, 0, E_STAGED, s.compute_ms);
    for (int k = 0; k < nch && rc == SMT_OK; k++) {
        rc = ms(k, E_H2D_START, k, E_H2D_DONE, s.h2d_ms);
        if (rc == SMT_OK) rc = ms(k, E_COMP_START, k, E_COMPUTED, s.compute_ms);
        if (rc == SMT_OK) rc = ms(k, E_D2H_START, k, E_D2H_DONE, s.d2h_ms);
    }
    return rc;
}

SMT_API int smt_adcensus_host_stats(smt_adcensus_host *h, smt_host_stats *s)
{
    if (!h || !s) return SMT_ERR_ARG;
    *s = h->stats;
    return SMT_OK;
}

// Host-side check of the enqueue schedule (no GPU): both the fused and the plain-batch form, with and without the
// pack, simulated by hf_check.
SMT_API int smt_adcensus_host_selftest_schedule(int pairs, int chunk)
{
    if (pairs < 0 || chunk <= 0) return SMT_ERR_ARG;
    std::vector<HfOp> ops;
    for (int fused = 0; fused < 2; fused++)
        for (int pack = 0; pack < 2; pack++) {
            hf_schedule(pairs, chunk, fused, pack, ops);
            if ((pairs == 0) != ops.empty()) return SMT_ERR_STATE;
            const int rc = hf_check(ops, pairs, chunk, fused, pack);
            if (rc != SMT_OK) return rc;
        }
    return SMT_OK;
}
