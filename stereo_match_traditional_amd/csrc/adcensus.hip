// AD + 9x7 census cost volume with fused WTA -- replaces class AD_Census
// (AD-CensusV1/AD-Census.h) for both views.
//
// Formulation (different from the reference's per-(i,j,d) census rebuild, AD-Census.h:142-269,
// same results):
//   left  view: census(i,j,d) = popcount((cenA_L[i][j] ^ cenX_R[i][max(j-d,-3)]) & M[i][j])
//               AD(i,j,d)     = |L[i][j] - R[i][max(j-d,0)]|
//   right view: census(i,j,d) = popcount((cenA_R[i][j] ^ cenX_L[i][min(j+d,W+3)]) & M[i][j])
//               AD(i,j,d)     = |L[i][min(j+d,W-1)] - R[i][j]|
// with cenA_* the ordinary 63-bit census of the anchor image (invalid taps = 0), M the
// in-image tap mask of the anchor pixel (validity is tested on anchor coordinates,
// AD-Census.h:173 / :238), cenX_R the right image's census on a left-replicate-extended
// row (:159-160, :177-178) and cenX_L the left image's census with the reference's
// "column 0 past the right edge" rule for neighbours and "column W-1" rule for the
// centre (:224-225, :242-243).  The "copy d-1" branches of ComputeAD (:88-92, :116-120)
// are exactly the clamps above.
//   cost = lutA[AD] + lutC[census], lutA[k] = 1-expf(-(k/sigmaC)), lutC[k] = 1-expf(-(k/sigmaS))
// built on the HOST with the reference's own float expression (:287-289), so the device
// never evaluates exp.  AD in 0..255 and census in 0..63 because images are integer-valued.
//
// Main kernel: one wavefront spans the disparity axis of one pixel; lane l owns the C =
// D/64 consecutive hypotheses d = l*C .. l*C+C-1 and stores them with one
// dword/x2/x3/x4 store (64*C*4 contiguous bytes per wave).  Row operands are staged in
// LDS once per workgroup; WTA is a wave min + ballot (first strict minimum, :355-373).
// This file is the host side; the kernels are in adcensus_kernels.h, the rules both share in adcensus_rules.h.
#include "adcensus_kernels.h"
#include "adcensus_internal.h"

struct ChainState {
    long n_pairs;        // pairs issued on this chain ([0]: and by every schedule that is not chained)
    bool conv_pending;
    int conv_map;        // index into skeys[]
    float *conv_dR;
};

struct smt_adcensus {
    int device;          // HIP device the handle lives on
    int H, W, D;
    float sigmaC, sigmaS;
    hipStream_t stream;
    float *vol[2];
    Tables T;            // table set used by the pair being issued (= TS[chain_slot(cur, its chain's n_pairs)])
    // Two sets per chain (chain c owns 2c and 2c+1): the tables of a chain's next pair are built while its pair runs.
    // Chain 0 is the state of every schedule but the chained one (smt_adcensus_compute, schedules 0 .. 2, host-fed flow).
    Tables TS[2 * SMT_MAX_CHAINS];
    hipStream_t prep_stream;                 // internal, non-blocking: schedule 1's table stream and chain 1's stream
    hipStream_t chain2_stream;               // internal, non-blocking: chain 2's stream
    hipEvent_t in_ready, prep_done[2], cost_done[2];
    hipEvent_t fork_ev, join_ev[SMT_MAX_CHAINS];   // the chained schedule's edges per call (chain_plan); join_ev[0] unused
    ChainState chain[SMT_MAX_CHAINS];
    // The chain whose state the pair being issued uses, and the internal stream each chain runs on in the call being
    // issued (0: the caller's stream).  All 0 outside adcensus_batch_chained.
    int cur, chain_on[SMT_MAX_CHAINS];
    // The pair being issued runs beside another chain's launch, which fills its drain: the tapered tail's default rule
    // is off for it (maps_taper, chain_taper).  False outside adcensus_batch_chained.
    bool beside;
    hipEvent_t *ev;      // SMT_TIMING_SLOTS * 4, lazily created
    bool timing;
    bool force_generic;  // test hook: route D%64==0 through the generic kernel too
    long n_timed;        // pairs recorded since timing was (re-)enabled
    long n_seen;         // pairs processed since timing was (re-)enabled
    int timing_stride;   // every timing_stride-th pair is recorded
    bool *ev_merged;     // slot recorded 3 events (tables end == cost start, one stream)
    bool plain_stores;   // both-views cost kernel with ordinary instead of streaming stores (chosen at create)
    float store_mode_ms[2];   // calibration: kernel ms with streaming / plain stores (0: not calibrated)
    int place_tries;     // candidate volume pairs tried by place_volumes
    float place_ms;      // store-only time of the pair that was kept (0: no search)
    // Two [H][W] key maps of the shared maps-only form per chain; a chain's pair n merges into map chain_slot(c, n).
    // All are SH_NOKEY after create and whenever no conversion is pending.  chain[c].conv_pending: the shared pair the
    // chain issued last has its partial keys in skeys[conv_map], still to be converted into its right map conv_dR -- by
    // the chain's next shared launch, or by flush_conversion().  Never true when an entry point returns (the caller may
    // free its maps).
    unsigned long long *skeys[2 * SMT_MAX_CHAINS];
    // Deferred volumes of a batch's last pair (smt_adcensus_compute_batch, smt_adcensus_volume).  vol_lent: a caller
    // has been given a volume pointer, so every batch from then on writes its last pair's volumes itself.
    // vol_pending: the last pair took the maps-only path and its volumes are still to be written, by the both-views
    // cost kernel on T.  All that launch needs stays in the handle until the next compute replaces the pending state:
    // T is the pair's table set (nothing rebuilds it; the quirk state of the pair is in the tables' contents, and
    // smt_adcensus_set_quirks changes only edge_col, which the table kernels alone read) and plain_stores is fixed at
    // create.
    bool vol_lent, vol_pending;
    // Workgroups that one slice's CUs (an eighth of the device) hold at a time, of the maps-only kernel this handle's D
    // launches: [0] k_cost_maps_shared, [1] k_cost_maps2p float, [2] k_cost_maps2p rank.  From the occupancy query at
    // create; 0 (unknown, or D > 256) leaves the tapered tail's default rule off (maps_taper).
    int maps_resident[3];
};

// The store-only twin of the both-views cost kernel on (v0, v1): D = 64 C, C = 1..4 (any other C launches C = 4's).
static void store_only(smt_adcensus *h, float *v0, float *v1, hipStream_t st)
{
    const int nbx = (h->W + FTJ - 1) / FTJ, C = h->D / 64;
    (void)dispatch_c<4>(C >= 1 && C <= 3 ? C : 4, [&](auto c) {
        hipLaunchKernelGGL((k_store_only2<decltype(c)::value>), dim3(cost_grid(nbx, h->H, 2)), dim3(NT), 0, st, h->H, h->W, v0, v1, nbx);
    });
}

// Placement-aware allocation of the two cost volumes.  The cost kernel is a pure store stream (8 XCDs,
// each writing its own contiguous eighth of the two volumes), and what that stream reaches depends on
// WHICH physical pages hipMalloc handed out: on one MI355X, in one process, at a constant 2.37 GHz shader
// clock, the store-only twin of the kernel runs at either ~7.0 TB/s or ~5.9 TB/s on successive
// allocations of the same size, and the same virtual range re-allocated later lands in the other mode
// (tools/alloc_probe.hip).  Nothing in the kernel can change that afterwards, so
// Initialize takes up to PLACE_TRIES candidate pairs, times the store-only twin on each (a few launches,
// ~5 ms per candidate at 1080p x 192), keeps the fastest and frees the rest.  Rejected candidates stay
// allocated until the end so that every try gets different pages.  SMT_PLACEMENT=0 in the environment
// turns the search off (first allocation is used).
static int place_volumes(smt_adcensus *h, bool allow_search)
{
    const size_t V = (size_t)h->H * h->W * h->D;
    constexpr int PLACE_TRIES = 6;
    const bool search = allow_search && !placement_off() && h->D % 64 == 0 && h->D <= 256 && V >= ((size_t)1 << 22);
    float *cand[PLACE_TRIES][2] = {};
    float ms[PLACE_TRIES];
    int n = 0, best = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (search && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) return SMT_ERR_HIP;
    // a candidate at this rate is in the fast mode (7.0 TB/s measured at 1080p x 192): stop looking
    const double good_ms = 2.0 * V * 4 / 6.75e12 * 1e3;
    for (; n < (search ? PLACE_TRIES : 1); n++) {
        if (smt_malloc((void **)&cand[n][0], V * 4) != SMT_OK) break;
        if (smt_malloc((void **)&cand[n][1], V * 4) != SMT_OK) { (void)hipFree(cand[n][0]); cand[n][0] = nullptr; break; }
        if (!search) { best = n; n++; break; }
        const int reps = 8;
        for (int k = 0; k < 3; k++) store_only(h, cand[n][0], cand[n][1], nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int k = 0; k < reps; k++) store_only(h, cand[n][0], cand[n][1], nullptr);
        (void)hipEventRecord(e1, nullptr);
        float t = 0;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) t = 1e30f;
        ms[n] = t / reps;
        if (best < 0 || ms[n] < ms[best]) best = n;
        if (ms[n] <= good_ms) { n++; break; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (int k = 0; k < n; k++)
        if (k != best) { (void)hipFree(cand[k][0]); (void)hipFree(cand[k][1]); }
    if (best < 0) return SMT_ERR_ALLOC;
    h->vol[0] = cand[best][0]; h->vol[1] = cand[best][1];
    h->place_tries = n;
    h->place_ms = search ? ms[best] : 0.0f;
    return SMT_OK;
}

// launch_fast<C, FULL> (below) by runtime C = 1..4 hypotheses per lane and full: D == 64 C; false for any other C
static bool launch_fast_as(int C, bool full, smt_adcensus *h, int views, float *dL, float *dR, const float *nL = nullptr,
                           const float *nR = nullptr, bool maps = false);

// Streaming (non-temporal) or ordinary stores for the volumes?  Streaming stores were worth 8-19 % on the
// devices of round 1; on another device the store-only twin is 5 % FASTER with ordinary stores (DESIGN.md
// section 4).  Like the placement this is a property of the device, so Initialize times the real both-views
// kernel a few launches each way on the handle's own (zeroed) tables and volumes and keeps ordinary stores
// only when they win by more than 2 %.  SMT_STORE_MODE=nt / plain in the environment fixes the choice.
static void calibrate_store_mode(smt_adcensus *h, bool allow)
{
    h->plain_stores = false; h->store_mode_ms[0] = h->store_mode_ms[1] = 0.0f;
    const char fixed = store_mode_env();
    if (fixed == 'p') h->plain_stores = true;
    if (fixed == 'p' || fixed == 'n' || !allow) return;
    const size_t V = (size_t)h->H * h->W * h->D;
    if (h->D % 64 != 0 || V < ((size_t)1 << 22)) return;
    const size_t N = (size_t)h->H * h->W;
    // zeroed tables are valid inputs (census 0, bytes 0); the speed of a store-bound kernel does not depend on them
    for (int t = 0; t < 2; t++) {
        for (int v = 0; v < 2; v++) {
            if (hipMemset(h->TS[t].cenA[v], 0, N * 8) != hipSuccess || hipMemset(h->TS[t].u8[v], 0, N) != hipSuccess ||
                hipMemset(h->TS[t].cenX[v], 0, (size_t)h->H * h->TS[t].WX * 8) != hipSuccess) return;
        }
        if (hipMemset(h->TS[t].mask, 0, N * 8) != hipSuccess) return;
    }
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return;
    const hipStream_t keep = h->stream;
    h->stream = nullptr;
    float best[2] = {1e30f, 1e30f};
    for (int round = 0; round < 2; round++)                    // interleaved: nt, plain, nt, plain
        for (int mode = 0; mode < 2; mode++) {
            h->plain_stores = mode == 1;
            const int reps = 4;
            auto launch = [&]() { (void)launch_fast_as(std::min(h->D / 64, 4), true, h, SMT_VIEW_BOTH, nullptr, nullptr); };
            launch();
            (void)hipEventRecord(e0, nullptr);
            for (int k = 0; k < reps; k++) launch();
            (void)hipEventRecord(e1, nullptr);
            float t = 1e30f;
            if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) t /= reps;
            if (t < best[mode]) best[mode] = t;
        }
    h->stream = keep;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    h->store_mode_ms[0] = best[0]; h->store_mode_ms[1] = best[1];
    h->plain_stores = best[1] < 0.98f * best[0];
    // Initialize's contract: the volumes read as zeros until the first Compute* (AD-Census.h:341-342)
    (void)hipMemset(h->vol[0], 0, V * 4); (void)hipMemset(h->vol[1], 0, V * 4);
    (void)hipMemset(h->TS[0].flag, 0, 4);
}

SMT_API int smt_adcensus_store_mode(smt_adcensus *h, int *plain, float *nt_ms, float *plain_ms)
{
    if (!h) return SMT_ERR_ARG;
    if (plain) *plain = h->plain_stores ? 1 : 0;
    if (nt_ms) *nt_ms = h->store_mode_ms[0];
    if (plain_ms) *plain_ms = h->store_mode_ms[1];
    return SMT_OK;
}

SMT_API int smt_adcensus_placement(smt_adcensus *h, int *tries, float *store_only_ms)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (tries) *tries = h->place_tries;
    if (store_only_ms) *store_only_ms = h->place_ms;
    return SMT_OK;
}

// The stream chain c runs on in the call being issued: the caller's, or the internal one the chained schedule gave it.
static hipStream_t chain_stream(const smt_adcensus *h, int c)
{
    return h->chain_on[c] == 0 ? h->stream : h->chain_on[c] == 1 ? h->prep_stream : h->chain2_stream;
}
// The stream of the pair being issued.
static hipStream_t run_stream(const smt_adcensus *h) { return chain_stream(h, h->cur); }

// The pending conversion of chain c's shared form, if any, as a launch of its own on the chain's stream.  Every path
// that is not the chain's next shared launch calls this before it does anything else on that stream.
static void flush_conversion(smt_adcensus *h, int c)
{
    ChainState &ch = h->chain[c];
    if (!ch.conv_pending) return;
    const long N = (long)h->H * h->W;
    hipLaunchKernelGGL(k_shared_convert, dim3((unsigned)shared_conv_items(h->H, h->W)), dim3(NT), 0, chain_stream(h, c),
                       h->skeys[ch.conv_map], ch.conv_dR, N);
    ch.conv_pending = false;
}

// maps_resident of the handle: CUs / 8 x the workgroups per CU the runtime reports for the instantiation that D selects
// (launch_fast_as).  A query that fails leaves 0: the tapered tail's default rule stays off.
template <int C, bool FULL>
static void query_maps_resident(smt_adcensus *h, int cus)
{
    int n[3] = {0, 0, 0};
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[0], k_cost_maps_shared<C, FULL>, NT, 0) != hipSuccess) n[0] = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[1], k_cost_maps2p<C, FULL, MODE_MAPS_FLOAT>, NT, 0) != hipSuccess) n[1] = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n[2], k_cost_maps2p<C, FULL, MODE_MAPS_RANK>, NT, 0) != hipSuccess) n[2] = 0;
    for (int t = 0; t < 3; t++) h->maps_resident[t] = n[t] > 0 ? cus / 8 * n[t] : 0;
}
static void set_maps_resident(smt_adcensus *h)
{
    h->maps_resident[0] = h->maps_resident[1] = h->maps_resident[2] = 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || cus < 8) return;
    (void)dispatch_c<4>((h->D + 63) / 64, [&](auto c) {
        if (h->D % 64 == 0) query_maps_resident<decltype(c)::value, true>(h, cus);
        else query_maps_resident<decltype(c)::value, false>(h, cus);
    });
    (void)hipGetLastError();
}

static int adcensus_create(int H, int W, int D, float sigmaC, float sigmaS, unsigned flags, smt_adcensus **out)
{
    if (!out || H <= 0 || W <= 0 || D <= 0 || D > SMT_MAX_DISPARITY || !(sigmaC > 0.0f) || !(sigmaS > 0.0f) ||
        (long long)H * W >= (1ll << 31))                 // pixel counts and key-map items are int
        return SMT_ERR_ARG;
    smt_adcensus *h = new (std::nothrow) smt_adcensus();
    if (!h) return SMT_ERR_ALLOC;
    h->device = smt_current_device();
    h->H = H; h->W = W; h->D = D; h->sigmaC = sigmaC; h->sigmaS = sigmaS;
    h->stream = nullptr; h->timing = false; h->force_generic = false; h->ev = nullptr; h->n_timed = 0; h->n_seen = 0; h->timing_stride = 1; h->ev_merged = nullptr;
    const size_t N = (size_t)H * W, V = N * D;
    const int WX = W + 4;
    int rc = place_volumes(h, !(flags & SMT_ADCENSUS_NO_PLACEMENT_SEARCH));
    auto alloc = [&](void **p, size_t bytes) { if (rc == SMT_OK) rc = smt_malloc(p, bytes); };
    alloc((void **)&h->TS[0].lut, 320 * 4);
    alloc((void **)&h->TS[0].rank, RANK_N * 2);
    alloc((void **)&h->TS[0].flag, 4);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) {
        h->TS[t].WX = WX;
        h->TS[t].stamp = nullptr;
        h->TS[t].lut = h->TS[0].lut;                     // shared
        h->TS[t].rank = h->TS[0].rank;
        h->TS[t].flag = h->TS[0].flag;
        for (int v = 0; v < 2; v++) {
            alloc((void **)&h->TS[t].cenA[v], N * 8);
            alloc((void **)&h->TS[t].cenX[v], (size_t)H * WX * 8);
            alloc((void **)&h->TS[t].u8[v], N);
        }
        alloc((void **)&h->TS[t].mask, N * 8);
    }
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) alloc((void **)&h->skeys[t], N * 8);
    h->T = h->TS[0];
    if (rc != SMT_OK) { smt_adcensus_destroy(h); return rc; }
    if (hipStreamCreateWithFlags(&h->prep_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->chain2_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->in_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming) != hipSuccess) {
        smt_adcensus_destroy(h);
        return SMT_ERR_HIP;
    }
    for (int c = 1; c < SMT_MAX_CHAINS; c++)
        if (hipEventCreateWithFlags(&h->join_ev[c], hipEventDisableTiming) != hipSuccess) {
            smt_adcensus_destroy(h);
            return SMT_ERR_HIP;
        }
    for (int t = 0; t < 2; t++)
        if (hipEventCreateWithFlags(&h->prep_done[t], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->cost_done[t], hipEventDisableTiming) != hipSuccess) {
            smt_adcensus_destroy(h);
            return SMT_ERR_HIP;
        }
    float lut[320];
    build_lut(sigmaC, sigmaS, lut);
    uint16_t *rank = new (std::nothrow) uint16_t[RANK_N];
    if (!rank || !build_rank(lut, rank)) { delete[] rank; smt_adcensus_destroy(h); return SMT_ERR_ALLOC; }
    const bool rank_ok = hipMemcpy(h->TS[0].rank, rank, RANK_N * 2, hipMemcpyHostToDevice) == hipSuccess;
    delete[] rank;
    // the reference's `new float[size*dispRange]()` value-initialises the volumes (AD-Census.h:341-342):
    // GetPtrLeft/Right before the first Compute* reads zeros
    if (!rank_ok || hipMemcpy(h->TS[0].lut, lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(h->vol[0], 0, V * 4) != hipSuccess || hipMemset(h->vol[1], 0, V * 4) != hipSuccess ||
        hipMemset(h->TS[0].flag, 0, 4) != hipSuccess) {
        smt_adcensus_destroy(h);
        return SMT_ERR_HIP;
    }
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++)
        if (hipMemset(h->skeys[t], 0xFF, N * 8) != hipSuccess) { smt_adcensus_destroy(h); return SMT_ERR_HIP; }
    calibrate_store_mode(h, !(flags & SMT_ADCENSUS_NO_STORE_CALIBRATION));
    set_maps_resident(h);
    *out = h;
    return SMT_OK;
}

SMT_API int smt_adcensus_create(int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out)
{
    return adcensus_create(H, W, D, sigmaC, sigmaS, 0u, out);
}

SMT_API int smt_adcensus_create_ex(int device, int H, int W, int D, float sigmaC, float sigmaS, unsigned flags, smt_adcensus **out)
{
    if (flags & ~(unsigned)(SMT_ADCENSUS_NO_PLACEMENT_SEARCH | SMT_ADCENSUS_NO_STORE_CALIBRATION)) return SMT_ERR_ARG;
    if (device < 0) return adcensus_create(H, W, D, sigmaC, sigmaS, flags, out);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return adcensus_create(H, W, D, sigmaC, sigmaS, flags, out);
}

SMT_API int smt_adcensus_create_on(int device, int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(device);
    return smt_adcensus_create(H, W, D, sigmaC, sigmaS, out);
}

SMT_API int smt_adcensus_destroy(smt_adcensus *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    for (int c = 0; c < SMT_MAX_CHAINS; c++)                 // never pending here; chain_on is all 0: the handle's stream
        if (h->chain[c].conv_pending) { flush_conversion(h, c); (void)hipStreamSynchronize(h->stream); }
    if (h->prep_stream) { (void)hipStreamSynchronize(h->prep_stream); (void)hipStreamDestroy(h->prep_stream); }
    if (h->chain2_stream) { (void)hipStreamSynchronize(h->chain2_stream); (void)hipStreamDestroy(h->chain2_stream); }
    if (h->in_ready) (void)hipEventDestroy(h->in_ready);
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    for (int c = 1; c < SMT_MAX_CHAINS; c++)
        if (h->join_ev[c]) (void)hipEventDestroy(h->join_ev[c]);
    for (int t = 0; t < 2; t++) {
        if (h->prep_done[t]) (void)hipEventDestroy(h->prep_done[t]);
        if (h->cost_done[t]) (void)hipEventDestroy(h->cost_done[t]);
    }
    (void)hipFree(h->vol[0]); (void)hipFree(h->vol[1]);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) {
        for (int v = 0; v < 2; v++) {
            (void)hipFree(h->TS[t].cenA[v]); (void)hipFree(h->TS[t].cenX[v]); (void)hipFree(h->TS[t].u8[v]);
        }
        (void)hipFree(h->TS[t].mask);
    }
    (void)hipFree(h->TS[0].lut); (void)hipFree(h->TS[0].rank); (void)hipFree(h->TS[0].flag);
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) (void)hipFree(h->skeys[t]);
    if (h->ev) {
        for (int k = 0; k < SMT_TIMING_SLOTS * 4; k++) (void)hipEventDestroy(h->ev[k]);
        delete[] h->ev_merged;
        delete[] h->ev;
    }
    delete h;
    return SMT_OK;
}

SMT_API int smt_adcensus_set_stream(smt_adcensus *h, void *s)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->stream = smt_stream(s);
    return SMT_OK;
}

SMT_API int smt_adcensus_set_quirks(smt_adcensus *h, unsigned quirks)
{
    if (!h || (quirks & ~SMT_QUIRK_FIX_ALL)) return SMT_ERR_ARG;
    // every launch takes its Tables (this pair's and, for the table workgroups riding in a cost launch, the next
    // pair's) by value from these at issue time; no call leaves tables built for the next one
    const int col = (quirks & SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE) ? h->W - 1 : 0;
    h->T.edge_col = col;
    for (int t = 0; t < 2 * SMT_MAX_CHAINS; t++) h->TS[t].edge_col = col;
    return SMT_OK;
}

template <int C, bool FULL>
static void launch_cost(smt_adcensus *h, int view0, int nviews, float *d0, float *d1)
{
    const int D = h->D;
    dim3 grid((h->W + TJ - 1) / TJ, h->H, nviews);
    const int NX = TJ + D;
    size_t shm = (size_t)NX * 8 + TJ * 16 + 320 * 4 + NX + TJ;
    shm = (shm + 15) & ~(size_t)15;
    hipLaunchKernelGGL((k_cost<C, FULL>), grid, dim3(NT), shm, run_stream(h), h->H, h->W, D, h->T,
                       view0, h->vol[0], h->vol[1], d0, d1);
}

// The pair takes the shared form (k_cost_maps_shared); every other pair flushes a pending conversion first.
static bool pair_takes_shared(const smt_adcensus *h, int views, const float *dL, const float *dR, bool maps)
{
    if (!(views == SMT_VIEW_BOTH && maps) || h->force_generic || (h->D + 63) / 64 > 4) return false;
    return !maps_kernel_rank() && dL && dR && maps_shared_shape(h->W, h->D);
}

template <int C, bool FULL>
static void launch_fast(smt_adcensus *h, int views, float *dL, float *dR, const float *nL, const float *nR, bool maps)
{
    const int nbx = (h->W + FTJ - 1) / FTJ;
    auto blocks = [&](int nviews) { return dim3(cost_grid(nbx, h->H, nviews)); };
    ChainState &ch = h->chain[h->cur];
    const hipStream_t st = run_stream(h);
    if (views == SMT_VIEW_BOTH && maps) {
        // pair of a batch whose volumes nobody can read: maps only, the next pair's table workgroups (if any) fused in
        const int K = maps_chunks();
        int nprep = 0, ptx = 1;
        if (nL) nprep = prep_items(h->H, h->W, ptx);
        const Tables &Tn = h->TS[chain_slot(h->cur, ch.n_pairs + 1)];
        int n2, n1;
        if (pair_takes_shared(h, views, dL, dR, maps)) {
            // One launch on the chain's stream: the left-view runs, this pair's edge items, the table tiles of the
            // chain's next pair and the conversion of its previous shared pair.  This pair's own conversion stays pending.
            const int km = chain_slot(h->cur, ch.n_pairs);
            if (ch.conv_pending && ch.conv_map == km) flush_conversion(h, h->cur);   // cannot happen: shared pairs in a row alternate
            const bool carried = ch.conv_pending;
            maps_taper(h->beside ? 0 : h->maps_resident[0], ((long)nbx * h->H + 7) >> 3, K, n2, n1);
            const int ncs = maps_groups(nbx, h->H, 1, K, n2, n1), Dd = FULL ? 64 * C : h->D;
            const int cbody = maps_body_groups(nbx, h->H, 1, K, n2, n1);
            const int nconv = carried ? shared_conv_items(h->H, h->W) : 0, nedge = shared_edge_items(h->H, h->W, Dd);
            const unsigned gs = 8u * (unsigned)fused_grid(ncs, nprep + nconv + nedge, cbody).groups;
            hipLaunchKernelGGL((k_cost_maps_shared<C, FULL>), dim3(gs), dim3(NT), 0, st, h->H, h->W, h->D, h->T, dL, dR,
                               h->skeys[km], nbx, K, shared_pub_hi(h->W), ncs, nprep, nL, nR, Tn, ptx, nconv, nedge,
                               carried ? h->skeys[ch.conv_map] : nullptr, carried ? ch.conv_dR : nullptr, n2, n1, cbody);
            if (SMT_SHARED_KNOCKOUT != 2) { ch.conv_pending = true; ch.conv_map = km; ch.conv_dR = dR; }
            else ch.conv_pending = false;
            if (shared_finish_apart()) flush_conversion(h, h->cur);
            return;
        }
        const bool rank = maps_kernel_rank();
        maps_taper(h->beside ? 0 : h->maps_resident[rank ? 2 : 1], ((long)nbx * h->H * 2 + 7) >> 3, K, n2, n1);
        const int ncost = maps_groups(nbx, h->H, 2, K, n2, n1), cbody = maps_body_groups(nbx, h->H, 2, K, n2, n1);
        const unsigned grid = nL ? 8u * (unsigned)fused_grid(ncost, nprep, cbody).groups : (unsigned)ncost;
        if (rank)
            hipLaunchKernelGGL((k_cost_maps2p<C, FULL, MODE_MAPS_RANK>), dim3(grid), dim3(NT), 0, st, h->H, h->W,
                               h->D, h->T, dL, dR, nbx, K, ncost, nprep, nL, nR, Tn, ptx, n2, n1, cbody);
        else
            hipLaunchKernelGGL((k_cost_maps2p<C, FULL, MODE_MAPS_FLOAT>), dim3(grid), dim3(NT), 0, st, h->H, h->W,
                               h->D, h->T, dL, dR, nbx, K, ncost, nprep, nL, nR, Tn, ptx, n2, n1, cbody);
        return;
    }
    if (views == SMT_VIEW_BOTH && nL) {
        // this pair's cost workgroups + the next pair's table workgroups (into the other table set) in one launch
        const int ncost = (int)blocks(2).x;
        int ptx;
        const int nprep = prep_items(h->H, h->W, ptx);
        const unsigned grid = 8u * (unsigned)fused_grid(ncost, nprep).groups;
        const Tables &Tn = h->TS[chain_slot(h->cur, ch.n_pairs + 1)];
        if (h->plain_stores)
            hipLaunchKernelGGL((k_cost_fast2p<C, FULL, false>), dim3(grid), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                               h->vol[0], h->vol[1], dL, dR, nbx, ncost, nprep, nL, nR, Tn, ptx);
        else
            hipLaunchKernelGGL((k_cost_fast2p<C, FULL, true>), dim3(grid), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                               h->vol[0], h->vol[1], dL, dR, nbx, ncost, nprep, nL, nR, Tn, ptx);
        return;
    }
    if (views == SMT_VIEW_BOTH) {
        if (h->plain_stores)
            hipLaunchKernelGGL((k_cost_fast2<C, FULL, false>), blocks(2), dim3(NT), 0, st, h->H, h->W, h->D, h->T, h->vol[0],
                               h->vol[1], dL, dR, nbx);
        else
            hipLaunchKernelGGL((k_cost_fast2<C, FULL, true>), blocks(2), dim3(NT), 0, st, h->H, h->W, h->D, h->T, h->vol[0],
                               h->vol[1], dL, dR, nbx);
        return;
    }
    if (views & SMT_VIEW_LEFT)
        hipLaunchKernelGGL((k_cost_fast<C, 0, FULL>), blocks(1), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                           h->vol[0], dL, nbx);
    if (views & SMT_VIEW_RIGHT)
        hipLaunchKernelGGL((k_cost_fast<C, 1, FULL>), blocks(1), dim3(NT), 0, st, h->H, h->W, h->D, h->T,
                           h->vol[1], dR, nbx);
}

static bool launch_fast_as(int C, bool full, smt_adcensus *h, int views, float *dL, float *dR, const float *nL,
                           const float *nR, bool maps)
{
    return dispatch_c<4>(C, [&](auto c) {
        if (full) launch_fast<decltype(c)::value, true>(h, views, dL, dR, nL, nR, maps);
        else launch_fast<decltype(c)::value, false>(h, views, dL, dR, nL, nR, maps);
    });
}

// One pair into its chain's table set chain_slot(cur, n).  Three schedules for the pairs of a batch on chain 0, and the
// chained one (chain_plan below), which issues every pair as a `prepped` pair of the fused schedule on its chain:
//   fused (default, both views through the register-window kernel): the table workgroups of pair n + 1 ride in the
//     grid of pair n's cost kernel (k_cost_fast2p) -- one stream, one launch per pair, no events; `prepped` says this
//     pair's tables were built that way, `nL / nR` are the next pair's images (null for the last pair of a batch);
//   overlap (SMT_OVERLAP=1, and the schedule of single views / D > 256): the table kernels run on the handle's internal
//     stream beside the previous pair's cost kernel on the caller's stream; event edges:
//       cost_done[n-2] --> prep stream               (table set n&1 is free again)
//       prep_done[n]   --> caller stream --> cost kernel(s) --> cost_done[n]
//     only for pairs b >= 1 of a batch (their inputs were already ordered behind the caller's stream by pair 0);
//   in order on the caller's stream (single pairs, the first pair of a batch, SMT_OVERLAP=0).
// Measured on MI355X the overlap gives +18 % at 1242x375 D=256 and +2-3.5 % at 1920x1080 D=192 over the in-order form
// (the table kernels then take 0.09 instead of 0.04 ms, hidden behind a cost kernel that gets 1 % slower); the fused
// form against the overlap: DESIGN.md section 4.
static bool fast_both_views(const smt_adcensus *h, int views)
{
    return views == SMT_VIEW_BOTH && !h->force_generic && (h->D + 63) / 64 <= 4;
}

// The stand-alone table kernel of one pair: tile workgroups + the workgroups of the 13 border columns (16 rows each)
// in one launch.
static void launch_prep(const smt_adcensus *h, hipStream_t st, const float *L, const float *R, const Tables &T)
{
    int tx;
    const int items = prep_items(h->H, h->W, tx);            // a whole number of rows of tx workgroups
    hipLaunchKernelGGL(k_prep, dim3(tx, items / tx), dim3(PNT), 0, st, L, R, h->H, h->W, T);
}

// maps: the pair's volumes are not written (a batch pair before the last; fast_both_views only).
static int adcensus_pair(smt_adcensus *h, const float *L, const float *R, int views, float *dL,
                         float *dR, bool overlap, bool prepped = false, const float *nL = nullptr,
                         const float *nR = nullptr, bool maps = false)
{
    const int D = h->D;
    ChainState &ch = h->chain[h->cur];
    const int set = chain_slot(h->cur, ch.n_pairs);
    const hipStream_t st = run_stream(h);                    // the caller's stream unless a chain runs on an internal one
    h->T = h->TS[set];
    h->vol_pending = false;                                  // never observable: dropped with the tables they would come from
    if (!pair_takes_shared(h, views, dL, dR, maps)) flush_conversion(h, h->cur);
    const bool timed = h->timing && (h->n_seen++ % h->timing_stride) == 0;
    const long slot = h->n_timed % SMT_TIMING_SLOTS;
    hipEvent_t *ev = timed ? h->ev + 4 * slot : nullptr;
    // overlap == false: everything in order on the caller's stream (single pairs, first pair of a batch)
    hipStream_t ps = overlap ? h->prep_stream : st;          // overlap: chain 0 only, set is 0 or 1
    if (overlap && ch.n_pairs >= 2) SMT_HIP(hipStreamWaitEvent(ps, h->cost_done[set], 0));
    if (timed) (void)hipEventRecord(ev[0], ps);
    if (!prepped) launch_prep(h, ps, L, R, h->T);
    if (timed) (void)hipEventRecord(ev[1], ps);
    if (overlap) {
        SMT_HIP(hipEventRecord(h->prep_done[set], ps));
        SMT_HIP(hipStreamWaitEvent(st, h->prep_done[set], 0));
    }
    // one stream: the event after the table kernels is also the cost kernel's start
    if (timed) { h->ev_merged[slot] = !overlap; if (overlap) (void)hipEventRecord(ev[2], st); }
    const int view0 = (views & SMT_VIEW_LEFT) ? 0 : 1;
    const int nviews = (views == SMT_VIEW_BOTH) ? 2 : 1;
    const int C = (D + 63) / 64;
    const bool full = (D % 64) == 0;
    if (h->force_generic || C > 4) {
        // the table-lookup kernel of the first version: kept as an independent formulation, and the kernel for
        // 256 < D <= 512 (a lane then owns 5..8 consecutive hypotheses; the register-window kernel stops at 4)
        (void)dispatch_c<SMT_MAX_DISPARITY / 64>(C, [&](auto c) { launch_cost<decltype(c)::value, false>(h, view0, nviews, dL, dR); });
    } else if (!launch_fast_as(C, full, h, views, dL, dR, nL, nR, maps)) return SMT_ERR_ARG;
    if (timed) { (void)hipEventRecord(ev[3], st); h->n_timed++; }
    // the two-stream schedule waits on this before it reuses the table set; the fused one is ordered by its stream and
    // a chain > 0 by the call's join
    if (!prepped && !nL && h->cur == 0) SMT_HIP(hipEventRecord(h->cost_done[set], st));
    ch.n_pairs++;
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

SMT_API int smt_adcensus_compute(smt_adcensus *h, const float *L, const float *R, int views,
                                 float *dispL, float *dispR)
{
    if (!h || !L || !R || views < 1 || views > 3) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    return adcensus_pair(h, L, R, views, dispL, dispR, false);
}

// schedule of the pairs b >= 1 of a batch: 0 in order, 1 two streams, 2 fused launches (adcensus_pair), 3 fused
// launches in chains (chain_plan); smt_adcensus_compute_batch keeps 2 where 3 does not apply
static int batch_schedule(const smt_adcensus *h, int views)
{
    const int forced = overlap_env();                        // tuning hook: SMT_OVERLAP = 0 / 1 / 2 / 3 forces the choice
    int want = forced >= 0 ? forced : SMT_CHAINED_DEFAULT ? 3 : 2;
    if (want >= 2 && !fast_both_views(h, views)) want = 1;
    return want;
}

// Schedule 3 of adcensus_batch_pairs: issues chain_plan's list.  Events only, no host synchronisation.  Whatever
// happens, every chain's pending conversion is issued and every internal stream that was given work is joined into the
// caller's stream before this returns, ahead of anything else the caller's stream gets.
static int adcensus_batch_chained(smt_adcensus *h, const float *L, const float *R, int n, int views, float *dispL,
                                  float *dispR, bool last_volumes)
{
    const size_t N = (size_t)h->H * h->W;
    unsigned flags = 0;
    if (pair_takes_shared(h, views, dispL, dispR, true)) flags |= CHAIN_SHARED;
    if (last_volumes) flags |= CHAIN_LAST_VOLUMES;
    if (chain_fork_start()) flags |= CHAIN_FORK_START;
    if (shared_finish_apart()) flags |= CHAIN_FINISH_APART;
    long count0[SMT_MAX_CHAINS];
    for (int c = 0; c < SMT_MAX_CHAINS; c++) count0[c] = h->chain[c].n_pairs;
    std::vector<ChainOp> ops;
    const int nc = chain_count(), order = chain_order(), taper = chain_taper();
    int rc = chain_plan(n, nc, count0, order, flags, ops);
    if (rc != SMT_OK) return rc;
    const bool concurrent = order == CHAIN_ORDER_BESIDE && std::min(nc, n) >= 2;
    auto internal = [&](int s) { return s == 1 ? h->prep_stream : h->chain2_stream; };
    auto stream = [&](int s) { return s == 0 ? h->stream : internal(s); };
    bool open[SMT_MAX_CHAINS] = {false, false, false};       // internal stream s has work that no join event covers yet
    int last_set = 0;
    auto issue = [&](const ChainOp &o) -> int {
        if (o.stream > 0 && o.kind != CH_RECORD) open[o.stream] = true;
        h->cur = o.chain;
        h->chain_on[o.chain] = o.kind == CH_RECORD || o.kind == CH_WAIT ? h->chain_on[o.chain] : o.stream;
        switch (o.kind) {
        case CH_PREP:
            launch_prep(h, stream(o.stream), L + o.pair * N, R + o.pair * N, h->TS[o.ts_built]);
            return SMT_OK;
        case CH_PAIR: {
            const int b = o.pair;
            if (chain_slot(o.chain, h->chain[o.chain].n_pairs) != o.ts_read) return SMT_ERR_STATE;   // plan and state disagree
            if (b + 1 == n) last_set = o.ts_read;
            h->beside = concurrent && (taper == CHAIN_TAPER_NONE || (taper == CHAIN_TAPER_LAST && b + 1 < n));
            return adcensus_pair(h, L + b * N, R + b * N, views, dispL ? dispL + b * N : nullptr,
                                 dispR ? dispR + b * N : nullptr, false, true,
                                 o.ts_built >= 0 ? L + o.built_for * N : nullptr,
                                 o.ts_built >= 0 ? R + o.built_for * N : nullptr, !(b + 1 == n && last_volumes));
        }
        case CH_CONVERT:
            flush_conversion(h, o.chain);
            return SMT_OK;
        case CH_RECORD:
            SMT_HIP(hipEventRecord(o.ev ? h->join_ev[o.ev] : h->fork_ev, stream(o.stream)));
            if (o.stream > 0) open[o.stream] = false;
            return SMT_OK;
        default:
            SMT_HIP(hipStreamWaitEvent(stream(o.stream), o.ev ? h->join_ev[o.ev] : h->fork_ev, 0));
            return SMT_OK;
        }
    };
    for (size_t k = 0; k < ops.size() && rc == SMT_OK; k++) rc = issue(ops[k]);
    if (rc != SMT_OK) {
        // an error path: what the plan had not issued yet of conversions and joins.  Waiting on a join event a second
        // time is harmless; an event recorded again is waited on again.
        for (int c = 0; c < SMT_MAX_CHAINS; c++) flush_conversion(h, c);
        for (int s = 1; s < SMT_MAX_CHAINS; s++) {
            bool used = open[s];
            for (int c = 0; c < SMT_MAX_CHAINS; c++) used = used || h->chain_on[c] == s;
            if (!used) continue;
            (void)hipEventRecord(h->join_ev[s], internal(s));
            (void)hipStreamWaitEvent(h->stream, h->join_ev[s], 0);
        }
    } else {
        h->T = h->TS[last_set];                              // the deferred volumes come from the last pair's tables
    }
    h->cur = 0;
    h->beside = false;
    for (int c = 0; c < SMT_MAX_CHAINS; c++) h->chain_on[c] = 0;
    if (rc != SMT_OK) return rc;
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

// The per-pair loop of a batch (adcensus_internal.h).  Pair b >= 1 follows `sched`; pair 0 is in order, with its tables
// already built when `prepped`; with sched 2 the last pair builds the tables of (nL, nR) inside its launch when they are
// given.  With `maps_ok` and fast_both_views the pairs take the maps-only kernel, all but the last when `last_volumes`
// is set (the last one then leaves its volumes in the handle), every pair when it is clear.
int adcensus_batch_pairs(smt_adcensus *h, const float *L, const float *R, int n, int views, float *dispL,
                         float *dispR, int sched, bool prepped, const float *nL, const float *nR, bool maps_ok,
                         bool last_volumes)
{
    const size_t N = (size_t)h->H * h->W;
    maps_ok = maps_ok && fast_both_views(h, views);
    if (sched == 3) {
        if (maps_ok && n >= 2 && !prepped && !nL && !nR)
            return adcensus_batch_chained(h, L, R, n, views, dispL, dispR, last_volumes);
        sched = 2;                                           // every pair stores the handle's two volumes, or a host-fed chunk
    }
    for (int b = 0; b < n; b++) {
        const bool last = b + 1 == n;
        const float *bl = sched == 2 ? (last ? nL : L + (b + 1) * N) : nullptr;
        const float *br = sched == 2 ? (last ? nR : R + (b + 1) * N) : nullptr;
        int rc = adcensus_pair(h, L + b * N, R + b * N, views, dispL ? dispL + b * N : nullptr,
                               dispR ? dispR + b * N : nullptr, sched == 1 && b > 0, b > 0 ? sched == 2 : prepped,
                               bl, br, maps_ok && (!last || !last_volumes));
        if (rc != SMT_OK) { flush_conversion(h, 0); return rc; }
    }
    // the last shared pair has no next launch; the caller may read or free its maps behind this call
    flush_conversion(h, 0);
    SMT_LAUNCH_CHECK();
    return SMT_OK;
}

bool adcensus_fused_both_views(const smt_adcensus *h) { return fast_both_views(h, SMT_VIEW_BOTH); }

// The volumes of a batch's deferred last pair, written now: the both-views cost kernel with null maps on the pair's
// tables (h->T, see vol_pending), on the handle's stream behind the batch's launches -- where an eager last pair would
// have stored them -- and waits for it.  The cost kernels do not touch the domain flag (k_prep raises it), so smt_adcensus_status reports
// what it would have.  With timing on, the launch is recorded like a pair whose tables were already built.
static int materialise_volumes(smt_adcensus *h)
{
    flush_conversion(h, 0);                                  // never pending here: no entry point leaves one
    if (!h->vol_pending) return SMT_OK;
    const long slot = h->n_timed % SMT_TIMING_SLOTS;
    hipEvent_t *ev = h->timing ? h->ev + 4 * slot : nullptr;
    if (ev) { (void)hipEventRecord(ev[0], h->stream); (void)hipEventRecord(ev[1], h->stream); h->ev_merged[slot] = true; }
    if (!launch_fast_as((h->D + 63) / 64, h->D % 64 == 0, h, SMT_VIEW_BOTH, nullptr, nullptr))
        return SMT_ERR_STATE;                                // only fast_both_views pairs are deferred
    if (ev) { (void)hipEventRecord(ev[3], h->stream); h->n_timed++; }
    h->vol_pending = false;
    SMT_LAUNCH_CHECK();
    // A caller that synchronised the stream after its batch could read an eager last pair's volumes from anywhere;
    // keep that true.  This happens at most once per handle: after the first lend nothing is deferred.
    SMT_HIP(hipStreamSynchronize(h->stream));
    return SMT_OK;
}

SMT_API int smt_adcensus_compute_batch(smt_adcensus *h, const float *L, const float *R, int pairs,
                                       int views, float *dispL, float *dispR)
{
    if (!h || !L || !R || pairs <= 0 || views < 1 || views > 3) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    const int sched = pairs > 1 ? batch_schedule(h, views) : 0;
    if (sched == 1) {
        // order the internal stream behind whatever produced the [pairs][H][W] inputs
        SMT_HIP(hipEventRecord(h->in_ready, h->stream));
        SMT_HIP(hipStreamWaitEvent(h->prep_stream, h->in_ready, 0));
    }
    // Only the last pair's volumes stay readable (every pair writes the same two), so pairs 0 .. pairs-2 of the
    // both-views register-window path take the maps-only kernel.  The last pair takes it too while no volume pointer
    // of this handle has been lent (nobody can read them yet): its volumes are then pending, written by
    // smt_adcensus_volume if it is called before the next compute.  SMT_BATCH_VOLUMES in the environment (read at
    // every call): `last` writes the last pair's volumes in the batch itself whatever has been lent, `all` writes
    // every pair's, as the first versions did: same-process A/Bs and tests.
    const char volumes = batch_volumes_env();
    const bool all_volumes = volumes == 'a';
    const bool defer = !volumes && !h->vol_lent && fast_both_views(h, views);
    const int rc = adcensus_batch_pairs(h, L, R, pairs, views, dispL, dispR, sched, false, nullptr, nullptr, !all_volumes, !defer);
    h->vol_pending = defer && rc == SMT_OK;
    return rc;
}

SMT_API int smt_adcensus_volume(smt_adcensus *h, int view, float **vol)
{
    if (!h || !vol || (view != SMT_VIEW_LEFT && view != SMT_VIEW_RIGHT)) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    // lending is for good: a pointer handed out stays valid until destroy, so nothing is deferred after this call
    h->vol_lent = true;
    const int rc = materialise_volumes(h);
    if (rc != SMT_OK) return rc;
    *vol = h->vol[view == SMT_VIEW_LEFT ? 0 : 1];
    return SMT_OK;
}

SMT_API int smt_adcensus_status(smt_adcensus *h)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    int f = 0;
    SMT_HIP(hipMemcpyAsync(&f, h->T.flag, 4, hipMemcpyDeviceToHost, h->stream));
    SMT_HIP(hipMemsetAsync(h->T.flag, 0, 4, h->stream));            // read-and-clear
    SMT_HIP(hipStreamSynchronize(h->stream));
    return f ? SMT_ERR_DOMAIN : SMT_OK;
}

SMT_API int smt_adcensus_force_generic(smt_adcensus *h, int on)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    h->force_generic = on != 0;
    return SMT_OK;
}

SMT_API int smt_adcensus_timing(smt_adcensus *h, int enable)
{
    if (!h) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (enable && !h->ev) {
        h->ev = new (std::nothrow) hipEvent_t[SMT_TIMING_SLOTS * 4];
        h->ev_merged = new (std::nothrow) bool[SMT_TIMING_SLOTS]();
        if (!h->ev || !h->ev_merged) return SMT_ERR_ALLOC;
        for (int k = 0; k < SMT_TIMING_SLOTS * 4; k++) SMT_HIP(hipEventCreate(&h->ev[k]));
    }
    if (enable < 0) return SMT_ERR_ARG;
    h->timing = enable != 0;
    h->timing_stride = enable > 0 ? enable : 1;
    h->n_timed = 0;
    h->n_seen = 0;
    return SMT_OK;
}

SMT_API int smt_adcensus_kernel_times(smt_adcensus *h, float *prep_ms, float *cost_ms, int capacity,
                                      int *count)
{
    if (!h || !count || capacity < 0) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    if (!h->ev) return SMT_ERR_STATE;
    long n = h->n_timed < SMT_TIMING_SLOTS ? h->n_timed : SMT_TIMING_SLOTS;
    if (n > capacity) n = capacity;
    const long first = h->n_timed - n;
    for (long k = 0; k < n; k++) {
        hipEvent_t *ev = h->ev + 4 * ((first + k) % SMT_TIMING_SLOTS);
        SMT_HIP(hipEventSynchronize(ev[3]));
        float a = 0, b = 0;
        SMT_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));      // table kernels, internal stream
        const long slot = (first + k) % SMT_TIMING_SLOTS;
        SMT_HIP(hipEventElapsedTime(&b, ev[h->ev_merged[slot] ? 1 : 2], ev[3]));   // cost kernel(s), caller's stream
        if (prep_ms) prep_ms[k] = a;
        if (cost_ms) cost_ms[k] = b;
    }
    *count = (int)n;
    return SMT_OK;
}

// Measurement hook (bench.py): see include/smt.h.
namespace {
// everything smt_adcensus_diag_impl acquires, released on every exit path (its SMT_HIP early returns included)
struct DiagResources {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    unsigned long long *stamp = nullptr;
    unsigned long long *hs = nullptr;
    float *ratio = nullptr;
    ~DiagResources()
    {
        for (auto &x : e) if (x) (void)hipEventDestroy(x);
        if (stamp) (void)hipFree(stamp);
        delete[] hs;
        delete[] ratio;
    }
};
}  // namespace

static int smt_adcensus_diag_impl(smt_adcensus *h, int reps, float *sclk_mhz, float *cost_ms, float *store_only_ms, DiagResources &res)
{
    if (h->chain[0].n_pairs == 0) return SMT_ERR_STATE;      // needs the tables of a computed pair
    const int D = h->D, C = D / 64;
    if (D % 64 != 0 || C < 1 || C > 4) return SMT_ERR_ARG;
    const int nbx = (h->W + FTJ - 1) / FTJ;
    const unsigned nblk = cost_grid(nbx, h->H, 2);
    hipEvent_t (&e)[3] = res.e;
    for (auto &x : e) SMT_HIP(hipEventCreate(&x));
    if (smt_malloc((void **)&res.stamp, (size_t)nblk * 32) != SMT_OK) return SMT_ERR_ALLOC;
    unsigned long long *stamp = res.stamp;
    SMT_HIP(hipMemsetAsync(stamp, 0, (size_t)nblk * 32, h->stream));
    Tables T = h->T;
    T.stamp = stamp;
    SMT_HIP(hipEventRecord(e[0], h->stream));
    for (int r = 0; r < reps; r++) store_only(h, h->vol[0], h->vol[1], h->stream);
    SMT_HIP(hipEventRecord(e[1], h->stream));
    // the real kernel with stamps, last, so that the volumes hold the pair's costs again afterwards
    for (int r = 0; r < reps; r++)
        (void)dispatch_c<4>(C, [&](auto c) {
            constexpr int CC = decltype(c)::value;
            if (h->plain_stores) hipLaunchKernelGGL((k_cost_fast2<CC, true, false>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
            else hipLaunchKernelGGL((k_cost_fast2<CC, true, true>), dim3(nblk), dim3(NT), 0, h->stream, h->H, h->W, D, T, h->vol[0], h->vol[1], (float *)nullptr, (float *)nullptr, nbx);
        });
    SMT_HIP(hipEventRecord(e[2], h->stream));
    SMT_LAUNCH_CHECK();
    h->vol_pending = false;                                  // the stamped launches have just written the pair's volumes
    SMT_HIP(hipEventSynchronize(e[2]));
    float a = 0, b = 0;
    SMT_HIP(hipEventElapsedTime(&a, e[0], e[1]));
    SMT_HIP(hipEventElapsedTime(&b, e[1], e[2]));
    if (store_only_ms) *store_only_ms = a / reps;
    if (cost_ms) *cost_ms = b / reps;
    if (sclk_mhz) {
        // stamps of the last launch: median over workgroups of d(s_memtime) / d(s_memrealtime) * 100 MHz
        unsigned long long *hs = res.hs = new (std::nothrow) unsigned long long[(size_t)nblk * 4];
        float *ratio = res.ratio = new (std::nothrow) float[nblk];
        if (!hs || !ratio) return SMT_ERR_ALLOC;
        SMT_HIP(hipMemcpy(hs, stamp, (size_t)nblk * 32, hipMemcpyDeviceToHost));
        size_t n = 0;
        for (unsigned k = 0; k < nblk; k++) {
            const unsigned long long dt = hs[4 * k + 2] - hs[4 * k], dr = hs[4 * k + 3] - hs[4 * k + 1];
            if (hs[4 * k + 3] != 0 && dr >= 200) ratio[n++] = (float)((double)dt / (double)dr * 100.0);
        }
        if (n) { std::nth_element(ratio, ratio + n / 2, ratio + n); *sclk_mhz = ratio[n / 2]; }
        else *sclk_mhz = 0.0f;
    }
    return SMT_OK;
}

SMT_API int smt_adcensus_diag(smt_adcensus *h, int reps, float *sclk_mhz, float *cost_ms, float *store_only_ms)
{
    if (!h || reps <= 0 || reps > 1000) return SMT_ERR_ARG;
    smt_dev_guard dev_guard(h->device);
    DiagResources res;
    return smt_adcensus_diag_impl(h, reps, sclk_mhz, cost_ms, store_only_ms, res);
}
