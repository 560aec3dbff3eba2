/*
 * smt.h -- C ABI of the MI355X-native dense stereo cost-volume engine (libsmt_hip.so).
 *
 * This is the drop-in boundary for the per-pixel x per-disparity hot path of
 * Asherchi/Stereo_Match_Traditional.  The reference has no FFI of its own: its
 * boundary is the set of C++ entry points its five main()s call with raw buffers
 * (SURVEY.md 8b).  Each entry point below names the reference function(s) it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the C++ shim a
 * maintainer of the reference would add to route those calls here.
 *
 * Conventions
 *   - plain C types only; every image / map / volume pointer is a DEVICE pointer (HIP
 *     global memory) owned by the caller unless stated otherwise.  smt_malloc /
 *     smt_memcpy_* are provided for hosts that have no allocator of their own.
 *   - images  [H][W] row-major; volumes [H][W][D], d fastest, float32 -- the reference
 *     layout (AD-CensusV1/AD-Census.h:87).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream unless documented as synchronising.  tests/test_stream_order_gpu.py holds every entry
 *     point that takes device buffers to this sentence: called on a busy stream with inputs that arrive behind the work
 *     in front of them, it computes what it computes on an idle one, and returns before the stream has drained unless
 *     its comment ends with "Synchronising." (the decisions: tests/stream_order_cases.py).
 *   - every function returns SMT_OK (0) or a negative smt_status.  The reference
 *     validates nothing (void functions, UB on bad sizes); this ABI rejects bad
 *     arguments instead.
 *   - handles are thread-compatible, not thread-safe (the reference objects hold
 *     mutable state too, e.g. CrossArm.h:34 `_tao`).
 *   - reference defects that change results are reproduced by default; see the
 *     SMT_QUIRK_* flags.
 *   - caller buffers.  A pointer needs the natural alignment of its element type (1 byte for uint8, 4 for float32 /
 *     int32, 8 for float64) and nothing coarser: kernels that fetch caller bytes as dwords or volumes as 16-byte
 *     vectors do so with unaligned global accesses, none requires 16-byte alignment of a caller pointer.  No byte
 *     outside the documented extents of a buffer is written -- not in front of it, not behind it, not in the gap
 *     between two maps of a strided batch -- and inputs (const pointers) are not written at all.  Outputs are fully
 *     defined: every element of every non-NULL output is written by the call, whatever the buffer held before,
 *     including the elements the reference leaves untouched (their value is stated per entry: 0 in the border of
 *     smt_ncc's map and cost volume, in the last row / column of SAD's right view, 0 / NaN in the costVolume[-1]
 *     columns of ASW's).  Nothing outside an input's extents reaches a result, and neither does what the library's
 *     scratch arena held before the call (smt_scratch_poison).  tests/test_bounds_gpu.py holds every entry point
 *     that takes device buffers to this paragraph.
 */
#ifndef SMT_H_
#define SMT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMT_VERSION 100 /* 0.1.0 */

typedef enum smt_status {
    SMT_OK = 0,
    SMT_ERR_ARG = -1,     /* null pointer / non-positive size / unsupported parameter */
    SMT_ERR_HIP = -2,     /* a HIP runtime call failed (smt_last_hip_error has the code) */
    SMT_ERR_ALLOC = -3,   /* device allocation failed */
    SMT_ERR_DOMAIN = -4,  /* image values outside the integer 0..255 domain the path assumes */
    SMT_ERR_REF_UB = -5,  /* inputs for which the reference's behaviour is undefined */
    SMT_ERR_STATE = -6    /* call order violated (e.g. aggregate before arms) */
} smt_status;

/* Reference-defect switches.  Default (0) = reference-faithful. */
#define SMT_QUIRK_FIX_RIGHT_ARM_STRIDE 0x1u /* undo `col = _row` in ComputeRightArmLength (CrossArm.cpp:265) */
/* the arm threshold is local to one arm walk: every walk starts at tau and uses tau_low from iteration
 * sec_length + 1 on, instead of one `_tao` that stays lowered for every later pixel and direction (CrossArm.cpp:223-225) */
#define SMT_QUIRK_FIX_STICKY_TAU 0x2u
/* the up / down scanline passes run the recurrence of the left / right ones along a column: last[d-1] for the "d-1"
 * term, the guide read at the pixel itself, grayLast updated every step (ScanlineOptimizer.h:210, :221/:250, :238) */
#define SMT_QUIRK_FIX_SCAN_VERTICAL 0x4u
/* the right view's census replicates column W-1 for neighbours past the right edge, as the left view replicates
 * column 0, instead of reading column 0 (AD-Census.h:242-243) */
#define SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE 0x8u
#define SMT_QUIRK_FIX_ALL (SMT_QUIRK_FIX_RIGHT_ARM_STRIDE | SMT_QUIRK_FIX_STICKY_TAU | SMT_QUIRK_FIX_SCAN_VERTICAL | \
                           SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE)
/* Every entry that takes quirks accepts any combination of the four and acts on the flags of its own stage; another
 * bit gives SMT_ERR_ARG. */

/* views bit mask */
#define SMT_VIEW_LEFT 1
#define SMT_VIEW_RIGHT 2
#define SMT_VIEW_BOTH 3

const char *smt_strerror(int status);
int smt_version(void);
int smt_last_hip_error(void);
int smt_device_count(int *count);
int smt_set_device(int device);
/* Devices.  A handle lives on the HIP device that was current in the calling thread when it was created
 * (smt_*_create) or on the one named explicitly (smt_*_create_on(device, ...), same arguments otherwise);
 * its entry points make that device current for the duration of the call and restore the caller's, so
 * one host thread can drive a handle per GPU.  Buffers and streams passed to a handle must belong to its
 * device.  The stateless entry points (smt_wta, smt_lrcheck, smt_sad, ...) run on the device that is
 * current in the calling thread.
 *
 * Limits (the reference has none; outside them SMT_ERR_ARG):  dispRange D <= SMT_MAX_DISPARITY = 512 on the
 * AD-Census pipeline (smt_adcensus_*, smt_wta, smt_crossarm_*, smt_scanline_*, smt_pipeline_*: one wavefront
 * spans the disparity axis, a lane owns up to 8 consecutive hypotheses; the tuned kernels cover D <= 256, beyond
 * it the first-version kernels run -- the table-lookup cost kernel, the one-pixel-per-wave rectangle walk, the
 * predicated scanline passes -- with the same results, untuned), and D <= SMT_MAX_DISPARITY on the window matchers and
 * the CrossAggregator (smt_sad*, smt_ncc*, smt_asw*, smt_crossagg_*, smt_adcensus_option_aggregate: tuned kernels at
 * every D -- 5..8 hypothesis slots per lane in SAD, NCC and the CrossAggregator, ASW in chunks of 256 hypotheses with
 * WinTakeAll's state carried between them; the same rules and bits as below 256).  The CBLSM helpers (smt_cblsm_*)
 * have no cap of their own (one thread per pixel and hypothesis).  ASW window side
 * 2*(winSize+1)+1 <= 64 (winSize <= 30; one window row per wavefront pass); MedianFilter wnd_size <= 7;
 * volumes of 4 GiB or more take the plain one-pixel-per-wave aggregation kernel (32-bit tap offsets in
 * the shared-tap kernels).  Image size: H * W < 2^31 everywhere (pixel indices are int: smt_adcensus_create*,
 * smt_crossarm_create*, smt_scanline_create*, smt_wta, smt_ncc and the batch and post-processing entry points reject
 * more); hypothesis addresses are 64-bit, so a volume of H * W * D elements may pass 2^31 elements and 2^32 bytes
 * (tests/test_large_volume_gpu.py runs every volume stage at 4 GiB to 8 GiB; DESIGN.md section 2, "Large volumes").
 * The one-thread-per-hypothesis CBLSM helpers take up to 2^39 hypotheses (the grid size). */

#define SMT_MAX_DISPARITY 512

/* ---- device memory helpers (plumbing; not part of the reference's surface) ---------- */
int smt_malloc(void **dptr, size_t bytes);
int smt_free(void *dptr);
int smt_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int smt_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int smt_memset(void *dst_dev, int byte, size_t bytes, void *stream);
int smt_stream_create(void **stream);
int smt_stream_destroy(void *stream);
int smt_stream_sync(void *stream); /* synchronising */

/* float64 sum of a float32 device array into *out_dev (device double; zeroed on the stream first) -- the
 * per-device term of the gather checksum of the batched multi-GPU configuration. */
int smt_sum_f32(const float *x, size_t n, double *out_dev, void *stream);

/* ---- kernel timing (bench.py roofline leg) ----------------------------------------------
 * When enabled, every N-th pair processed on the handle records HIP events -- around the table
 * kernels and around the cost kernel(s), each on the stream the kernels are launched on -- into a ring
 * of `SMT_TIMING_SLOTS` slots (a pair whose tables were built inside the previous pair's cost launch,
 * smt_adcensus_compute_batch, reports ~0 for them); nothing synchronises until
 * smt_adcensus_kernel_times, which waits for the last event and returns the per-pair
 * durations in milliseconds, oldest first. */
#define SMT_TIMING_SLOTS 1024
typedef struct smt_adcensus smt_adcensus;
int smt_adcensus_timing(smt_adcensus *h, int enable); /* 0 off, N > 0: record every N-th pair; also clears the ring */
int smt_adcensus_kernel_times(smt_adcensus *h, float *prep_ms, float *cost_ms, int capacity,
                              int *count);

/* Measurement hook (bench.py roofline leg; not part of the reference's surface).  Needs a pair already
 * computed on the handle and D = 64, 128, 192 or 256.  On the handle's stream it runs `reps` launches of
 * a store-only twin of the both-views cost kernel (identical grid, chunk order and streaming stores into
 * the handle's own volumes, no arithmetic) and then `reps` launches of the real kernel with in-kernel
 * counter stamps, and returns
 *   sclk_mhz       median over workgroups of d(s_memtime)/d(s_memrealtime) x 100 MHz inside the last
 *                  stamped launch = the shader clock the cost kernel actually ran at,
 *   cost_ms        mean duration of the stamped launches (no WTA maps are written),
 *   store_only_ms  mean duration of the store-only launches = the store ceiling of this pattern in
 *                  this process on these buffers.
 * Any of the three may be NULL.  The volumes hold the last pair's costs again on return.  Synchronising. */
int smt_adcensus_diag(smt_adcensus *h, int reps, float *sclk_mhz, float *cost_ms, float *store_only_ms);

/* =====================================================================================
 * AD-Census cost volume + WTA        replaces class AD_Census, AD-CensusV1/AD-Census.h
 * ===================================================================================== */

/* AD_Census::Initialize (AD-Census.h:322-344): fixes H, W, D, sigmaC (AD, `_sigmaC`) and
 * sigmaS (census, `_sigmaS`); allocates the left and right cost volumes (costVolume,
 * costVolumeRight) plus census tables.  The reference's separate AD / census volumes
 * (ADcostVolum, CensusVolum, ...) are never materialised. */
int smt_adcensus_create(int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out);
int smt_adcensus_create_on(int device, int H, int W, int D, float sigmaC, float sigmaS, smt_adcensus **out);
/* The same with the two measuring steps of Initialize under the caller's control (device < 0: the current one).
 * Without flags smt_adcensus_create allocates up to six candidate pairs of volumes (transiently 6 x 2 x 4*H*W*D
 * bytes: 19 GB at 1920x1080x192) to pick the placement with the fastest stores, and times the cost kernel with
 * streaming and with ordinary stores -- tens of milliseconds, worth it for a handle that lives for a batch, wrong
 * for a caller that creates a handle per request or shares the device:
 *   SMT_ADCENSUS_NO_PLACEMENT_SEARCH   keep the first allocation of the volumes
 *   SMT_ADCENSUS_NO_STORE_CALIBRATION  streaming stores without timing the alternative
 * (SMT_PLACEMENT=0 / SMT_STORE_MODE in the environment still do the same process-wide.) */
#define SMT_ADCENSUS_NO_PLACEMENT_SEARCH 0x1u
#define SMT_ADCENSUS_NO_STORE_CALIBRATION 0x2u
int smt_adcensus_create_ex(int device, int H, int W, int D, float sigmaC, float sigmaS, unsigned flags, smt_adcensus **out);
int smt_adcensus_destroy(smt_adcensus *h);
/* How smt_adcensus_create placed the two volumes: it allocates up to 6 candidate pairs, times a
 * store-only twin of the cost kernel on each and keeps the fastest (the HBM write rate of the same
 * kernel differs by ~18 % between allocations); SMT_PLACEMENT=0 in the
 * environment disables the search.  tries = candidate pairs allocated, store_only_ms = the kept pair's
 * store-only time (0 when there was no search).  Either pointer may be NULL. */
int smt_adcensus_placement(smt_adcensus *h, int *tries, float *store_only_ms);
/* Which stores the both-views cost kernel uses on this handle: smt_adcensus_create times the kernel a few
 * launches with streaming (non-temporal) and with ordinary stores and keeps ordinary ones only when they win by
 * more than 2 % (a device property like the placement; SMT_STORE_MODE=nt|plain in the environment fixes it).
 * plain = 1 / 0, nt_ms / plain_ms = the calibration times (0 when there was none).  Any pointer may be NULL. */
int smt_adcensus_store_mode(smt_adcensus *h, int *plain, float *nt_ms, float *plain_ms);
int smt_adcensus_set_stream(smt_adcensus *h, void *stream);
/* SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE, from the next smt_adcensus_compute / _compute_batch on (0 = faithful, the default).
 * Not the `flags` of smt_adcensus_create_ex: those are SMT_ADCENSUS_* values. */
int smt_adcensus_set_quirks(smt_adcensus *h, unsigned quirks);

/* ComputeADcensus (AD-Census.h:271-294) for SMT_VIEW_LEFT, ComputeADcensusRight
 * (:296-318) for SMT_VIEW_RIGHT, followed -- when dispL / dispR are non-NULL -- by
 * AD_Census::WTA (:346-380) fused into the same kernel.
 *   L, R        float32 [H][W], integer-valued 0..255 (main.cpp:46-55 builds them from
 *               uchar gray images); anything else raises SMT_ERR_DOMAIN at the next
 *               smt_adcensus_status.
 *   dispL/R     float32 [H][W] out, integer-valued, may be NULL. */
int smt_adcensus_compute(smt_adcensus *h, const float *L, const float *R, int views,
                         float *dispL, float *dispR);

/* Same, for a batch of `pairs` image pairs laid out [pairs][H][W]; the disparity maps are
 * [pairs][H][W].  The volumes are reused per pair and after the call hold the LAST pair's costs:
 * with both views and D <= 256 the volumes of pairs 0 .. pairs-2 are not written at all (those pairs
 * take a maps-only kernel; a view whose map is NULL then does no cost work), elsewhere they are
 * overwritten by the next pair.  There, until smt_adcensus_volume has been called on the handle once, the last
 * pair takes the maps-only kernel too and its volumes are written by the first smt_adcensus_volume call that
 * follows the batch (dropped if another compute comes first); once a pointer has been lent, every batch writes
 * its last pair's volumes itself.  SMT_BATCH_VOLUMES in the environment (read at every call), for
 * same-process comparisons: `last` writes the last pair's volumes in the batch whatever has been lent, `all`
 * writes every pair's.  This is the sharding unit of the multi-GPU configuration.  The census tables
 * are double-buffered inside the handle: with both views and D <= 256 the table workgroups of pair
 * b+1 are spread through the grid of pair b's cost launch (one launch per pair, one stream); single
 * views and D > 256 build them on an internal stream beside pair b's cost kernel.  SMT_OVERLAP =
 * 0 / 1 / 2 / 3 in the environment forces in-order / internal-stream / fused / chained (read at every call).
 * Chained (3, the default wherever the fused schedule would apply): the fused schedule on NC chains.  Pair b belongs to chain b % NC; a chain is the
 * fused schedule with a stride of NC on two table sets and two key maps of its own (its first pair's tables by a
 * stand-alone table kernel, pair b's launch carrying the tables of pair b + NC and the conversion of pair b - NC).
 * Chain 0 runs on the caller's stream, chain c > 0 on an internal non-blocking stream that waits for an event the
 * caller's stream records behind chain 0's table kernel, and the caller's stream waits for one event per internal
 * chain behind its last launch before the call returns: events only, the call stays asynchronous, and nothing of it is
 * pending or un-joined when it returns.  Launches of consecutive pairs then share the device, so one fills the other's
 * ramp and drain.  A call takes it where it would take the fused schedule, with pairs >= 2 and not under
 * SMT_BATCH_VOLUMES=all (every pair would store the same two volumes); else it keeps the fused one.  The maps are the
 * same bit for bit.  A last pair that writes its volumes does so on its chain's stream.  All chains' state is allocated
 * at create: 2 table sets and 2 key maps per chain, 84 H W + 128 H bytes for the sets and 16 H W for the maps, 207 MB
 * per chain at 1920 x 1080 (415 MB for the two extra chains) beside 3.2 GB of volumes at D = 192.
 *   SMT_CHAINS=<1..3> (read at every call; default 2; 3 is the maximum, a process has 4 hardware queues and the
 *   caller's stream is one).  SMT_CHAIN_FORK=start forks the internal streams from the start of the call instead
 *   (measurement).  SMT_CHAIN_ORDER=pairs|ab|ba (tests) keeps every chain's state indexing and changes the order on
 *   the device: every chain on the caller's stream in pair order / chain c + 1 behind the whole of chain c / chain 0
 *   behind the whole of the internal chains.  SMT_CHAIN_TAPER=all|last|none (measurement; default none): which
 *   launches of a chained call keep the tapered tail's default rule -- beside another chain's launch a launch has no
 *   drain of its own to recover ("Tapered tail" below; SMT_MAPS_TAPER still forces counts).
 *   With smt_adcensus_timing a chained pair's events are recorded on its chain's stream: kernel_ms of such a pair spans
 *   a launch that shares the device with its neighbour's, and the stand-alone table kernel of a chain's first pair is
 *   not inside its table interval.
 * Test hook, host only (no GPU), exported, defined in csrc/adcensus_selftest.hip:
 *   int smt_adcensus_selftest_chains(int pairs, int chains, long c0, long c1, long c2, int order, unsigned flags);
 * writes the plan of such a call down (the function the call itself runs) for chains whose pair counters stand at c0,
 * c1, c2 (earlier calls leave any parity), order 0 (default) / 1 pairs / 2 ab / 3 ba, flags 1 shared form | 2 the last
 * pair writes volumes | 4 fork at the start | 8 SMT_SHARED_FINISH=apart, and computes happens-before over its launches
 * from stream order and the event edges.  SMT_OK iff every event is recorded before it is waited on, every table set a
 * launch reads was built for its pair by a launch before it and is built by no other unless before that builder or
 * behind the reader, every key map is merged, converted exactly once into the merging pair's map and only then merged
 * again, by launches in a total order, every pair is launched once and its right map is complete before the call's end
 * on the caller's stream, and every operation lies between the call's start and its end there.  SMT_ERR_STATE
 * otherwise; SMT_ERR_ARG unless 1 <= pairs <= 512, 1 <= chains <= 3, counters >= 0, order 0..3, flags < 16. */
int smt_adcensus_compute_batch(smt_adcensus *h, const float *L, const float *R, int pairs,
                               int views, float *dispL, float *dispR);

/* ---- host-fed batches: uint8 images in host memory in, both views' maps in host memory out ----------------------
 * What main.cpp does around the hot path (imread + cvtColor BGR2GRAY, :16-20; the uchar -> float staging, :46-55; the
 * maps back to the host for imwrite, :115-117) for a whole batch.  The handle owns a smt_adcensus (created with
 * SMT_ADCENSUS_NO_PLACEMENT_SEARCH | SMT_ADCENSUS_NO_STORE_CALIBRATION; it exposes no volumes), three streams (copies
 * in, compute, copies out) and two slots of every device buffer for `chunk` pairs: the copies of chunk k+1 in and of
 * chunk k-1 out run beside the compute of chunk k, and with D <= 256 the tables of a chunk's first pair are built
 * inside the previous chunk's last launch, as smt_adcensus_compute_batch does between pairs.  The maps equal
 * smt_adcensus_compute_batch's (both views) bit for bit. */
typedef struct smt_adcensus_host smt_adcensus_host;
#define SMT_MAP_F32 0 /* float32 maps, as smt_adcensus_compute_batch writes them (any D <= 512) */
#define SMT_MAP_U8 1  /* uint8 maps, exact for the WTA indices; D <= 256 only, else SMT_ERR_ARG */
/* device < 0: the current one.  channels 1 (gray) or 3 (B, G, R as imread gives them; converted with smt_bgr2gray's
 * rule).  chunk >= 1 pairs per step. */
int smt_adcensus_host_create(int device, int H, int W, int D, float sigmaC, float sigmaS, int channels, int map_format,
                             int chunk, smt_adcensus_host **out);
/* HOST pointers: L, R uint8 [pairs][H][W][channels]; dispL, dispR [pairs][H][W] of map_format.  Synchronising:
 * returns once both maps of every pair are in host memory.  pairs == 0 is a no-op.  Pinned memory (smt_host_malloc,
 * hipHostRegister, torch pin_memory) is what makes the copies overlap; pageable pointers give the same results,
 * slower. */
int smt_adcensus_host_run(smt_adcensus_host *h, const uint8_t *L, const uint8_t *R, int pairs, void *dispL,
                          void *dispR);
typedef struct smt_host_stats {
    double wall_ms;                    /* first H2D start -> last D2H end (device events) */
    double h2d_ms, compute_ms, d2h_ms; /* summed per-chunk event durations on each stream */
    uint64_t h2d_bytes, d2h_bytes;
    int chunks, pinned_in, pinned_out; /* pinned_*: both buffers reported as pinned host memory by HIP */
} smt_host_stats;
int smt_adcensus_host_stats(smt_adcensus_host *h, smt_host_stats *s); /* of the last run */
int smt_adcensus_host_destroy(smt_adcensus_host *h);
int smt_host_malloc(void **p, size_t bytes); /* pinned host memory (hipHostMalloc); plumbing for C / C++ callers */
int smt_host_free(void *p);
/* Test hook, host only (no GPU): builds the enqueue schedule of a run of `pairs` pairs in chunks of `chunk` (with and
 * without the fused table builds, with and without the uint8 pack) and simulates it.  SMT_ERR_STATE if a wait is
 * enqueued before its record, a slot is overwritten before its last reader is ordered before the write, a pair is
 * copied in or out other than once, or a pair's tables are not built exactly once before its cost launch; SMT_ERR_ARG
 * for chunk <= 0 or pairs < 0; else SMT_OK. */
int smt_adcensus_host_selftest_schedule(int pairs, int chunk);

/* GetPtrLeft / GetPtrRight (AD-Census.h:50-72): borrowed device pointer, valid until
 * destroy, to the view's float32 [H][W][D] volume. view = SMT_VIEW_LEFT or SMT_VIEW_RIGHT.  The first call on a handle ends the deferral of
 * smt_adcensus_compute_batch's last pair for good; if that pair's volumes are pending it writes both with one
 * launch of the both-views cost kernel on the handle's stream and waits for it (with smt_adcensus_timing on,
 * that launch is one more entry of smt_adcensus_kernel_times, with ~0 for the tables).  Every later call only
 * returns the pointer. */
int smt_adcensus_volume(smt_adcensus *h, int view, float **vol);

/* Test hook: on != 0 routes the pair through the first-version table-lookup kernel (a second,
 * independent formulation kept for cross-checking) instead of the register-window kernel. */
int smt_adcensus_force_generic(smt_adcensus *h, int on);

/* Test hook, host only (no GPU): checks the workgroup arithmetic of the fused batch launch -- with `ncost` cost
 * workgroups (a multiple of 8) and `nprep` table workgroups every cost group and every table group is reached exactly
 * once.  SMT_OK, or SMT_ERR_STATE if the mapping is not a bijection. */
int smt_adcensus_selftest_fused_grid(int ncost, int nprep);
/* Test hook, host only (no GPU): checks the workgroup arithmetic of the maps-only batch launch -- with K chunks per
 * cost workgroup every 64-pixel chunk of an H x (nbx*64) both-views launch is reached exactly once and on its XCD, and
 * with `nprep` > 0 table workgroups fused in, every cost and table workgroup too.  SMT_OK or SMT_ERR_STATE. */
int smt_adcensus_selftest_maps_grid(int nbx, int H, int K, int nprep);
/* Test hook, host only (no GPU): checks the rank table of the maps-only kernel for these sigmas against the float sums
 * lut[ad] + lut[256+hd] it stands for (order preserved, equal ranks exactly when the bits are equal).  SMT_OK or
 * SMT_ERR_STATE; SMT_ERR_ARG unless both sigmas are > 0. */
int smt_adcensus_selftest_cost_rank(float sigmaC, float sigmaS);
/* Shared maps-only form of smt_adcensus_compute_batch (adcensus_kernels.h, k_cost_maps_shared).  For 3 <= j' and j' + d <= W-4
 * the right view's cost(i, j', d) is bit for bit the left view's cost(i, j' + d, d), so for the pairs of a batch that
 * write maps only (both maps requested, D <= 256, W >= D + 6) the right map of the columns 3 <= j' <= W-3-D is taken
 * from keys (cost bits << 32 | d) that the left pass publishes.  The columns j' > W-3-D get the keys of their
 * hypotheses with j' + d <= W-4 the same way; what is left to them are the edge hypotheses W-3 <= j' + d <= W+3 (the
 * cost is constant in d past W+3-j', so later ones cannot be a first minimum), which the launch's edge items evaluate
 * with the right view's arithmetic and merge into the key, as they evaluate every hypothesis of the columns 0..2.
 * Maps are those of the two-view kernel, bit for bit.  The host takes this form for D <= 192 and keeps the two-view
 * kernel for 192 < D <= 256, where it measured slower.
 *   SMT_MAPS_SHARED=0 in the environment (read at every call, like SMT_MAPS_CHUNKS / SMT_MAPS_KERNEL / SMT_OVERLAP)
 *   keeps the two-view kernel everywhere, SMT_MAPS_SHARED=force takes the shared form for every D <= 256 with
 *   W >= D + 6: same-process A/Bs and tests.  SMT_MAPS_KERNEL=rank selects the rank kernel as before.
 * In the left pass a workgroup stages a run of up to 4 consecutive 64-pixel chunks of one row once, every wave walks a
 * contiguous quarter of it in one pass and the run's columns are flushed once.
 * Test hook, host only (no GPU), exported by the library, defined in csrc/adcensus_selftest.hip:
 *   int smt_adcensus_selftest_shared_keys(int H, int W, int D, int K, unsigned seed);
 * walks the runs of K chunks per workgroup, the key ring, its flushes and the key-map merges of that form through the
 * kernel's own index functions over pseudo-random costs with many exact ties (seed % 3: 0 a palette with ties, 1 every
 * cost equal, 2 mostly distinct; the right view's edge hypotheses have pseudo-costs of their own).  SMT_OK iff every
 * right pixel is written exactly once, with the first minimum over its shared and its edge hypotheses, every ring ends
 * empty and the key map is reset; and that the split finish below (edge merges in front of or behind the publishes'
 * merges, by seed & 4, then the conversion) gives the single pass's result;
 * SMT_ERR_STATE otherwise; SMT_ERR_ARG unless H, W >= 1, 1 <= D <= 256, 1 <= K <= 64.
 * Finishing a pair.  The launch of a shared pair carries three kinds of auxiliary workgroups beside its cost
 * workgroups: the table tiles of the NEXT pair, the edge items of ITS OWN pair (the edge hypotheses above, merged into
 * the key map with atomic minima for the columns <= W-4 and written to the map for the columns W-3 .. W-1 and 0..2) and
 * the conversion items of the PREVIOUS shared pair (key -> map entry, key reset; they need no tables).  A handle has
 * two key maps, pair n merges into map n & 1.  The last shared pair of a call, and a shared pair followed by anything
 * but another shared pair, is converted by a small launch of its own on the handle's stream before anything else is
 * issued there: no conversion is pending when an entry point returns.
 *   SMT_SHARED_FINISH=apart in the environment (read at every call) converts every pair with that launch of its own
 *   right behind the pair's launch (two launches per pair): same-process A/Bs and tests.  Maps are the same.
 * Test hooks, host only (no GPU), exported, defined in csrc/adcensus_selftest.hip:
 *   int smt_adcensus_selftest_shared_aux_grid(int ncost, int nprep, int nedge, int nconv);
 * every cost workgroup (ncost > 0, a multiple of 8) and every table, edge and conversion item of such a launch is
 * decoded exactly once;
 *   int smt_adcensus_selftest_shared_aux(int H, int W, int D, int K, int first, int last);
 * the same for the counts of an H x W x D pair (first: nothing to convert, last: no tables to build), and the items'
 * pixel arithmetic covers each key, each pixel of the columns W-2-D .. W-1 and each of the columns 0..2 exactly once,
 * and no column W-3-D < j' <= W-4 has an empty edge range.  SMT_OK, SMT_ERR_STATE, or SMT_ERR_ARG (also for W < D + 6).
 * Tapered tail.  The chunks of a maps-only launch (shared or two-view) are cut into workgroups per XCD slice by one span
 * rule (adcensus_rules.h, maps_span): the slice's last n1 workgroups take 1 chunk, the n2 before them max(1, K/2), all
 * before those K (SMT_MAPS_CHUNKS), and the launch's auxiliary workgroups are placed in front of the first tapered one.
 * Maps do not depend on it.  The counts come from the device (workgroups resident per slice, queried at create) and
 * are 0 for a launch of at most one round of workgroups (DESIGN.md section 4 "Tapered tail").
 *   SMT_MAPS_TAPER in the environment (read at every call): 0 is off, the plain rule and placement exactly; n2,n1 are
 *   these counts per slice whatever the launch size (tests, sweeps).  The host-only selftests above walk what the
 *   variable selects.
 * Test hook, host only (no GPU), exported, defined in csrc/adcensus_selftest.hip:
 *   int smt_adcensus_selftest_spans(long nb, int K, int n2, int n1);
 * over the 8 slices of a launch of nb chunks: every chunk belongs to exactly one workgroup, none crosses its slice or
 * has more than K chunks, the workgroup count is the rule's, tails that fit have the sizes above, and n2 = n1 = 0 is
 * the plain rule [g K, g K + K).  SMT_OK, SMT_ERR_STATE, or SMT_ERR_ARG unless 1 <= nb <= 2^28, 1 <= K <= 64,
 * n2, n1 >= 0. */

/* Synchronises the stream and returns SMT_ERR_DOMAIN if any pixel seen since the previous
 * smt_adcensus_status call (or since create) was not an integer in 0..255 (then those pairs' volumes
 * are unspecified), else SMT_OK.  Read-and-clear: a bad pair does not poison later checks.  Bad input is
 * therefore reported late, at the first status call after the compute; call it before consuming results
 * (the host mirrors do so in WTA() / GetPtr*()). */
int smt_adcensus_status(smt_adcensus *h);

/* First-strict-minimum argmin over d of one volume.  Replaces
 * CrossArmAggregation::WTA (CrossArm.cpp:33-57), ScanlineOptimizer::WTA
 * (ScanlineOptimizer.h:40-64), ComputeDispOringin (CBLSM/CBLSM.h:383-407) and, applied
 * twice, AD_Census::WTA. */
int smt_wta(const float *vol, int H, int W, int D, float *disp, void *stream);

/* Sub-pixel disparities: the parabola through the winner and its two neighbours that SAD/Sad.h:76-81 and
 * CBLSM/CBLSM.h:285-290 compute and then drop (they return best_disp).  One rule everywhere
 * (csrc/subpixel_rule.h), for a cost row c[0..D) in float32, one rounding per operation:
 *   w = the winner by smt_wta's rule;  if w == 0 or w == D - 1 the result is (float)w;  otherwise
 *   s = (c[w-1] + c[w+1]) - 2 c[w];  den = min_den < s ? s : min_den  (std::max(min_den, s): a NaN s gives min_den);
 *   off = (c[w-1] - c[w+1]) / (2 den);  result = isfinite(off) ? (float)w + off : (float)w.
 * min_den is the reference's literal 1 (Sad.h:80); it must be finite and > 0, else SMT_ERR_ARG.  Volumes of
 * AD-Census magnitude (costs in [0, 2]) almost always sit under that clamp: pass a small value for the true parabola. */
typedef struct smt_subpixel_params { float min_den; } smt_subpixel_params;   /* 1: Sad.h:80 */
void smt_subpixel_default_params(smt_subpixel_params *p);
/* smt_wta with the rule above: vol float32 [H][W][D] (4-byte aligned, D <= SMT_MAX_DISPARITY), disp float32 [H][W].
 * p == NULL means the defaults.  Argument checks as smt_wta, plus min_den.  Asynchronous on `stream`. */
int smt_wta_subpixel(const float *vol, int H, int W, int D, const smt_subpixel_params *p, float *disp, void *stream);
/* The same on host buffers with the same rule header, no GPU. */
int smt_wta_subpixel_host(const float *vol, int H, int W, int D, const smt_subpixel_params *p, float *disp);

/* =====================================================================================
 * Cross-arm rectangle aggregation     replaces class CrossArmAggregation
 *                                     (AD-CensusV1/CrossArm.{h,cpp}) and the active
 *                                     CBLSM.h functions ArmLength{L,R,Up,Down},
 *                                     costAggregationV5
 * ===================================================================================== */
typedef struct smt_crossarm smt_crossarm;

typedef struct smt_crossarm_params {
    int tau;          /* initial threshold: 30 (main.cpp:27) / 25 (CBLSM.cpp:30) */
    int tau_low;      /* 6  (CrossArm.cpp:225, CBLSM.h:719) */
    int sec_length;   /* 17 (CrossArm.cpp:223) / secLength (CBLSM.cpp:32) */
    int max_length;   /* 34 (CrossArm.cpp:226) / maxLength (CBLSM.cpp:31) */
    int chain_tau;    /* 1: `_tao` is a member, sticky across the four direction calls
                            (CrossArm.h:34); 0: by-value per call (CBLSM.h:643) */
    unsigned quirks;  /* SMT_QUIRK_*; 0 = faithful.  CBLSM-style arms have no stride bug:
                            pass SMT_QUIRK_FIX_RIGHT_ARM_STRIDE for them.  With SMT_QUIRK_FIX_STICKY_TAU
                            chain_tau has no effect and smt_crossarm_tau reports tau. */
} smt_crossarm_params;

void smt_crossarm_default_params(smt_crossarm_params *p); /* AD-CensusV1 main.cpp values */
void smt_crossarm_cblsm_params(smt_crossarm_params *p);   /* CBLSM.cpp values */

/* CrossArmAggregation::Initialize (CrossArm.cpp:6-18): allocates the four arm maps and
 * resets the sticky threshold. */
int smt_crossarm_create(int H, int W, int D, const smt_crossarm_params *p, smt_crossarm **out);
int smt_crossarm_create_on(int device, int H, int W, int D, const smt_crossarm_params *p, smt_crossarm **out);
int smt_crossarm_destroy(smt_crossarm *h);
int smt_crossarm_set_stream(smt_crossarm *h, void *stream);

/* ComputeLeftArmLength, ComputeRightArmLength, ComputeTopArmLength,
 * ComputeButtonArmLength (CrossArm.cpp:147-598) in that order with the threshold state
 * chained as the reference's member does.  Resets the threshold first, i.e. it is
 * Initialize + the four calls of main.cpp:68-72.
 *   img        uint8 [H][W][channels], channels 1 (gray branch) or 3 (Vec3b branch). */
int smt_crossarm_arms(smt_crossarm *h, const uint8_t *img, int channels);

/* One-to-one forms of the reference's four calls (CrossArm.h:15-18), for callers that run a subset or
 * another order -- which changes the sticky-threshold chain (`_tao` is lowered at CrossArm.cpp:223-225 by
 * whichever call first walks past sec_length and stays lowered for every later pixel and call):
 *   smt_crossarm_reset    = the state part of Initialize (CrossArm.cpp:13-17): threshold back to tau, the
 *                           four maps zeroed;
 *   smt_crossarm_arm_dir  = ComputeLeftArmLength (dir 0, :147-260), ComputeRightArmLength (1, :262-373),
 *                           ComputeTopArmLength (2, :375-486), ComputeButtonArmLength (3, :488-598) with
 *                           the threshold as the previous call left it;
 *   smt_crossarm_tau      = the current `_tao` (synchronising; for tests).
 * smt_crossarm_arms(h, img, ch) == reset + arm_dir 0, 1, 2, 3, in two launches.  With chain_tau = 0
 * (CBLSM.h:643, by-value threshold) every call starts from tau. */
int smt_crossarm_reset(smt_crossarm *h);
int smt_crossarm_arm_dir(smt_crossarm *h, const uint8_t *img, int channels, int dir);
int smt_crossarm_tau(smt_crossarm *h, int *tau);

/* Test hook: on != 0 computes arms with the first-version kernels (neighbour-by-neighbour walk, an
 * independent formulation) instead of the bit-mask kernels; they are also what runs when sec_length or
 * max_length exceeds 63. */
int smt_crossarm_set_arm_walk(smt_crossarm *h, int on);

/* Borrowed pointers to the int32 [H][W] arm maps (leftLength, rightLength, topLength,
 * buttonLenght; CrossArm.h:30-33). */
int smt_crossarm_arm_maps(smt_crossarm *h, int **left, int **right, int **top, int **bottom);
/* The other direction: arm maps the caller already has (DEVICE int32 [H][W] each) become the handle's maps, so that
 * the aggregation entry below serves callers whose reference signature takes the four arrays --
 * costAggregationV5(dispvolume, CostVolume, ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown, ...) (CBLSM.h:1179);
 * CBLSM.cpp:150 aggregates the RIGHT view's volume with the LEFT image's arms this way.  Lengths outside 0..8191
 * are clamped and make smt_crossarm_status return SMT_ERR_REF_UB. */
int smt_crossarm_load_arm_maps(smt_crossarm *h, const int *left, const int *right, const int *top, const int *bottom);

/* order 0: AggregationVertical (CrossArm.cpp:60-102), columns outer / rows inner;
 * order 1: costAggregationV5 (CBLSM.h:1179-1224), rows outer / columns inner;
 * order 2: Aggregation (CrossArm.cpp:104-145; public in CrossArm.h:19, no call site): rows outer with
 *          EXCLUSIVE upper bounds [-up, down) x [-L, R); a pixel whose rectangle is empty divides 0 by 0
 *          (:138) -- the result is NaN there and smt_crossarm_status returns SMT_ERR_REF_UB.
 * Sequential float adds in exactly that order, divided by the tap count.
 * vol_in, vol_out float32 [H][W][D] of the handle, distinct; disp float32 [H][W].
 * If disp != NULL the WTA of the aggregated volume is fused (CrossArm.cpp:33-57).
 * Returns SMT_ERR_REF_UB from smt_crossarm_status when a rectangle leaves the plane
 * (possible with the right-arm stride bug on small / non-landscape images). */
int smt_crossarm_aggregate(smt_crossarm *h, const float *vol_in, float *vol_out, int order,
                           float *disp);
int smt_crossarm_status(smt_crossarm *h); /* synchronising; read-and-clear: reports rectangles that left the
                                             plane (or, order 2, were empty) since the previous status call */
/* Test / tuning hook: which aggregation kernel runs.  13 (default) = 12 with the scalar side of a tap (byte offsets of
 * its two flag rows, one "group has a member" bit per tile row) packed into one word by the vector classification of
 * the batch; 12 = 4x4 pixels per wave, every tap of the union of
 * their rectangles loaded once and added under membership flags (v_pk_fma_f32, flag pairs in SGPRs), tile rows
 * without a member skipped, flag rows fetched one tap ahead, per-axis membership tables, and the four waves of a
 * workgroup (8 x 8 pixels) walking their common bounding box in lock-step, one s_barrier per 64 positions;
 * 7 = the same with 2x8 tiles; 6 = 7 free-running (strip width 16); 4 = 6 with the flags fetched per live group and
 * pixel-by-pixel classification; 5 = 4 without the skip; 3 = 1x8 pixels without the skip; 8, 9, 11 = the flagged
 * accumulate on the matrix pipe (v_mfma_f32_4x4x1_16b_f32 with A = membership flags: every group / live groups only /
 * live groups with 4x4 tiles); 10 = four taps per v_mfma_f32_16x16x4_f32 (4x4 tiles, free-running, D a multiple of
 * 64, else 12 runs); 0 = four adjacent pixels per wave, 16-way switch on the mask; 1 = plain one-pixel-per-wave walk
 * (the only form for volumes >= 4 GiB, D > 256 and order 2); 2 = pipelined walk.  Every variant produces the same bits;
 * the matrix-pipe forms are measured equal to or slower than the default. */
int smt_crossarm_set_variant(smt_crossarm *h, int variant);
/* Tuning hook: width (multiple of 4, 4 .. 4096; anything else is SMT_ERR_ARG -- beyond 4096 the 32-bit grid size of a
 * small image overflows) of the column strips each XCD sweeps (all variants but 1; variant 0 rounds it up to a multiple
 * of 16, variants 3 .. 13 to 8, 16 or a multiple of 32). */
int smt_crossarm_set_strip_width(smt_crossarm *h, int width);
/* Tuning hook: aggregation waves per SIMD (3, 4 or 5, enforced through an LDS claim per workgroup; 0 = whatever the
 * register count allows, i.e. 6: the default).  Limiting it leaves VGPRs for kernels of other streams, which on this
 * path buys nothing (the scanline passes then run beside the aggregation and both slow down).
 * SMT_AGG_WAVES in the environment overrides the default for every handle. */
int smt_crossarm_set_occupancy(smt_crossarm *h, int waves_per_simd);
/* Tuning hook (variants 3 .. 13, the default included; 0 .. 2 ignore it): 0 = column strips interleaved over the 8 XCDs,
 * 1 = every XCD owns one contiguous band of rows and sweeps it strip by strip.  Placement only; results are identical. */
int smt_crossarm_set_sweep(smt_crossarm *h, int sweep);
/* Sub-pixel switch: with p != NULL, smt_crossarm_aggregate writes to `disp` the winner refined by the rule of
 * smt_wta_subpixel with p->min_den; NULL = off, the integer map (the default).  From the next call on the handle,
 * between runs.  Fused into the default variant (13) and the plain walk (1, also D > 256, volumes >= 4 GiB and order 2);
 * every other variant aggregates into vol_out and smt_wta_subpixel reads it back.  vol_out is the same either way. */
int smt_crossarm_set_subpixel(smt_crossarm *h, const smt_subpixel_params *p);
/* Test hook, host only (no GPU, no handle): the workgroup-to-pixel map of aggregation variant `variant` on an H x W image
 * with smt_crossarm_set_strip_width(strip_width) (0 = the width smt_crossarm_set_variant selects) and
 * smt_crossarm_set_sweep(sweep), through the functions the kernels and the launchers run.  Every workgroup and wave of
 * the grid the launcher would ask for is enumerated; SMT_ERR_STATE when a pixel is owned twice or by no wave, when a
 * wave that owns pixels has rows or columns past the image, when a sweep-0 strip (and every strip of variants 0 and 2)
 * is not on XCD strip % 8, or when a sweep-1 band of rows is not on its own XCD.  Variant 1 checks the plain
 * (H * W + 3) / 4 grid.  SMT_ERR_ARG: variant outside 0 .. 13, H or W < 1, H * W > INT_MAX, sweep outside 0 .. 1, a width
 * smt_crossarm_set_strip_width would refuse, or a grid beyond INT_MAX workgroups. */
int smt_crossarm_selftest_grid(int variant, int H, int W, int strip_width, int sweep);

/* CBLSM.h:327-381 ComputeAD / ComputeADRight on uchar images -> float volume. */
int smt_cblsm_ad(const uint8_t *L, const uint8_t *R, int H, int W, int D, int view, float *vol,
                 void *stream);

/* CBLSM.h:65-236 chooseArmLengthLeft / Right / Up / Down (dir 0 / 1 / 2 / 3): per-hypothesis arm
 * lengths, int32 [H][W][D], from the two views' arm maps (int32 [H][W], e.g. smt_crossarm_arm_maps
 * of a left-image and a right-image handle).  own_arm = ArmLL / ArmLR / ArmLUp / ArmLDown;
 * other_vertical_arm = ArmRUp / ArmRDown for dir 2 / 3 (ignored for 0 / 1, may be NULL).  The
 * reference's call sites are commented out (CBLSM.cpp:108-111); the up / down forms read the right
 * view's arms at row i -/+ k for k <= own_arm, so own_arm must stay inside the image, as the arm
 * kernels guarantee. */
int smt_cblsm_choose_arm_length(int dir, const int *own_arm, const int *other_vertical_arm,
                                const int *armRL, const int *armRR, int H, int W, int D,
                                int *arm_volume, void *stream);

/* CBLSM.h:1087-1126 costAggregationNew with :969-1045 ComputeLocalValue (dead experiment, call site commented
 * out at CBLSM.cpp:113-116): cost[p][d] = | value(left image, arms at slot 0) - value(right image shifted by
 * d, arms at slot d) |, value = sum over rows [-Up, Down] of the row's pixels in [j-L-d, j+R-d) divided by
 * the sum of (L+R+1) -- the reference counts one pixel more per row than it adds (:1021, :1034), R+1 for
 * a left-clipped row (:1011) and 1 for a row clipped to column 0 (:996); all reproduced.
 *   Lp, Rp      uint8 [H+2w][W+2w], replicate-padded by w = winSize+1
 *   armvol*     int32 [H][W][D] from smt_cblsm_choose_arm_length (dir 0, 1, 2, 3); Up / Down must keep
 *               rows inside the image (rows outside are skipped)
 *   cost        float32 [H][W][D] out. */
int smt_cblsm_cost_aggregation_new(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winSize,
                                   const int *armvolL, const int *armvolR, const int *armvolUp,
                                   const int *armvolDown, float *cost, void *stream);

/* CBLSM.h:1128-1176 costAggregationV4, the consumer of the four smt_cblsm_choose_arm_length volumes (the reference
 * wrote it and left it uncalled): vol_out[p][d] = mean of vol_in[.][d] over rows [i - Up, i + Down) and columns
 * [j - L, j + R) with L, R, Up, Down the arm volumes' entries at (p, d) -- half-open on the far side, unlike V5 --
 * added row by row in float, in the reference's order, and divided by the int tap count.  An empty rectangle gives
 * 0.0f / 0 = NaN, as the reference does (sign and payload of the NaN are not part of the contract).
 *   vol_in, vol_out  float32 [H][W][D], distinct
 *   armvol*          int32 [H][W][D], any values
 *   disp             NULL, or float32 [H][W]: ComputeDispOringin (:383-407) of vol_out by smt_wta's rule -- the first
 *                    strict minimum wins, a NaN at d > 0 never wins, a NaN at d = 0 gives 0; needs D <= SMT_MAX_DISPARITY
 *   ub_flag          NULL, or a device int that is ORed with 1 when a tap lies outside the plane (the reference then
 *                    reads out of bounds or from a neighbouring row); such rectangles are clipped to the plane and
 *                    their hypotheses are unspecified
 * No cap on D without disp (one thread per pixel and hypothesis).  SMT_ERR_ARG for NULL or aliased volumes,
 * non-positive sizes, H * W >= 2^31 and more than 2^39 hypotheses.  Asynchronous on `stream`. */
int smt_cblsm_cost_aggregation_v4(const float *vol_in, const int *armvolL, const int *armvolR, const int *armvolUp,
                                  const int *armvolDown, int H, int W, int D, float *vol_out, float *disp, int *ub_flag,
                                  void *stream);

/* =====================================================================================
 * Scanline optimiser                  replaces class ScanlineOptimizer
 *                                     (AD-CensusV1/ScanlineOptimizer.h)
 * ===================================================================================== */
typedef struct smt_scanline smt_scanline;

/* ScanlineOptimizer::Initialize (:66-79).  The reference allocates five volumes; this
 * engine keeps one scratch volume. */
int smt_scanline_create(int H, int W, int D, int p1, int p2, smt_scanline **out);
int smt_scanline_create_on(int device, int H, int W, int D, int p1, int p2, smt_scanline **out);
int smt_scanline_destroy(smt_scanline *h);
int smt_scanline_set_stream(smt_scanline *h, void *stream);
/* SMT_QUIRK_FIX_SCAN_VERTICAL for the passes 2 and 3 of smt_scanline_pass / smt_scanline_run (0 = faithful, the default) */
int smt_scanline_set_quirks(smt_scanline *h, unsigned quirks);
/* Sub-pixel switch: with p != NULL, the fused WTA of smt_scanline_run writes the winner refined by the rule of
 * smt_wta_subpixel with p->min_den, inside the last pass; NULL = off, the integer map (the default).  From the next
 * call on the handle, between runs. */
int smt_scanline_set_subpixel(smt_scanline *h, const smt_subpixel_params *p);

/* ScanlineOptimizer::ScanLine (:104-128): the four passes and ((left+right)+up)+down,
 * written to vol_out (`_ProcessedVolume`).  gray: float32 [H][W] guidance image
 * (`leftptr`, main.cpp:88).  vol_in, vol_out float32 [H][W][D]; disp float32 [H][W].
 * If disp != NULL, ScanlineOptimizer::WTA (:40-64) is fused.
 * vol_out must not alias vol_in. */
int smt_scanline_run(smt_scanline *h, const float *vol_in, const float *gray, float *vol_out,
                     float *disp);

/* One path volume only (leftVolume/rightVolume/upVolume/downVolume), for tests.
 * pass: 0 left->right (isLeft=true), 1 right->left, 2 top->bottom (isUp=true), 3 bottom->top. */
int smt_scanline_pass(smt_scanline *h, const float *vol_in, const float *gray, int pass,
                      float *vol_out);

/* =====================================================================================
 * The whole AD-CensusV1/main.cpp pipeline, batched      (SURVEY 8b "batch variants"; BASELINE configs[2])
 * ===================================================================================== */
typedef struct smt_pipeline smt_pipeline;
typedef struct smt_pipeline_params {
    float sigmaC, sigmaS;   /* 10, 30   main.cpp:25-26 */
    int tao, p1, p2, gate;  /* 30, 10, 150, 2   main.cpp:27-30 */
} smt_pipeline_params;
void smt_pipeline_default_params(smt_pipeline_params *p);
/* Owns one AD_Census, one CrossArmAggregation, one ScanlineOptimizer and the three volumes between them. */
int smt_pipeline_create(int H, int W, int D, const smt_pipeline_params *p, smt_pipeline **out);
int smt_pipeline_create_on(int device, int H, int W, int D, const smt_pipeline_params *p, smt_pipeline **out);
int smt_pipeline_destroy(smt_pipeline *h);
int smt_pipeline_set_stream(smt_pipeline *h, void *stream);
/* SMT_QUIRK_* for every stage the handle owns (AD-Census, both views' arms, scanline), between runs; 0 = faithful, the
 * default.  With SMT_QUIRK_FIX_RIGHT_ARM_STRIDE square and portrait pairs (H >= W) run too: arms then never leave
 * their row; without it H > W gives SMT_ERR_REF_UB as before. */
int smt_pipeline_set_quirks(smt_pipeline *h, unsigned quirks);
/* Sub-pixel switch of the scanline handle and of both views' aggregation handles, under every SMT_PIPE_SCHEDULE, between
 * runs; NULL = off, the integer maps (the default).  With it smt_pipeline_run_batch and _post give dispL refined from
 * the scanline sum and dispR refined from the aggregated right volume; the LR check (which rounds j - disp + 0.5),
 * RemoveSpeckles and MedianFilter then run on those maps, unchanged. */
int smt_pipeline_set_subpixel(smt_pipeline *h, const smt_subpixel_params *p);
/* main.cpp:46-92 for `pairs` pairs of uint8 gray images [pairs][H][W] (the images after cvtColor, :19-20), in
 * main.cpp's order with lines 86-89 and 92 enabled: float copies, ComputeADcensus(+Right), CrossArm
 * Initialize + four arm passes + AggregationVertical + WTA on the left and on the right image,
 * ScanlineOptimizer on the LEFT aggregated volume + WTA, LeftRightConsistency(gate).
 *   dispL   float32 [pairs][H][W]: the scanline WTA map after the LR check (+inf = rejected)
 *   dispR   float32 [pairs][H][W]: WTA of the aggregated right volume (main.cpp:84)
 *   cls     uint8   [pairs][H][W] as smt_lrcheck;  counts int32 [pairs][2] (may be NULL)
 * dispL, dispR and cls are all required, and pairs >= 1: SMT_ERR_ARG for a NULL handle, image or map and for
 * pairs <= 0 (an empty batch is not a no-op here, unlike the flows below).
 * Asynchronous: the call enqueues and returns; part of the work runs on streams the handle owns (the right
 * view's aggregation beside the left view's scanline passes, see csrc/pipeline.hip), but everything a call
 * enqueued is ordered before whatever the caller enqueues next on the handle's stream, and after whatever the
 * caller enqueued there before the call (the inputs).  One caller thread per handle.  The volumes are reused
 * per pair (smt_pipeline_volumes: the last pair's, borrowed).  This is the sharding unit for the pair axis of
 * config 3.  SMT_PIPE_SCHEDULE=0|1|2 (environment, read at create) selects the stream schedule; results
 * are identical. */
int smt_pipeline_run_batch(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                           float *dispL, float *dispR, uint8_t *cls, int *counts);
int smt_pipeline_volumes(smt_pipeline *h, float **cost_left, float **cost_right, float **agg_left,
                         float **agg_right, float **scanline_sum);
/* synchronising: SMT_ERR_DOMAIN / SMT_ERR_REF_UB seen since the last call; SMT_ERR_STATE if a speckle kernel of
 * smt_pipeline_run_batch_post hit its loop cap (never expected; that pair's dispL / lastDisp are then unspecified) */
int smt_pipeline_status(smt_pipeline *h);
/* The two post-filters the driver runs after the LR check (main.cpp:93-94, commented out there like :86-89 and :92):
 *   RemoveSpeckles(leftDisp, col, row, speckle_diff, speckle_min_area, speckle_invalid)   1, 30, INT_MIN
 *   MedianFilter(leftDisp, lastDisp, col, row, median_wnd)                                 3
 * speckle_invalid is the x86 value of int(Invalid_Float = +inf). */
typedef struct smt_post_params {
    int speckle_diff;
    unsigned speckle_min_area;
    int speckle_invalid;
    int median_wnd;         /* 1..7 */
} smt_post_params;
void smt_post_default_params(smt_post_params *p);
/* smt_pipeline_run_batch plus main.cpp:93-94 for each pair, right after that pair's LR check: dispL holds the map
 * after the LR check and RemoveSpeckles (in place, as leftDisp in main.cpp), lastDisp float32 [pairs][H][W] (may be
 * NULL) its median -- the map main.cpp writes out (:115).  dispR, cls and counts as smt_pipeline_run_batch.  Same
 * asynchrony and the same results under every SMT_PIPE_SCHEDULE.  The first call allocates the handle's tail scratch
 * (10 bytes per pixel); later calls allocate nothing. */
int smt_pipeline_run_batch_post(smt_pipeline *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                float *dispL, float *dispR, uint8_t *cls, int *counts,
                                const smt_post_params *post, float *lastDisp);

/* =====================================================================================
 * The active CBLSM/CBLSM.cpp flow, batched      (:64-67, 101-104, 133-134, 146-153)
 * ===================================================================================== */
typedef struct smt_cblsm_flow smt_cblsm_flow;
typedef struct smt_cblsm_params {
    int tau, sec_length, max_length;   /* 25, 17, 34   CBLSM.cpp:30-32; tau_low is CBLSM.h:719's fixed 6 */
} smt_cblsm_params;
void smt_cblsm_default_params(smt_cblsm_params *p);
/* Owns two crossarm handles (arms of the left and of the right image: by-value threshold, no stride bug, as
 * smt_crossarm_cblsm_params), the two first-pass volumes and one [H][W][D] scratch: three 4-byte volumes whatever the
 * batch size.  SMT_ERR_ARG unless 1 <= D <= SMT_MAX_DISPARITY, 0 <= tau <= 255 (CBLSM.cpp:30's uchar),
 * sec_length >= 0 and 0 <= max_length <= 4096 (smt_crossarm_create's limit). */
int smt_cblsm_flow_create_on(int device, int H, int W, int D, const smt_cblsm_params *p, smt_cblsm_flow **out);
int smt_cblsm_flow_destroy(smt_cblsm_flow *h);
int smt_cblsm_flow_set_stream(smt_cblsm_flow *h, void *stream);
/* CBLSM.cpp's active lines for `pairs` pairs of uint8 gray images [pairs][H][W] (the images after cvtColor, :21-22),
 * in the file's order per pair: ArmLength{L,R,Up,Down} of the left and of the right image; the first
 * costAggregationV5 pass of the left view (ComputeAD volume, left arms) and of the right view (ComputeADRight volume,
 * right arms); the second pass of the left view on the left arms and of the right view on the LEFT arms (:150); the
 * WTA of each second pass (ComputeDispOringin, :152-153).
 *   dispL, dispR   float32 [pairs][H][W], integer-valued; both required (SMT_ERR_ARG for a NULL map or image, pairs < 0)
 * The first pass never materialises the AD volume while max(sec_length, max_length) <= 127: its sums are then exact in
 * float and come from a summed-area table, bit-identical to the reference's loop (csrc/cblsm.hip); above that bound it
 * is smt_cblsm_ad + smt_crossarm_aggregate(order 1).  pairs == 0 is a no-op.  Asynchronous like
 * smt_pipeline_run_batch, on the handle's stream only; one caller thread per handle. */
int smt_cblsm_flow_run_batch(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                             float *dispL, float *dispR);
/* The per-hypothesis-arm flow the reference's Visual Studio solution is named after, for `pairs` pairs, per pair:
 * ArmLength{L,R,Up,Down} of the left and of the right image (CBLSM.cpp:64-67, 101-104), chooseArmLength{Left,Right,Up,
 * Down} (:108-111), ComputeAD (:133), costAggregationV4 of the AD volume (CBLSM.h:1128-1176), ComputeDispOringin (:152).
 * LEFT VIEW ONLY: the reference has chooseArmLength* anchored on the left image and no right-view counterpart.
 *   dispL   float32 [pairs][H][W], integer-valued; a pixel whose hypothesis 0 has an empty rectangle (NaN) gets 0
 * While max(sec_length, max_length) <= 127 neither the four arm volumes nor the AD volume exist: the arms are derived
 * inside one kernel from the eight arm maps by the reference's rules (csrc/cblsm_v4_rules.h: the right image's arms
 * read at column j, not j - d; Up reset when LUp > RUp; Down keeping its count past RDown; their different
 * comparisons) and the rectangle sums come from the handle's summed-area table, exact because
 * 255 (2 * 127)^2 < 2^24.  Above that bound the handle composes smt_cblsm_ad, four smt_cblsm_choose_arm_length and
 * smt_cblsm_cost_aggregation_v4 and allocates three more [H][W][D] volumes on the first such call; otherwise the
 * handle's buffers suffice.  The parameters alone decide which path runs; both give the same bits.
 * smt_cblsm_flow_volumes then lends the last pair's V4 volume as pass1_left (pass1_right is not meaningful).
 * pairs == 0 is a no-op.  Asynchronous on the handle's stream; errors through smt_cblsm_flow_status. */
int smt_cblsm_flow_run_batch_v4(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL);
/* the last pair's first-pass volumes, float32 [H][W][D], borrowed (valid until the next run or destroy) */
int smt_cblsm_flow_volumes(smt_cblsm_flow *h, float **pass1_left, float **pass1_right);
/* synchronising, read-and-clear: SMT_ERR_REF_UB if a rectangle left the plane since the last call (never expected);
 * SMT_ERR_STATE if a speckle kernel of smt_cblsm_flow_run_batch_post hit its loop cap (never expected either) */
int smt_cblsm_flow_status(smt_cblsm_flow *h);
/* Test hook, host only (no GPU): the first pass's box arithmetic (rectangle corners in a uint32 summed-area table, the
 * clipping of arms that leave the plane) against direct sums on a random H x W x D volume of bytes (fill 0) or of 255s
 * (fill 1), arms up to max_arm; and (float)S / (float)n against costAggregationV5's sequential float sum where S < 2^24.
 * SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for sizes over 2^26 elements. */
int smt_cblsm_selftest_box(int H, int W, int D, int max_arm, int fill, unsigned seed);
/* Test hook, host only (no GPU): the arm rules smt_cblsm_flow_run_batch_v4's kernel runs (csrc/cblsm_v4_rules.h)
 * against the loops of CBLSM.h:65-236 as written, for every pixel and hypothesis of eight random H x W arm maps (zeros,
 * arms at max_arm or the border, W < D allowed); and the half-open box arithmetic (tap count, four-corner sums in a
 * uint32 table, (float)S / (float)n, NaN for an empty rectangle, clipping) against costAggregationV4's walk on random
 * bytes.  SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for non-positive sizes, max_arm outside 0..255 and more than 2^22
 * hypotheses. */
int smt_cblsm_selftest_v4(int H, int W, int D, int max_arm, unsigned seed);

/* =====================================================================================
 * CBLSM's window cost volumes      ComputeDispLeft / ComputeDispRight / ComputeDispV4
 *                                  (CBLSM/CBLSM.h:451-489, :409-447, :494-532; call site CBLSM.cpp:132)
 * =====================================================================================
 * With w = winSize + 1, side = 2 w + 1, n = side^2 and images replicate-padded by w (CBLSM.cpp:124-125), entry
 * vol[y][x][d] over the UNPADDED pixels is the mean absolute difference of two side x side windows of row y:
 *   S(y, xa, xb) = the integer sum of |Lp - Rp| over the windows centred at left column xa and right column xb;
 *   cost         = the float nearest to S / n (sadvalueMean, :17-22: cv::mean narrowed to float).
 *   LEFT   d <= x: cost of S(y, x, x - d); d > x repeats the entry at d = x (the `cost = last` chain, :476-481).
 *   RIGHT  x + d <= W-1-w: cost of S(y, x + d, x).  The guard of :434 stops the view w columns before its data does,
 *          and that is reproduced: for x <= W-1-w < x + d the entry repeats the one at d = W-1-w-x; for x > W-1-w even
 *          d = 0 copies, from the element before the pixel's vector, so all D entries of the last w columns of a row
 *          equal the cost at (y, W-1-w, 0).  W <= w makes the reference read before its buffer: SMT_ERR_REF_UB,
 *          nothing is written.
 *   V4     3-channel padded images [H+2w][W+2w][3]; per tap the smallest of the three channel differences (minValue
 *          ignores its T), added into a uchar, divided by n as an integer:
 *          (float)(((sum of min_c |L_c - R_c|) mod 256) / n); LEFT's edge rule; there is no right counterpart.
 * These functions call cv::mean and absdiff, whose source is in neither tree: they are "parity unpinned", held to a
 * loop-for-loop restatement (tests/cblsm_window_cases.py) and to the exactness of the quotient: for every integer
 * S <= 255 n and every odd side up to 65, 101 and 181, (float)((double)S / n), (float)((double)S * (1.0 / n)) and the
 * IEEE float quotient (float)S / (float)n are the same float (S < 2^24, so (float)S is exact).
 *
 * smt_cblsm_window_cost_batch: `pairs` padded pairs -> `pairs` volumes.  form: SMT_CBLSM_COST_*.  Strides in elements
 * (bytes of an image, floats of a volume) between consecutive pairs, 0 = dense; gaps between pairs are never written.
 * Asynchronous on `stream`, no allocation.  pairs == 0 is a no-op.  SMT_ERR_ARG for NULL pointers, non-positive sizes,
 * pairs < 0 or > 65535, D > SMT_MAX_DISPARITY, winSize < 0 or > 89 (side > 181), an unknown form and strides below a
 * map's size; SMT_ERR_REF_UB as above, before any launch. */
#define SMT_CBLSM_COST_LEFT  1
#define SMT_CBLSM_COST_RIGHT 2
#define SMT_CBLSM_COST_V4    3
int smt_cblsm_window_cost_batch(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D,
                                int winSize, int form, float *vol, size_t vol_stride, void *stream);
/* smt_cblsm_window_cost_batch on host memory, through the same inline rule functions (csrc/cblsm_window_rules.h: the
 * edge rule per form, the quotient, V4's minimum and wrap).  The same arguments without the stream, the same statuses. */
int smt_cblsm_window_cost_host(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D,
                               int winSize, int form, float *vol, size_t vol_stride);
/* Test hooks (process-wide, plain unsynchronised globals).  set_impl: 0 (default) = the dispatch rule in
 * csrc/cblsm_window.hip, 1 = the tap loop (one thread per pixel and hypothesis: the independent formulation), 2 = the box
 * kernel (row sums sliding along a row, a box sum moving down a row, lanes along d); V4 always runs the tap loop.
 * set_band: rows per band of the box kernel's grid, 0 = its own choice.  set_store: 0 = the default, 1 = plain,
 * 2 = non-temporal stores of the box kernel.  SMT_ERR_ARG outside those values.  last_form: 1 or 2, what the last
 * successful call ran (0 before the first). */
int smt_cblsm_window_set_impl(int impl);
int smt_cblsm_window_set_band(int band);
int smt_cblsm_window_set_store(int mode);
int smt_cblsm_window_last_form(void);
/* Test hook: out_dev[k] = the box kernel's own __device__ quotient of S_dev[k] by n (1 <= n <= 181^2, every
 * S_dev[k] < 2^24), so that the instruction sequence the kernel uses can be swept over every sum.  Asynchronous on
 * `stream`.  SMT_ERR_ARG for NULL pointers, n outside that range or count > 2^31. */
int smt_cblsm_window_quotient(const uint32_t *S_dev, size_t count, int n, float *out_dev, void *stream);
/* Test hook, host only (no GPU): on random bytes and on an all-0 against an all-255 pair of the shape, the box
 * arithmetic (row sums sliding along a row, a box sum moving down a row, in uint32) against direct window sums, and the
 * chain rules against a literal per-pixel walk over a flat buffer (a guarded entry copies the element before it).  V4:
 * the walk only.  SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for non-positive sizes, winSize outside 0..89, an unknown form,
 * D > SMT_MAX_DISPARITY or more than 2^22 hypotheses; SMT_ERR_REF_UB for RIGHT with W <= winSize + 1. */
int smt_cblsm_selftest_window(int H, int W, int D, int winSize, int form, unsigned seed);
/* CBLSM.cpp with :132 enabled (and its right-view counterpart) for `pairs` gray pairs [pairs][H][W], per pair: the
 * arms of both images as smt_cblsm_flow_run_batch computes them; the padding of :124-125 into buffers the handle owns;
 * the LEFT window volume into the handle's scratch and its first costAggregationV5 pass on the left arms; the RIGHT
 * window volume and its first pass on the right arms; the two second passes on the LEFT arms (:149-150) with the WTA
 * (:152-153), exactly as smt_cblsm_flow_run_batch.  Window costs are non-integer floats whose sums round, so both
 * passes are the in-order walk (smt_crossarm_aggregate, order 1), never a summed-area table.
 *   dispL, dispR   float32 [pairs][H][W], integer-valued
 * smt_cblsm_flow_volumes lends the last pair's first-pass volumes.  The handle's three volumes suffice and a handle may
 * be called with different winSize in turn, and with the other run_batch entries in between.  pairs == 0 is a no-op.
 * Asynchronous on the handle's stream only; errors through smt_cblsm_flow_status.  SMT_ERR_ARG for NULL arguments,
 * pairs < 0 and winSize outside 0..89; SMT_ERR_REF_UB for W <= winSize + 1, before any device work. */
int smt_cblsm_flow_run_batch_window(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int winSize,
                                    float *dispL, float *dispR);

/* =====================================================================================
 * Left-right consistency              replaces LeftRightConsistency
 *                                     (AD-CensusV1/PostProcessing.h:72-135)
 * ===================================================================================== */
/* In place on dispL (invalid -> +inf).  cls: uint8 [H][W], 0 kept / 1 occlusion /
 * 2 mismatch; the reference's two vectors are these classes in row-major order
 * (smt_lrcheck_lists rebuilds them on the host).  counts: device int32[2] = {occlusions,
 * mismatches}, may be NULL. */
int smt_lrcheck(float *dispL, const float *dispR, int H, int W, int gate, uint8_t *cls,
                int *counts, void *stream);

/* LeftAndRightConsistency (AD-CensusV1/PostProcessing.h:10-70; no call site): the out-of-place sibling.
 * dispL is only read; lastDisp float32 [H][W] receives dispL where the pixel is kept and 0 where it is
 * rejected; the test is abs(d - dR) >= gate with a float gate (:32), no +inf pre-check.  Classes as
 * smt_lrcheck.  A disparity for which `static_cast<int>(j - disp + 0.5)` overflows int (non-finite or
 * huge; undefined in C++) is treated as x86 does: INT_MIN, i.e. out of range -> mismatch. */
int smt_lrcheck_variant(const float *dispL, const float *dispR, float *lastDisp, int H, int W, float gate,
                        uint8_t *cls, int *counts, void *stream);

/* Host helper: expand a HOST copy of cls into the reference's (row, col) pair lists.
 * Each list must have room for H*W pairs (2 ints per pair); returns counts. */
int smt_lrcheck_lists(const uint8_t *cls_host, int H, int W, int *occlusion_pairs, int *n_occ,
                      int *mismatch_pairs, int *n_mis);

/* FillTheHole (AD-CensusV1/PostProcessing.h:156-248; same text in CBLSM/PostProcessing.h).
 * In place on the DEVICE map disp (row*col floats).  The reference swaps the extents
 * (`width = row`, `height = col`, :158-159) and this is reproduced: the buffer is addressed as
 * `col` lines of `row` entries, and a hole is an entry equal to 65535.0f (:182, :212) -- not the
 * +inf that LeftRightConsistency writes.  occ / mis: HOST arrays of (first, second) int pairs in
 * list order, as LeftRightConsistency fills them.  Pass 0 gives each occlusion the second
 * smallest of the first non-hole values met along 8 rays, pass 1 each mismatch their median,
 * pass 2 (only when the mismatch list is not empty, :174) every remaining hole the median.
 * The reference then leaves the third pass's pixel list in the caller's `mismatch` vector
 * (:186): third (HOST, room for row*col pairs, may be NULL) and *n_third (may be NULL; -1 when
 * the list was not replaced) return it.  SMT_ERR_REF_UB where the reference writes out of
 * bounds: a listed pair outside the buffer (nothing is modified), or more third-pass holes than
 * the mismatch list had entries (`fill_disps` is sized before the list is replaced, :177 vs
 * :186; passes 0 and 1 have been applied by then, as in the reference).  A list pointer may be NULL when
 * its count is 0 (the data() of an empty std::vector); n_occ / n_mis < 0 is SMT_ERR_ARG.  Synchronising. */
int smt_fill_the_hole(float *disp, int row, int col, int dispRange, const int *occlusion_pairs,
                      int n_occ, const int *mismatch_pairs, int n_mis, int *third_pairs,
                      int *n_third, void *stream);

/* FillTheHole for `pairs` maps with the lists LeftRightConsistency would have produced, taken from the
 * class maps on the device: exactly smt_fill_the_hole(disp_b, row, col, dispRange, occ, n_occ, mis, n_mis)
 * with (occ, mis) = smt_lrcheck_lists(cls_b).  Asynchronous: one memset and eight kernel launches on `stream`
 * whatever the data and the pair count, no host synchronisation, scratch (4 * pairs * row * col bytes and a few
 * words per pair) from the library's arena.
 *   disp    float32 [pairs][row][col], filled in place;  cls uint8 as smt_lrcheck writes it (values other than 1 and
 *           2 are not targets);  strides in ELEMENTS between consecutive maps, 0 = dense, otherwise >= row*col
 *   status  device int32 [pairs][4], may be NULL: {n_occ, n_mis, n_third, flags}.  n_third is the number of entries
 *           equal to 65535 after pass 1, -1 when pass 2 was not reached (empty mismatch list, :174, or
 *           SMT_FILL_UB_LIST).  flags: SMT_FILL_UB_LIST -- a class pixel (i, j) with i*row + j >= row*col, an
 *           out-of-bounds write in the reference (:244; needs row > col): that pair is not modified;
 *           SMT_FILL_UB_THIRD -- more holes than mismatches (`fill_disps`, :178 against :189): passes 0 and 1 are
 *           applied, pass 2 is not.  The other pairs of the batch are unaffected.
 * The third pass's pixel list is not returned, its count is; a caller who needs the list keeps smt_fill_the_hole,
 * which also takes lists that no class map expresses (duplicates, any order).
 * SMT_ERR_ARG for NULL disp or cls, non-positive sizes, dispRange < 0, pairs < 0, row*col >= 2^31 and strides below
 * row*col; pairs == 0 is a no-op. */
#define SMT_FILL_UB_LIST 1
#define SMT_FILL_UB_THIRD 2
int smt_fill_the_hole_batch(float *disp, const uint8_t *cls, int pairs, size_t disp_stride, size_t cls_stride,
                            int row, int col, int dispRange, int *status, void *stream);
/* Test hook, host only (no GPU): the same rule on HOST memory through the same inline functions (csrc/fill_rules.h:
 * target derivation, set choice, winner gather, pass-2 gating, flags), which is what holds the rule to the oracle
 * where there is no device.  Arguments and return values as smt_fill_the_hole_batch. */
int smt_fill_the_hole_batch_host(float *disp, const uint8_t *cls, int pairs, size_t disp_stride, size_t cls_stride,
                                 int row, int col, int dispRange, int *status);

/* =====================================================================================
 * CrossAggregator (vendored ethan-li AD-Census)   replaces class CrossAggregator
 *                                     (CBLSM/cross_aggregator.{h,cpp})
 * ===================================================================================== */
typedef struct smt_crossagg smt_crossagg;

/* Initialize(width,height,min_disparity,max_disparity) (:19-58). D = max-min, 1 <= D <= SMT_MAX_DISPARITY.
 * Returns SMT_ERR_ARG where the reference returns false (and for D > SMT_MAX_DISPARITY). */
int smt_crossagg_create(int W, int H, int D, smt_crossagg **out);
int smt_crossagg_create_on(int device, int W, int H, int D, smt_crossagg **out);
int smt_crossagg_destroy(smt_crossagg *h);
int smt_crossagg_set_stream(smt_crossagg *h, void *stream);
/* SetParams (:67-74); defaults L1=34 L2=17 t1=20 t2=6 (adcensus_types.h:69-70). */
int smt_crossagg_set_params(smt_crossagg *h, int L1, int L2, int t1, int t2);
/* SetData + Aggregate(num_iters) (:60-65, :89-118).  img_left: uint8 [H][W][3];
 * cost_init: float32 [H][W][D].  The result stays in the handle (get_cost_ptr). */
int smt_crossagg_aggregate(smt_crossagg *h, const uint8_t *img_left, const float *cost_init,
                           int num_iters);
/* Test hook: 2 = shared-tap passes (16 pixels per wave along the pass axis, default), 1 = one pixel per wave
 * (first formulation).  Identical bits. */
int smt_crossagg_set_impl(smt_crossagg *h, int impl);
/* get_cost_ptr (:125-133) / get_arms_ptr (:120-123): borrowed. cost: float32 [H][W][D]; arms: uint8 [H][W][4] =
 * left,right,top,bottom (struct CrossArm, cross_aggregator.h:17-20). */
int smt_crossagg_cost(smt_crossagg *h, float **cost);
int smt_crossagg_arms(smt_crossagg *h, uint8_t **arms);

/* ADCensusOption (CBLSM/adcensus_types.h:45-75), field for field, with its constructor's defaults
 * (smt_adcensus_option_default).  SURVEY 8f n3.  The reference tree holds this struct and the aggregator it
 * feeds but NOT the rest of ethan-li-coding/AD-Census (cost computer, its own scanline optimiser with
 * so_p1 / so_p2 / so_tso, the multi-step refiner with irv_ts / irv_th, filling, discontinuity adjustment,
 * sub-pixel): those fields are carried, nothing consumes them, and no part of that flow is claimed here
 * (it would be "parity unpinned" against a source that is not in /root/reference). */
typedef struct smt_adcensus_option {
    int32_t min_disparity, max_disparity;
    int32_t lambda_ad, lambda_census;
    int32_t cross_L1, cross_L2, cross_t1, cross_t2;
    float so_p1, so_p2;
    int32_t so_tso, irv_ts;
    float irv_th, lrcheck_thres;
    int32_t do_lr_check, do_filling, do_discontinuity_adjustment;      /* bool in the reference */
} smt_adcensus_option;
void smt_adcensus_option_default(smt_adcensus_option *o);
/* The one caller shape the reference holds for it (CBLSM/CBLSM.cpp:138-143, commented out; WTA :152):
 *   CrossAggregator a; a.Initialize(col, row, 0, dispRange); a.SetData(bytes_left, bytes_right, dispVolum);
 *   a.SetParams(option.cross_L1, option.cross_L2, option.cross_t1, option.cross_t2); a.Aggregate(4);
 *   cost = a.get_cost_ptr();  ComputeDispOringin(cost, disp, ...)
 * in one call: D = max_disparity - min_disparity, bytes_left uint8 [H][W][3], cost_init / cost_out float32
 * [H][W][D], disp float32 [H][W] (may be NULL).  Synchronising. */
int smt_adcensus_option_aggregate(const smt_adcensus_option *o, const uint8_t *bytes_left, const float *cost_init,
                                  int W, int H, int num_iters, float *cost_out, float *disp, void *stream);

/* ---- the same caller shape (CBLSM.cpp:133-143, 152) as a batched, device-resident flow: images in, maps out ---- */
typedef struct smt_crossagg_flow smt_crossagg_flow;
typedef struct smt_crossagg_flow_params {
    int L1, L2, t1, t2;   /* 34, 17, 20, 6   adcensus_types.h:69-70 */
    int num_iters;        /* 4               CBLSM.cpp:142 */
    int gate;             /* 5               CBLSM.cpp:155 */
} smt_crossagg_flow_params;
void smt_crossagg_flow_default_params(smt_crossagg_flow_params *p);
/* Owns one aggregated volume per view and one intermediate both views share: three float32 [H][W][D] volumes whatever
 * the batch size, plus arms, support counts and a gray pair.  p == NULL: the defaults.  SMT_ERR_ARG for NULL out,
 * non-positive sizes, D outside 1..SMT_MAX_DISPARITY, L1 outside 0..255 (arms are uint8), num_iters < 0 and a device
 * that does not exist. */
int smt_crossagg_flow_create_on(int device, int H, int W, int D, const smt_crossagg_flow_params *p, smt_crossagg_flow **out);
int smt_crossagg_flow_destroy(smt_crossagg_flow *h);
int smt_crossagg_flow_set_stream(smt_crossagg_flow *h, void *stream);
/* Per pair, in CBLSM.cpp's order:
 *   bgrL, bgrR     uint8 [pairs][H][W][3], the bytes of :72-87
 *   grayL, grayR   uint8 [pairs][H][W], the images after cvtColor (:21-22); both may be NULL together, the flow then
 *                  derives them with smt_bgr2gray's rule into buffers the handle owns
 *   views          SMT_VIEW_LEFT: ComputeAD (CBLSM.h:327-353; the chain for j - d < 0 is the right index max(j - d, 0)),
 *                  CrossAggregator::Aggregate(num_iters) with arms from bgrL, ComputeDispOringin -> dispL.
 *                  SMT_VIEW_RIGHT: ComputeADRight (:355-381, left index min(j + d, W - 1)), arms from bgrR, the same WTA
 *                  -> dispR.  The reference's commented lines run the left view only: the right view is this flow's own
 *                  composition of separately pinned stages, as CBLSM.cpp:146 is for the CBLSM flow.
 *   dispL, dispR   float32 [pairs][H][W], integer-valued; the map of a view that was not requested is not touched
 *   cls            non-NULL (both views only, else SMT_ERR_ARG): LeftRightConsistency(gate) (CBLSM.cpp:160) runs in
 *                  place on dispL through smt_lrcheck; cls uint8 [pairs][H][W], counts int32 [pairs][2] (may be NULL)
 * With num_iters >= 1 the first horizontal pass comes straight from the gray rows in integer arithmetic (the AD volume
 * never exists; exact, csrc/crossagg_first.h), the WTA sits in the last dividing pass, and that pass stores its volume
 * for the last pair only.  num_iters == 0 runs smt_cblsm_ad + smt_wta (the reference's result is the AD volume).
 * Asynchronous on the handle's stream only; one caller thread per handle; a warm call allocates nothing; pairs == 0 is a
 * no-op.  SMT_ERR_ARG for NULL handle or images, pairs < 0, views outside 1..3, a NULL map for a requested view and
 * exactly one gray pointer NULL. */
int smt_crossagg_flow_run_batch(smt_crossagg_flow *h, const uint8_t *bgrL, const uint8_t *bgrR,
                                const uint8_t *grayL, const uint8_t *grayR, int pairs, int views,
                                float *dispL, float *dispR, uint8_t *cls, int *counts);
/* the last pair's aggregated volumes (get_cost_ptr of each view), float32 [H][W][D], borrowed; a view that the last
 * call did not request keeps what it held */
int smt_crossagg_flow_volumes(smt_crossagg_flow *h, float **aggL, float **aggR);
/* Test and timing hook, per handle: 0 = fused kernels (default), 1 = the composed path inside the flow (smt_cblsm_ad,
 * smt_crossagg_aggregate's passes and smt_wta for every pair).  Identical bits. */
int smt_crossagg_flow_set_impl(smt_crossagg_flow *h, int impl);
/* Test hook, host only (no GPU): the integer form of the fused first pass, through the inline arithmetic the kernel
 * runs (csrc/crossagg_first.h), against sequential float sums over the chained ComputeAD / ComputeADRight volumes, both
 * views, random arms up to max_arm clipped to the row; fill 0 random bytes, 1 left all 255 and right all 0.  SMT_OK or
 * SMT_ERR_STATE; SMT_ERR_ARG for non-positive sizes, max_arm outside 0..255 and more than 2^24 hypotheses. */
int smt_crossagg_selftest_first_pass(int H, int W, int D, int max_arm, int fill, unsigned seed);

/* =====================================================================================
 * Window matchers                    replace SAD/Sad.h, NCC/NCC.h, ASW/ASW.h
 * 1 <= D <= SMT_MAX_DISPARITY on every entry point below (batch variants included); SMT_ERR_ARG beyond.
 * ===================================================================================== */
/* GetPointDepthLeft (Sad.h:96-139, view SMT_VIEW_LEFT, WTA = OptimalDisparity :40-85) /
 * GetPointDepthRight (:141-182, view SMT_VIEW_RIGHT, WTA = GetMinSadIndex :22-38).
 * Lp, Rp: uint8 [H+2w][W+2w] replicate-padded by w = winsize+1 (SADmain.cpp:47-48);
 * window side 2w+1.  disp: int32 [H][W] (right view leaves the last row/column 0). */
int smt_sad(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize, int view,
            int32_t *disp, void *stream);
/* Test hook (process-wide): 2 = window rows staged in LDS as byte-shifted dword copies, 32 pixels per workgroup
 * (default for windows of side >= 4), 1 = one wave per pixel straight from global memory (first formulation, and the
 * fallback for 3x3 windows).  Identical results. */
int smt_sad_set_impl(int impl);
/* CrossCheckDiaparity (Sad.h:184-222).  out int32 [H][W] (invalid = INT32_MIN, the x86
 * value of the reference's int(inf)); cls as smt_lrcheck. */
int smt_sad_crosscheck(const int32_t *dispL, const int32_t *dispR, int H, int W, int32_t *out,
                       uint8_t *cls, void *stream);

/* NCC_algorithem (NCC.h:69-95) = ComputeCost (:15-49, float64) + WinTakeAll (:53-67,
 * argMAX with a float32-narrowed running maximum).  L, R uint8 [H][W] unpadded; only the
 * interior winSize <= i < H-winSize, winSize <= j < W-winSize is written, the rest of
 * disp is set to 0.  cost (optional, may be NULL): float64 [H][W][D] per-hypothesis
 * costs for tolerance checks; the costs of the border pixels are 0.0. */
int smt_ncc(const uint8_t *L, const uint8_t *R, int H, int W, int D, int winSize, int32_t *disp,
            double *cost, void *stream);
/* Test hook (process-wide; SMT_NCC_IMPL in the environment overrides it): which formulation smt_ncc runs.
 *   2 (default)  window statistics once per image (k_ncc_stats) + the cross term Sab by v_dot4_u32_u8 (k_ncc2): windows up
 *                to 31x31, work per hypothesis side^2 / 4.
 *   3            the same statistics + Sab as a running box sum (k_ncc_box, csrc/ncc_box.hip): running sums down the
 *                rows, a sliding sum along the row, all in int32; the work per hypothesis does not grow with the window.
 *                Windows up to 181x181, where 255^2 side^2 < 2^31 keeps Sab, Saa and the statistics' int sums exact
 *                (2 130 284 025 at 181, 2 177 622 225 at 183).  Beyond that side the call runs the loop nest.
 *   1            the reference's loop nest, one lane per hypothesis (also the fallback of 2 and 3: wider windows, and
 *                when the scratch cannot be had).
 * 2 and 3 need 24*H*W bytes of stream-ordered scratch for the duration of the call and hand the same integers to the same
 * float64 expression: their costs and maps are equal bit for bit wherever both exist.  With n = side^2, each form is held
 * to the exact value of the rational function of the bytes: 2 and 3 within 2^-50 relative (integers below 2^53, then four
 * roundings), 1 within 4 n 2^-53 absolute (three length-n float64 sums) -- tests/exact_matchers.py -- and they give the
 * same NaN pattern, the integer statement A B == 0. */
int smt_ncc_set_impl(int impl);
/* Test hooks (process-wide, plain unsynchronised globals like smt_ncc_set_impl's).  smt_ncc_box_set_band: window rows per
 * band of the box kernel's grid, 0 (default) = chosen from the image size.  smt_ncc_last_form: which cost kernel the last
 * successful smt_ncc / smt_ncc_flow_run_batch of the process launched, one of SMT_NCC_FORM_* (0 before the first; a
 * call with an empty interior launches none and leaves it). */
#define SMT_NCC_FORM_LOOP 1   /* k_ncc: the reference's loop nest */
#define SMT_NCC_FORM_DOT4 2   /* k_ncc_stats + k_ncc2 */
#define SMT_NCC_FORM_BOX  3   /* k_ncc_stats + k_ncc_box */
int smt_ncc_box_set_band(int band);
int smt_ncc_last_form(void);
/* Test hook, host only (no GPU): on four unpadded pairs of the shape (pseudo-random, 255 against 255, opposed
 * checkerboards, a shifted copy) the box kernel's recurrence restated on the host -- same strips, bands, entering and
 * leaving rows, dword groups, sliding sum, clamped columns -- equals the direct double loop sum a*b for every (i, x, d),
 * under the band the launch would choose and under bands of 1 and 3 rows.  SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for
 * non-positive sizes, winSize < 0, side > 181, D > SMT_MAX_DISPARITY or more than 2^24 hypotheses. */
int smt_ncc_selftest_box(int H, int W, int D, int winSize, unsigned seed);

/* NCC/NCC_main.cpp:33 for `pairs` gray pairs uint8 [pairs][H][W]: disp int32 [pairs][H][W] (border pixels 0), cost
 * optional float64 [pairs][H][W][D] (border costs 0.0); per pair exactly what smt_ncc writes under the impl that matches
 * the form.  One statistics launch and one cost launch serve the whole batch, the pair on a grid axis.  The handle owns
 * the statistics tables (24*H*W bytes per pair, grown to the largest batch seen): a warm call neither allocates nor
 * synchronises.  At most 32767 pairs per call (the statistics launch carries two grid planes per pair); SMT_ERR_ARG beyond.
 * The tables are the handle's, not the call's: as with the other flow handles, consecutive calls on one handle must be
 * ordered on one stream -- after smt_ncc_flow_set_stream to another stream the caller orders the new stream behind the
 * work already enqueued.  Asynchronous on the handle's stream; pairs == 0 is a no-op; an empty interior (H <= 2 winSize or
 * W <= 2 winSize) gives all-zero maps and SMT_OK.  SMT_ERR_ARG for what smt_ncc rejects: non-positive sizes, NULL images
 * or map, winSize < 0, D outside 1..SMT_MAX_DISPARITY.
 * smt_ncc_flow_set_form: 0 (default) = the dispatch rule in csrc/ncc_box.hip, else SMT_NCC_FORM_*; SMT_ERR_ARG for a form
 * that does not cover the handle's window (DOT4 beyond 31x31, BOX beyond 181x181). */
typedef struct smt_ncc_flow smt_ncc_flow;
typedef struct smt_ncc_params { int winSize; } smt_ncc_params;                    /* 10: NCC_main.cpp:17 */
void smt_ncc_default_params(smt_ncc_params *p);
int smt_ncc_flow_create_on(int device, int H, int W, int D, const smt_ncc_params *p, smt_ncc_flow **out);
int smt_ncc_flow_destroy(smt_ncc_flow *h);
int smt_ncc_flow_set_stream(smt_ncc_flow *h, void *stream);
int smt_ncc_flow_set_form(smt_ncc_flow *h, int form);
int smt_ncc_flow_run_batch(smt_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *disp,
                           double *cost);

/* Both views of NCC from one pass over the costs.  The reference has no NCC right view; this one mirrors NCC.h:69-95 as
 * GetPointDepthRight mirrors GetPointDepthLeft.  For winSize <= i < H-winSize, winSize <= x < W-winSize:
 *   costR[i][x][d] = ComputeCost(R window centred (i, x), L window centred (i, x+d)) while x + winSize + d <= W-1, else the
 *                    `invalid` sentinel 255.0 (the mirror of j-winSize-d >= 0, NCC.h:81-89);
 *   dispR[i][x]    = WinTakeAll(costR[i][x][:]) (NCC.h:53-67: float-narrowed running maximum, the last hypothesis that
 *                    beats it wins, a NaN never wins, a NaN at d = 0 gives 0); border pixels: map 0, cost 0.0.
 * Equivalently dispR = fliplr(NCC_algorithem(fliplr(R), fliplr(L))).  dispL and costL are exactly what smt_ncc writes under
 * the impl in force (smt_ncc_set_impl); costL and costR are optional float64 [H][W][D].  Accepts and rejects what smt_ncc
 * does (both maps are required).  Scratch comes from the arena; asynchronous on `stream`.
 * Forms (smt_lrncc_set_impl: 0 = the dispatch rule, 1 = COMPOSED, 2 = KEYS wherever it exists; smt_lrncc_last_form reports
 * what the last successful call with a non-empty interior ran):
 *   KEYS      on the integer forms (impl 2 up to 31x31, impl 3 up to 181x181) the cost expression is symmetric in its two
 *             windows, so costR[i][x][d] == costL[i][x+d][d] bit for bit: the left cost kernel offers every real, non-NaN
 *             cost to right pixel x-d as a 64-bit rank key, combined per workgroup in LDS and then by one device-wide
 *             maximum per touched pixel in an [H][W] uint64 scratch map; a finishing launch names the winner (a NaN at
 *             d = 0 gives 0; a pixel with sentinel hypotheses gets the first of them, W - winSize - x).  costR is a
 *             diagonal gather of costL (held in scratch when the caller takes none).  8*H*W bytes of scratch more.
 *   COMPOSED  both images flipped on the device, the single-view path on the swapped pair, map and costs flipped back.
 *             The loop nest (impl 1, sides beyond the integer forms, no scratch) always takes it: its float64 sums are not
 *             symmetric.  Also the fallback when the key map cannot be had.
 * Both forms give identical bits on the integer kernels. */
#define SMT_LRNCC_FORM_COMPOSED 1
#define SMT_LRNCC_FORM_KEYS     2
int smt_lrncc(const uint8_t *L, const uint8_t *R, int H, int W, int D, int winSize, int32_t *dispL, int32_t *dispR,
              double *costL, double *costR, void *stream);
/* Test hooks (process-wide, plain unsynchronised globals): see smt_lrncc.  SMT_ERR_ARG outside 0..2. */
int smt_lrncc_set_impl(int impl);
int smt_lrncc_last_form(void);
/* Test hook, host only (no GPU): left costs [W - 2 winSize][D] of one row from a hostile palette chosen by seed % 4
 * (exact ties; doubles that round down and up to one float; NaN at d = 0 and d > 0; a mix) -- for every right pixel the
 * hypothesis the largest rank key names, with the NaN-at-0 and first-sentinel rules, equals the sequential WinTakeAll
 * of its row.  SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for non-positive sizes, winSize < 0, D > SMT_MAX_DISPARITY, W > 65536. */
int smt_lrncc_selftest_keys(int W, int D, int winSize, unsigned seed);

/* smt_lrncc for `pairs` gray pairs on the handle of smt_ncc_flow_run_batch, then per pair the int-map cross-check of
 * Sad.h:184-222 (NCC.h has none of its own; its maps are int like SAD's): dispL, dispR int32 [pairs][H][W], lastdisp and
 * cls exactly smt_sad_crosscheck of the call's own two maps.  Any output may be NULL (maps nobody takes live in arena
 * scratch; with every output NULL the call does nothing).  The left view is what smt_ncc_flow_run_batch writes under the
 * same smt_ncc_flow_set_form; one statistics launch serves both views under KEYS.  The handle's tables grow as in
 * smt_ncc_flow_run_batch: a warm call neither allocates nor synchronises.  Same limits: at most 32767 pairs, calls on one
 * handle ordered on one stream, pairs == 0 is a no-op, SMT_ERR_ARG for a NULL handle or image or pairs < 0. */
int smt_lrncc_flow_run_batch(smt_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, int32_t *dispL,
                             int32_t *dispR, int32_t *lastdisp, uint8_t *cls);

/* ncc() (NCC.h:117-272), the whole-image matcher NCC_main.cpp:24 calls in a commented line.  A different function from
 * NCC_algorithem: every pixel is written, and the reference has a right view of it.  L, R uint8 [H][W], k = kernel_size,
 * O = max_offset.  For pixel (y, x): rows sy = max(0, y-k) .. ey = min(H-1, y+k), columns sx .. ex likewise (:186-189);
 * the loops visit N = (ey-sy+1)(ex-sx+1) taps, the reference's count is n = (ey-sy)(ex-sx) (:190), one short per axis.
 * For o = 1 .. O the window holds two byte images:
 *   SMT_VIEW_LEFT  ("left")   a = L,  b = T:  T[y][c]  = R[y][c] for c < o, R[y][c-o] otherwise          (:147-158)
 *   SMT_VIEW_RIGHT ("right")  a = T', b = R:  T'[y][c] = L[y][c+o] for c < W-o, L[y][c] otherwise        (:162-173)
 * ma = sum a / n, mb = sum b / n (not the means: n != N); A = sum (a-ma)^2, B = sum (b-mb)^2, C = sum (a-ma)(b-mb), three
 * sequential float64 sums over the N taps, rows outer, each divided by n; res = C / (sqrt(A) sqrt(B)) / n (:224).  A running
 * maximum starts at -2.0 and o wins when res > max (:261-266): a NaN never wins and the first of equal costs stays.
 * depth uint8 [H][W] = (uchar)(3 o) of the winner, which wraps from o = 86 on; offset (optional, may be NULL) int32 [H][W]
 * = the winning o, 0 where no offset won; cost (optional, may be NULL) float64 [H][W][max_offset], index o-1 (a diagnostic
 * output: the INT form stores it with a stride of max_offset doubles across lanes, 1.5 to 1.7 times the maps-only call at 450x375).
 * Exact form: with the integer window sums and q = 2n - N, res = Ci / (n sqrt(Ai) sqrt(Bi)), Ai = n^2 Saa - q Sa^2,
 * Bi = n^2 Sbb - q Sb^2, Ci = n^2 Sab - q Sa Sb, evaluated as (double)Ci / ((double)n * (sqrt((double)Ai) * sqrt((double)Bi))).
 * Ai >= 0, and 0 only for an all-zero window; res is NaN exactly where Ai Bi = 0; |res| <= 1/n.  Every integer stays below
 * 2^53 for kernel_size <= 35 (the tight terms at k = 35: q Sa^2 <= 4759 * 255^2 * 71^4 = 7.864e15 and n^2 Saa <= 4900^2 *
 * 255^2 * 71^2 = 7.870e15, against 2^53 = 9.007e15; both pass it at k = 36; csrc/ncc_whole_rules.h has the arithmetic).
 * The expression is symmetric in a and b, so the left type's cost at (y, x, o) equals the right type's at (y, x-o, o) word
 * for word wherever x-k >= o and x+k <= W-1.
 * Forms (smt_whole_ncc_set_impl: 0 = the dispatch rule, 1 = LOOP, 2 = INT wherever it exists; smt_whole_ncc_last_form
 * reports what the last successful call ran; process-wide unsynchronised globals like smt_ncc_set_impl's):
 *   LOOP  :181-267 loop for loop, one lane per pixel: the independent formulation, and the only one for kernel_size > 35.
 *         The reference squares with pow(x, 2), this form with x * x: the same double wherever pow is correctly rounded
 *         for the exponent 2 (the recorded fixture pins the maps, not the costs).
 *   INT   the exact form: per-row prefix sums of the clamped vertical window sums of v and v^2 give Sa, Saa and the shifted
 *         image's Sb, Sbb as two or four loads per range; Sab is a running sum down the rows and a sum over the clamped
 *         columns, in uint32.
 * The two forms give the same NaN pattern and costs within their rounding bounds (tests/ncc_whole_cases.py derives them).
 * Decided defects.  (1) `Mat depth(height, width, 0)` is uninitialised in OpenCV: a pixel at which every offset is NaN
 * keeps garbage in the reference; here it is 0.  (2) For o > W the shift loops write outside tmp (:149, :169):
 * max_offset > W returns SMT_ERR_REF_UB before any launch; max_offset == W is defined (every column is fill).  (3) n = 0
 * needs a one-row or one-column window: H < 2, W < 2 or kernel_size < 1 is SMT_ERR_ARG.  (4) add_constant (:127-130) is
 * OpenCV's saturating `right += 10` and the reference applies it to the CALLER's image (`Mat right = in2` shares the data);
 * here min(R + 10, 255) goes to a scratch copy, for both views, and the caller's buffer stays as it is (parity unpinned,
 * like the other OpenCV restatements).
 * SMT_ERR_ARG also for NULL images or depth, a view other than SMT_VIEW_LEFT / SMT_VIEW_RIGHT, max_offset outside
 * 1 .. SMT_MAX_DISPARITY, H > 65535 or H * W >= 2^31.  params == NULL means the defaults (5, 79, 0: NCC.h:121-122).  Scratch
 * comes from the arena; asynchronous on `stream`.  (The entry points are named smt_whole_ncc*: the names that begin with
 * smt_ncc are NCC_algorithem's family, a closed list.) */
#define SMT_NCC_WHOLE_FORM_LOOP 1
#define SMT_NCC_WHOLE_FORM_INT  2
typedef struct smt_whole_ncc_params { int kernel_size, max_offset, add_constant; } smt_whole_ncc_params;
void smt_whole_ncc_default_params(smt_whole_ncc_params *p);
int smt_whole_ncc(const uint8_t *L, const uint8_t *R, int H, int W, const smt_whole_ncc_params *params, int view,
                  uint8_t *depth_u8, int32_t *offset_i32, double *cost_f64, void *stream);
/* Test hooks (process-wide, plain unsynchronised globals): see smt_whole_ncc.  SMT_ERR_ARG outside 0..2. */
int smt_whole_ncc_set_impl(int impl);
int smt_whole_ncc_last_form(void);
/* Test hook (process-wide, a plain unsynchronised global): into how many consecutive runs a cost launch splits the offsets
 * 1 .. max_offset (each workgroup keeps the winner of one run; a finishing launch combines the runs in their order), capped
 * at max_offset; 0 (default) = chosen from the size of the grid.  Every value gives the same maps and costs.  SMT_ERR_ARG
 * below 0.  smt_whole_ncc_last_groups: the number of runs of the last successful call (0 before the first). */
int smt_whole_ncc_set_groups(int groups);
int smt_whole_ncc_last_groups(void);
/* Test hook, host only (no GPU): on four pairs of the shape (pseudo-random, 255 against 255, opposed checkerboards, a
 * shifted copy) the INT kernel's recurrences restated on the host with the kernel's own index helpers
 * (csrc/ncc_whole_rules.h) -- tiles, row strips, halo lanes, entering and leaving rows, clamped column sums, the shifted
 * image's two ranges in the prefix tables -- equal the direct double loop over the shifted copy for Sab, Sb and Sbb at
 * every (y, x, o), fill columns and all four clamps included; and on hostile cost rows (exact ties, NaN first and later, all
 * NaN) the kernels' split of the offsets into G runs (nw_group) tiles 1 .. max_offset once and in order and the run-wise
 * winner (nw_offer) names the sequential loop's offset, for every G.  SMT_OK or SMT_ERR_STATE; rejects what smt_whole_ncc
 * rejects, and SMT_ERR_ARG for kernel_size > 35 or more than 2^22 hypotheses. */
int smt_whole_ncc_selftest_box(int H, int W, int kernel_size, int max_offset, int view, unsigned seed);
/* bgr_to_grey (NCC.h:97-115) for n images: BGR uint8 [n][H][W][3] -> uint8 [n][H][W].  Each channel is uchar(0.333 v),
 * truncated, from a 256-entry table made on the host with the reference's expression; the three are added (at most
 * 3 * 84: no wrap).  Not the rule of smt_bgr2gray.  n == 0 is a no-op; SMT_ERR_ARG for n < 0, non-positive sizes or NULL
 * buffers.  Asynchronous on `stream`. */
int smt_bgr_to_grey_batch(const uint8_t *bgr, int n, int H, int W, uint8_t *grey, void *stream);

/* NCC_main.cpp with :24 enabled, for both types and for `pairs` gray pairs uint8 [pairs][H][W]: depthL / depthR uint8 and
 * offL / offR int32 [pairs][H][W] are per pair bit for bit what smt_whole_ncc writes for SMT_VIEW_LEFT / SMT_VIEW_RIGHT under
 * the matching impl; then per pair the int-map cross-check of Sad.h:184-222 on the two OFFSET maps: lastdisp int32 and cls
 * uint8 [pairs][H][W] are exactly smt_sad_crosscheck of the call's own offL and offR.  Any output may be NULL (maps nobody
 * takes live in arena scratch; with every output NULL the call does nothing); pairs == 0 is a no-op.  One statistics launch
 * and one cost launch serve both views of the whole batch (the view and the pair on a grid axis); the right type's costs
 * are computed, not taken from the left pass.  The handle owns no device memory: every table comes from the arena, and the
 * call is asynchronous on the handle's stream.  create_on rejects what smt_whole_ncc rejects (SMT_ERR_REF_UB for
 * max_offset > W); set_form: 0 (default) = as smt_whole_ncc chooses, else SMT_NCC_WHOLE_FORM_*, SMT_ERR_ARG for INT with
 * kernel_size > 35.  At most 32767 pairs per call; SMT_ERR_ARG for a NULL handle or image or pairs < 0. */
typedef struct smt_whole_ncc_flow smt_whole_ncc_flow;
int smt_whole_ncc_flow_create_on(int device, int H, int W, const smt_whole_ncc_params *p, smt_whole_ncc_flow **out);
int smt_whole_ncc_flow_destroy(smt_whole_ncc_flow *h);
int smt_whole_ncc_flow_set_stream(smt_whole_ncc_flow *h, void *stream);
int smt_whole_ncc_flow_set_form(smt_whole_ncc_flow *h, int form);
int smt_whole_ncc_flow_run_batch(smt_whole_ncc_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, uint8_t *depthL,
                                 uint8_t *depthR, int32_t *offL, int32_t *offR, int32_t *lastdisp, uint8_t *cls);

/* getGausssianMask (ASW.h:16-35) and getColorMask (:41-47), computed on the HOST in
 * float64 exactly as the reference does.  space: (2*winSize+3)^2 doubles, color: 256. */
int smt_asw_masks(int winSize, double sigma_space, double sigma_color, double *space_host,
                  double *color_host);

/* AdaptiveSupportWeight (ASW.h:329-378, SMT_VIEW_LEFT) / AdaptiveSupportWeightRight
 * (:382-431, SMT_VIEW_RIGHT): bilateralfiterWight (:210-257) per hypothesis + WinTakeAll
 * (:193-208).  Lp, Rp: uint8 [H+2w][W+2w] replicate-padded by w = winSize+1
 * (ASWeight.cpp:54-57); space/color: DEVICE float64 tables from smt_asw_masks, (2*winSize+3)^2 and 256 entries, all of
 * which are read whatever the caller allocated; T: error
 * truncation.  disp float32 [H][W]; cost (optional) float32 [H][W][D]. */
int smt_asw(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winSize,
            const double *space, const double *color, int T, int view, float *disp, float *cost,
            void *stream);
/* Both views' maps from ONE evaluation of the hypotheses (ASWeight.cpp:60-61 without the second tap loop).  The weight of
 * a tap is one factor per image and the error min(|a - b|, T) is symmetric, so the right view's cost at column x' and
 * hypothesis d is the left view's at column x' + d.  Arguments, limits (D <= SMT_MAX_DISPARITY, winSize <= 30), scratch
 * arena and stream behaviour as smt_asw; costL / costR (float32 [H][W][D]) are optional.  With wins = winSize + 1:
 *   dispL, costL       exactly what smt_asw(..., SMT_VIEW_LEFT, ...) writes, bit for bit, under every smt_asw_set_impl
 *                      and for D > 256.
 *   costR[i][x'][d]    costL[i][x'+d][d] where x' + d <= W - wins - 2 (ASW.h:401 accepts d), otherwise costR[i][x'][d-1]
 *                      (the chain of :422-425); NaN for every d where x' > W - wins - 2 (the costVolume[-1] columns, where
 *                      smt_asw writes NaN too).
 *   dispR              WinTakeAll (ASW.h:193-208, first strict minimum) of that costR; 0 in the costVolume[-1] columns.
 * This is the reference's right view up to the rounding the library's ASW costs already carry: smt_asw's kernels fold the
 * weight product as (w0*space^2)*color, so a left cost and smt_asw's right cost of the same hypothesis may differ in the
 * last bit of the float64 sums.  dispR is therefore NOT promised to equal smt_asw(SMT_VIEW_RIGHT) bit for bit; it follows
 * from the left costs exactly and meets the bar of the other ASW entry points: every cost within ulp_f32 / 2 +
 * 4 n 2^-53 relative of the exact value (n = (2 winSize + 3)^2; tests/exact_matchers.py), hence equal or adjacent to the
 * oracle's float, and maps equal to the oracle's wherever its two smallest costs are more than 2 float ulps apart. */
int smt_asw_both(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winSize,
                 const double *space, const double *color, int T,
                 float *dispL, float *dispR, float *costL, float *costR, void *stream);
/* Test hook (process-wide): how smt_asw_both gets the right view.  2 (default) = rank keys: every hypothesis the left
 * view computes offers (ordered bits of its float cost) << 32 | d to right pixel x - d, minimum per workgroup in LDS, then
 * one agent-scope atomic min per touched pixel into an [H][W] key map (8 bytes per pixel of scratch), and a finishing
 * launch; no volume is written.  1 = the left view with its cost volume (in scratch when costL is NULL) and a
 * diagonal-gather WinTakeAll kernel.  costR always comes from 1.  Identical maps. */
int smt_asw_both_set_impl(int impl);
/* Test hook, host only (no GPU): on pseudo-random float cost rows of a W-column, D-hypothesis left volume (exact ties,
 * +-0.0, negative values, +inf, NaN at d = 0 and at d > 0) the minimum rank key over a right pixel's diagonal gives the
 * map of WinTakeAll over the chained right row.  SMT_OK or SMT_ERR_STATE. */
int smt_asw_selftest_right_keys(int W, int D, int wins, unsigned seed);
/* Scratch device memory of smt_asw / smt_ncc comes from an arena the library owns (csrc/scratch.hip: hipMalloc'ed
 * blocks cached per device and handed out stream-ordered on the caller's stream).  The arena keeps what it has grown
 * to -- the anchor weights of an smt_asw call (H*W*(2*winSize+3)^2*8 bytes while that is under 6 GiB, beyond it one
 * slot per workgroup in flight: 160 MB at 35 x 35 whatever the image size), 24*H*W bytes after an smt_ncc -- until the
 * process ends or the host asks
 * for it back: smt_scratch_trim synchronises the current device and returns every idle block beyond `keep_bytes` to
 * the driver (hipFree); smt_scratch_info reports what the arena holds / has handed out.  smt_scratch_poison (test hook)
 * synchronises the current device and fills every idle block of it with `byte` (hipMemset), so that the next call finds
 * hostile scratch instead of its own previous tables: SMT_OK, or SMT_ERR_STATE outside arena mode; no effect on any other
 * path (tests/test_bounds_gpu.py: results must not move with it).
 * Why not hipMallocAsync: on ROCm 7.2 a stream-ordered pool that trims and grows again hands out a block that is
 * zero-filled while the kernels already run on it (wrong ASW maps in round 2; tools/asw_bisect.py).
 * SMT_SCRATCH_MODE=pool|default|malloc (environment, for that tool) selects a never-trimming hipMemPool / the
 * device's default pool (the failing configuration) / plain hipMalloc per call. */
int smt_scratch_trim(size_t keep_bytes);
int smt_scratch_info(size_t *reserved_bytes, size_t *used_bytes);
int smt_scratch_poison(int byte);
/* Test hook (process-wide): which ASW formulation runs.  0 (default) = 3 while the whole-image anchor table stays
 * under 6 GiB (SMT_ASW_TABLE_MAX_MB), 6 beyond.  3 = per-row other-image weight tables in LDS, anchor weights from a
 * whole-image table written by a table kernel first (H*W*(2*winSize+3)^2*8 bytes of scratch: 5 GB at 960x540, 35x35),
 * two pixels per wave; 6 = the same tap loop with the anchor weights in one scratch slot per workgroup in flight, rebuilt
 * by the workgroup for every tile it takes (k_asw4: 160 MB at 35x35 whatever the image size, 7 % slower at config 4);
 * 4 = 3 with one pixel per wave; 5 = 3 with the anchor operands read by vector loads instead of through the scalar
 * cache; 1 = the first formulation (everything recomputed per tap; also the fallback when the scratch cannot be had).
 * All produce identical bits. */
int smt_asw_set_impl(int impl);
/* Batch variants of the three window matchers ("batch variants taking a pair count and strides"):
 * `pairs` image pairs and maps, consecutive pairs `img_stride` / `disp_stride` ELEMENTS apart (0 = dense: one
 * padded image, (H+2w)*(W+2w) bytes for SAD / ASW and H*W for NCC; one map, H*W).  Exactly the results of
 * `pairs` single calls, enqueued on `stream`; the per-call scratch of NCC / ASW is reused from pair to pair. */
int smt_sad_batch(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D, int winsize,
                  int view, int32_t *disp, size_t disp_stride, void *stream);
int smt_ncc_batch(const uint8_t *L, const uint8_t *R, int pairs, size_t img_stride, int H, int W, int D, int winSize,
                  int32_t *disp, size_t disp_stride, void *stream);
int smt_asw_batch(const uint8_t *Lp, const uint8_t *Rp, int pairs, size_t img_stride, int H, int W, int D, int winSize,
                  const double *space, const double *color, int T, int view, float *disp, size_t disp_stride,
                  void *stream);
/* CrossCheckDiaparity (ASW.h:108-145): float maps -> uint8 map, 0 = rejected. */
int smt_asw_crosscheck(const float *dispL, const float *dispR, int H, int W, uint8_t *out,
                       void *stream);

/* The active lines of ASW/ASWeight.cpp for a batch of gray pairs (uint8 [pairs][H][W], unpadded), per pair in the file's
 * order: copyMakeBorder of both images by winSize + 1 (:54-55), both views (:60-61, through smt_asw_both),
 * CrossCheckDiaparity (:66) into lastDisp, uint8 [pairs][H][W].  smt_asw_flow_run_batch stops at :66;
 * smt_asw_flow_run_batch_post (below) goes on through :67-78 (normalize, filterSpeckles, medianBlur, FillImageNew) and
 * reaches the end of the file.  The handle owns the two masks (smt_asw_masks, built and
 * uploaded once at create), the padded images and one pair of maps: a warm call allocates nothing beyond the scratch
 * arena.  Asynchronous on the handle's stream; pairs == 0 is a no-op; any of the three outputs may be NULL.
 * SMT_ERR_ARG for non-positive sizes, NULL inputs, winSize outside 1..30, D outside 1..SMT_MAX_DISPARITY and
 * non-positive sigmas. */
typedef struct smt_asw_flow smt_asw_flow;
typedef struct smt_asw_params { int winSize, T; double sigma_space, sigma_color; } smt_asw_params;  /* 11, 40, 50, 30: ASWeight.cpp:43-47 */
void smt_asw_default_params(smt_asw_params *p);
int smt_asw_flow_create_on(int device, int H, int W, int D, const smt_asw_params *p, smt_asw_flow **out);
int smt_asw_flow_destroy(smt_asw_flow *h);
int smt_asw_flow_set_stream(smt_asw_flow *h, void *stream);
int smt_asw_flow_run_batch(smt_asw_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                           float *dispL, float *dispR, uint8_t *lastDisp);

/* Both SAD maps from ONE evaluation of the hypotheses (SADmain.cpp:66-67).  Lp, Rp, H, W, D, winsize as smt_sad; every
 * argument smt_sad accepts is accepted, everything it rejects is rejected.
 *   dispL  int32 [H][W]      exactly smt_sad(..., SMT_VIEW_LEFT, ...)
 *   dispR  int32 [H][W]      exactly smt_sad(..., SMT_VIEW_RIGHT, ...) (last row / column 0, Sad.h:157,160)
 *   costL  float32 [H][W][D] optional: the left view's `sad` vector per pixel, chain entries included
 *                            (sad[d] = sad[d-1] for d > x, Sad.h:125-129); integer-valued
 * The right view's cost at (i, x', d) (Sad.h:173-174) is the left view's at (i, x' + d, d) -- sadvalue is an exact,
 * symmetric integer sum -- and every hypothesis the right view accepts (:167) is one the left view evaluates (:125), so
 * both maps equal smt_sad's bit for bit.  The costs come from a box-sum kernel (running column sums down the rows, a
 * sliding sum along the row: the work per hypothesis does not grow with the window) for windows up to 181 x 181
 * (winsize <= 89, where (cost << 9) | d fits 32 bits); larger windows, and the sizes the dispatch rule in
 * csrc/sad_both.hip names, run smt_sad once per view inside the call.  Needs 4 * H * W bytes of the scratch arena
 * (4 * H * W * D under smt_sad_both_set_impl(1) without costL). */
int smt_sad_both(const uint8_t *Lp, const uint8_t *Rp, int H, int W, int D, int winsize,
                 int32_t *dispL, int32_t *dispR, float *costL, void *stream);
/* Test hook (process-wide): how the box form gets the right view.  2 (default) = rank keys: every hypothesis offers
 * (cost << 9) | d to right pixel x - d, minimum per workgroup in LDS, one agent-scope atomic min per touched pixel into
 * an [H][W] uint32 key map, then a finishing launch.  1 = the left volume (in scratch when costL is NULL) and a
 * diagonal-gather minimum kernel.  Identical maps. */
int smt_sad_both_set_impl(int impl);
/* Test hooks (process-wide; plain unsynchronised globals like smt_sad_both_set_impl's: a test-only contract, not
 * thread-safe -- set them while no other thread is inside smt_sad_both).  smt_sad_both_set_dispatch: 0 (default) = the
 * dispatch rule, 1 = the box form wherever it covers the window, 2 = always the composed smt_sad calls.
 * smt_sad_both_set_band: rows per band of the box kernel's grid, 0 (default) = chosen from the image size (small
 * images get bands of one row, which never take a row out of the running sums).  smt_sad_both_last_form: what the last
 * successful smt_sad_both of the process ran, one of SMT_SAD_FORM_* (0 before the first call). */
#define SMT_SAD_FORM_COMPOSED   1   /* smt_sad per view */
#define SMT_SAD_FORM_BOX_KEYS   2   /* box kernel + rank keys */
#define SMT_SAD_FORM_BOX_VOLUME 3   /* box kernel + left volume + diagonal gather */
int smt_sad_both_set_dispatch(int mode);
int smt_sad_both_set_band(int band);
int smt_sad_both_last_form(void);
/* Test hooks, host only (no GPU).  smt_sad_selftest_box: on four padded pairs of the shape (pseudo-random, 0 against
 * 255, opposed checkerboards, a shifted copy) the box kernel's recurrence restated on the host -- same strips, bands,
 * entering and leaving rows, masked dword groups, sliding sum, chain -- equals the direct double loop for every
 * (i, x, d).  smt_sad_selftest_right_keys: the minimum key over a right pixel's diagonal is GetMinSadIndex
 * (Sad.h:22-38) of its chained row, with exact ties (seed % 3 == 0), all-equal rows (1) and costs at the window's
 * largest value (2).  SMT_OK or SMT_ERR_STATE; SMT_ERR_ARG for non-positive sizes, D > SMT_MAX_DISPARITY, windows the
 * box kernel does not cover, or (box) more than 2^24 hypotheses. */
int smt_sad_selftest_box(int H, int W, int D, int winsize, unsigned seed);
int smt_sad_selftest_right_keys(int W, int D, int winsize, unsigned seed);

/* SAD/SADmain.cpp with :67-68 enabled, for `pairs` gray pairs uint8 [pairs][H][W] (the images after imread(..., 0) /
 * cvtColor, :27-41), per pair in the file's order: copyMakeBorder by winsize + 1 (:47-48), both views (:66-67, through
 * smt_sad_both), CrossCheckDiaparity (:68).  dispL, dispR, lastdisp int32 [pairs][H][W]; cls uint8 [pairs][H][W] as
 * smt_sad_crosscheck; any output may be NULL.  The flow stops at :68: RemoveSpeckles at :69 reads an int Mat through
 * at<float>, and :71-78 are OpenCV calls and scan-order fillers.  The handle owns the padded images and one set of
 * maps: a warm call allocates nothing beyond the library's scratch arena.  Asynchronous on the handle's stream;
 * pairs == 0 is a no-op.  SMT_ERR_ARG for non-positive sizes, NULL inputs, winsize < 0 and D outside
 * 1..SMT_MAX_DISPARITY. */
typedef struct smt_sad_flow smt_sad_flow;
typedef struct smt_sad_params { int winsize; } smt_sad_params;                    /* 3: SADmain.cpp:34 */
void smt_sad_default_params(smt_sad_params *p);
int smt_sad_flow_create_on(int device, int H, int W, int D, const smt_sad_params *p, smt_sad_flow **out);
int smt_sad_flow_destroy(smt_sad_flow *h);
int smt_sad_flow_set_stream(smt_sad_flow *h, void *stream);
int smt_sad_flow_run_batch(smt_sad_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                           int32_t *dispL, int32_t *dispR, int32_t *lastdisp, uint8_t *cls);

/* =====================================================================================
 * Either side of the path: input staging and the first post-filter
 * ===================================================================================== */
/* Image files, HOST side (no GPU work): what the reference's drivers do with cv::imread(path) /
 * cv::imwrite(path, img) (AD-CensusV1/main.cpp:16-17, :115-117; SADmain.cpp:28-29; ASWeight.cpp:11-12),
 * without OpenCV / libpng / zlib.
 * smt_image_read: 8-bit PNG (colour types 0, 2, 3, 4, 6; bit depths 1-16 -- 16-bit samples keep their
 * high byte; alpha dropped; palettes expanded; non-interlaced) and binary PGM / PPM (P5 / P6).
 *   want_channels  3: always 3-channel B, G, R like cv::imread's default flag (a gray file is replicated);
 *                  1: gray (a colour file goes through the BGR2GRAY rule of smt_bgr2gray);
 *                  0: as stored (1 or 3).
 *   *pixels is malloc'd [H][W][channels]; release it with smt_image_free.
 * smt_image_write: by extension -- .png (8-bit gray or colour, filter 0, stored deflate blocks: valid,
 * uncompressed), .pgm / .ppm / .pnm; channels 1 or 3 (B, G, R in memory).
 * Both return SMT_ERR_ARG for unreadable / malformed / unsupported files. */
int smt_image_read(const char *path, int want_channels, uint8_t **pixels, int *H, int *W, int *channels);
int smt_image_free(uint8_t *pixels);
int smt_image_write(const char *path, const uint8_t *pixels, int H, int W, int channels);

/* cvtColor(CV_BGR2GRAY) as the drivers call it (AD-CensusV1/main.cpp:19-20): OpenCV 3.1.0's
 * 8-bit fixed-point rule (1868 B + 9617 G + 4899 R + 8192) >> 14.  bgr uint8 [H][W][3]. */
int smt_bgr2gray(const uint8_t *bgr, int H, int W, uint8_t *gray, void *stream);
/* copyMakeBorder(..., BORDER_REPLICATE) with equal borders (SADmain.cpp:47-48, ASWeight.cpp:54-57).
 * dst uint8 [H+2*pad][W+2*pad]. */
int smt_pad_replicate(const uint8_t *src, int H, int W, int pad, uint8_t *dst, void *stream);
/* uchar -> float image copy (main.cpp:46-55). */
int smt_u8_to_f32(const uint8_t *src, int H, int W, float *dst, void *stream);
/* MedianFilter(in, out, width, height, wnd_size) (AD-CensusV1/PostProcessing.h:314-344): median of
 * the in-image part of the window, element [n/2] of the ascending order.  wnd_size <= 7. */
int smt_median_filter(const float *in, float *out, int W, int H, int wnd_size, void *stream);
/* RemoveSpeckles(disparity_map, width, height, diff_insame, min_speckle_aera, invalid_val)
 * (AD-CensusV1/PostProcessing.h:250-311), in place.  invalid_val is an int as in the reference
 * (its call sites pass +inf: undefined conversion, INT_MIN on x86 when converted at run time.  A compiler that folds
 * the constant at the call site need not agree: g++ -O2 does not give INT_MIN for `RemoveSpeckles(..., Invalid_Float)`,
 * which is why the reference build used by the tests receives invalid_val as an int argument).  Synchronising. */
int smt_remove_speckles(float *disparity_map, int W, int H, int diff_insame, unsigned min_speckle_area,
                        int invalid_val, void *stream);
/* Batch forms, asynchronous: `pairs` maps `stride` / `disp_stride` ELEMENTS apart (0 = dense, H*W; otherwise >= H*W),
 * H*W < 2^31, enqueued on `stream` in a fixed number of launches (one for the median, four for the speckle filter)
 * whatever the data and the pair count.
 * smt_median_filter_batch: every map as smt_median_filter (in and out distinct).  Bit-identical to it and to
 *   MedianFilter on maps without NaN or -0.0, where the reference's std::sort order is defined.
 * smt_remove_speckles_batch: every map in place as smt_remove_speckles, bit for bit for every float input.  No host
 *   synchronisation and, once the library's scratch arena holds 10 * pairs * H * W bytes, no allocation.  err_dev
 *   (device int, may be NULL) is set nonzero if a kernel hits a loop cap (never expected; the maps are then
 *   unspecified); the caller clears it. */
int smt_median_filter_batch(const float *in, float *out, int pairs, size_t stride, int W, int H, int wnd_size,
                            void *stream);
int smt_remove_speckles_batch(float *disp, int pairs, size_t disp_stride, int W, int H, int diff_insame,
                              unsigned min_speckle_area, int invalid_val, int *err_dev, void *stream);
/* MedianFilter(d, d, width, height, wnd_size): the reference's filter called with in == out, as CBLSM.cpp:162 calls it
 * (`MedianFilter(dispLeft, dispLeft, col, row, 3)`).  That is NOT the out-of-place filter: PostProcessing.h:314-344 reads
 * `in` while it writes `out` in raster order, so the window of pixel (i, j) holds already-filtered values in the rows
 * above and to the left on its own row and unfiltered values elsewhere -- a recurrence.  These entries compute exactly
 * that, per map, bit for bit on maps without NaN or -0.0 (where the reference's std::sort order is defined; with them
 * the result is unspecified, as for smt_median_filter_batch); +inf is an ordinary value.  wnd_size 1..7; even sizes as
 * the reference: radius wnd_size / 2, window (2 * radius + 1)^2; wnd_size 1 leaves the map as it is.
 * Pixel (i, j) runs at step i * (radius + 1) + j: everything it reads filtered has a smaller step number, everything it
 * reads unfiltered is overwritten at a larger one (csrc/median_schedule.h).  One map belongs to
 * one workgroup (a thread per row, taller maps band after band), the batch is the parallel axis.  Asynchronous on
 * `stream`, one launch whatever the data and the pair count, no allocation, no scratch beyond LDS.
 * SMT_ERR_ARG, before any device work, for NULL disp, pairs <= 0, non-positive sizes, H*W >= 2^31, wnd_size outside
 * 1..7 and strides (in ELEMENTS, 0 = dense) below H*W.  smt_median_filter[_batch] keep rejecting in == out. */
int smt_median_filter_inplace(float *disp, int W, int H, int wnd_size, void *stream);
int smt_median_filter_inplace_batch(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, void *stream);
/* Test hook (process-wide, unsynchronised like smt_sad_set_impl): 0 (default) = a thread keeps its window in registers
 * and slides it; rows exchange the entering column through rings in LDS, one barrier per step; unfiltered values come
 * from a register run refilled by 16-byte loads two refills ahead.  1 = the plain formulation: every step reads its
 * window from global memory, barrier, writes, barrier.  Identical bits. */
int smt_median_inplace_set_impl(int impl);
/* Test hooks, host only (no GPU): the same schedule on HOST memory through the inline functions the kernels run
 * (csrc/median_schedule.h: step -> (row, column), bands, rings, refill points), which is what holds the schedule to the
 * oracle where there is no device.  Arguments and return values as smt_median_filter_inplace_batch; the formulation is
 * smt_median_inplace_set_impl's.  _ex names the formulation, the rows per band (0 = the kernel's: 1024 plain; 1022,
 * 1020, 506 for radius 1, 2, 3 of the ring form, which spends 2 * radius threads on halo rows; larger: SMT_ERR_ARG) and
 * the order in which the ring form's threads run inside a step (reverse != 0: descending). */
int smt_median_filter_inplace_host(float *disp, int pairs, size_t stride, int W, int H, int wnd_size);
int smt_median_filter_inplace_host_ex(float *disp, int pairs, size_t stride, int W, int H, int wnd_size, int impl, int band,
                                      int reverse);

/* The tail of CBLSM/CBLSM.cpp (:155, :160-162), which follows both flows built from that file:
 *   LeftRightConsistency(col, row, gate, dispLeft, dispRight, occlusion, mismatches)   5
 *   RemoveSpeckles(dispLeft, col, row, speckle_diff, speckle_min_area, speckle_invalid)   1, 50, INT_MIN
 *   MedianFilter(dispLeft, dispLeft, col, row, median_wnd)                              3, in == out
 * speckle_invalid is the x86 value of int(Invalid_Float = +inf), as in smt_post_params (see smt_remove_speckles). */
typedef struct smt_cblsm_post_params {
    int gate;
    int speckle_diff;
    unsigned speckle_min_area;
    int speckle_invalid;
    int median_wnd;         /* 1..7 */
} smt_cblsm_post_params;
void smt_cblsm_post_default_params(smt_cblsm_post_params *p);
/* :160-162 on `pairs` DEVICE maps, in that order: smt_lrcheck in place on every dispL (rejected -> +inf; cls uint8
 * [pairs][H][W] dense, required; counts int32 [pairs][2], may be NULL), then smt_remove_speckles_batch and
 * smt_median_filter_inplace_batch, each once for the whole batch.  dispL and dispR are `stride` ELEMENTS apart (0 =
 * dense, otherwise >= H*W); dispR is only read.  post == NULL: the defaults.  err_dev as smt_remove_speckles_batch.
 * Asynchronous on `stream`; scratch as smt_remove_speckles_batch.  pairs == 0 is a no-op.  SMT_ERR_ARG for NULL maps or
 * cls, pairs < 0, non-positive sizes, H*W >= 2^31, short strides and median_wnd outside 1..7. */
int smt_cblsm_tail_batch(float *dispL, const float *dispR, int pairs, size_t stride, int H, int W,
                         const smt_cblsm_post_params *post, uint8_t *cls, int *counts, int *err_dev, void *stream);
/* smt_cblsm_flow_run_batch / smt_crossagg_flow_run_batch (both views) for all pairs, then smt_cblsm_tail_batch once over
 * the batch -- after the batch and not after each pair, because the in-place median only fills the machine across
 * maps.  dispL ends as the finished map of CBLSM.cpp; dispR is what run_batch writes; cls, counts as smt_cblsm_tail_batch
 * (cls required).  On the handle's stream with run_batch's asynchrony contract; pairs == 0 is a no-op.  The
 * CrossAggregator flow takes the gate from `post` (the handle's own gate keeps serving run_batch only).  A speckle
 * kernel that hit its loop cap (never expected) makes the flow's *_status return SMT_ERR_STATE. */
int smt_cblsm_flow_run_batch_post(smt_cblsm_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs,
                                  float *dispL, float *dispR, uint8_t *cls, int *counts, const smt_cblsm_post_params *post);
int smt_crossagg_flow_run_batch_post(smt_crossagg_flow *h, const uint8_t *bgrL, const uint8_t *bgrR, const uint8_t *grayL,
                                     const uint8_t *grayR, int pairs, float *dispL, float *dispR, uint8_t *cls, int *counts,
                                     const smt_cblsm_post_params *post);
/* synchronising, read-and-clear: SMT_ERR_STATE if a speckle kernel of smt_crossagg_flow_run_batch_post hit its loop cap */
int smt_crossagg_flow_status(smt_crossagg_flow *h);
/* Test hook, host only (no GPU): checks that every 8-adjacent pixel pair of an H x W map lying in two different tiles
 * of smt_remove_speckles_batch is examined by exactly one thread of its border-merge kernel.  SMT_OK or SMT_ERR_STATE
 * (SMT_ERR_ARG unless 0 < H*W < 2^28). */
int smt_speckle_selftest_tiles(int H, int W);

/* =====================================================================================
 * The tail of ASW/ASWeight.cpp (:67-78) on the device (csrc/asw_tail.hip)
 * =====================================================================================
 *   :67-72  normalize(.., 0, 255, NORM_MINMAX) of dispLeft, dispRight, lastDisp and convertTo(CV_8UC1)
 *   :73     filterSpeckles(lastDisp, 0, 40, 2)
 *   :74     medianBlur(lastDisp, lastDisp, 5)            -> speckle.png
 *   :76     FillImageNew(lastDisp) (ASW/ASW.h:434-511)   -> filled.png
 *   :78     medianBlur(lastDisp, lastDisp, 3)            -> medain.png
 * Batch conventions, all entry points below, as smt_median_filter_batch: `pairs` maps `stride` ELEMENTS apart (0 =
 * dense, otherwise >= H*W), asynchronous on `stream`, a fixed number of launches whatever the data and the pair count,
 * no host synchronisation, no allocation once the scratch arena is warm.  SMT_ERR_ARG, before any device work, for NULL
 * maps, pairs <= 0, non-positive sizes, strides below H*W and H*W >= 2^28.
 *
 * The three OpenCV steps are "parity unpinned", like smt_bgr2gray: OpenCV's source is in neither tree, so the rules
 * below are this library's DEFINITION of the steps, restated from a reading of OpenCV 3.1 that no test could hold
 * against OpenCV itself.
 *
 * normalize(src, dst, 0, 255, NORM_MINMAX) + convertTo(CV_8UC1)  (3 launches; 8 * pairs bytes of scratch):
 *   smin, smax over the map; in double  scale = 255.0 * (smax - smin > DBL_EPSILON ? 1.0 / (smax - smin) : 0.0)  (the
 *   division correctly rounded) and  shift = 0.0 - smin * scale;  per pixel convertTo's  t = (float)v * (float)scale
 *   rounded to float, then  t + (float)shift  rounded to float (no fused multiply-add);  a uint8 destination takes
 *   saturate_cast<uchar>(t): round half to even, clamp to 0..255.  A constant map gives all zeros.
 *   smt_minmax_normalize_u8_batch: uint8 -> uint8, once, as :69 + :72 treat lastDisp.  in == out is allowed.
 *   smt_minmax_normalize_f32_u8_batch: float -> uint8, as :67-68 + :70-71 treat dispLeft / dispRight: the float result
 *     above is the normalised float map, the same rounding makes it uint8.  Every input must be finite (with a NaN or
 *     an infinity the result is unspecified). */
int smt_minmax_normalize_u8_batch(const uint8_t *in, uint8_t *out, int pairs, size_t stride, int H, int W, void *stream);
int smt_minmax_normalize_f32_u8_batch(const float *in, uint8_t *out, int pairs, size_t stride, int H, int W, void *stream);
/* filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on CV_8UC1, in place (parity unpinned): the connected components
 * of the 4-NEIGHBOUR graph whose edges join neighbours a, b with |a - b| <= maxDiff and neither equal to newVal; every
 * pixel of a component of AT MOST maxSpeckleSize pixels becomes newVal (its low byte).  The relation is symmetric, so
 * the order of traversal does not matter: this is smt_remove_speckles_batch's tiled union-find (four launches,
 * 10 * pairs * H * W bytes of scratch) instantiated for uint8 pixels, 4 neighbours and `<=`.  err_dev as
 * smt_remove_speckles_batch. */
int smt_filter_speckles_u8_batch(uint8_t *maps, int pairs, size_t stride, int W, int H, int newVal, int maxSpeckleSize,
                                 int maxDiff, int *err_dev, void *stream);
/* medianBlur(src, dst, ksize), uint8, ksize 3 or 5 (else SMT_ERR_ARG) (parity unpinned): the true median of the
 * ksize x ksize window under BORDER_REPLICATE; any H, W >= 1 (a window wider than the image is all border).  OpenCV
 * copies when src == dst, so "in place" means out of place: in != out here (SMT_ERR_ARG), smt_asw_tail_batch brings the
 * copy.  One launch, no scratch: a tile and its halo in LDS, four adjacent outputs per thread, selection by a min/max
 * network on packed 16-bit lanes (csrc/median_net.h; smt_median_blur_selftest_nets, host only, checks both networks on
 * every input of zeros and ones: SMT_OK or SMT_ERR_STATE). */
int smt_median_blur_u8_batch(const uint8_t *in, uint8_t *out, int pairs, size_t stride, int W, int H, int ksize,
                             void *stream);
int smt_median_blur_selftest_nets(void);
/* FillImageNew(disp) (ASW/ASW.h:434-511), uint8, in place, W <= 65535 (:480's 0xffff must end the right walk; wider:
 * SMT_ERR_ARG), as the reference's code behaves, not as it may have been meant.  A pixel is a hole when it is 0; the
 * holes are listed in raster order; every read is of the unmodified map.  With T(k) = k (k + 1) / 2, hole i at (r, c):
 *   1. left walk: probes columns c - T(k), k = 0, 1, ..; the first nonzero value is pushed to a list and the hole is
 *      done; a probe below column 0 abandons the walk;
 *   2. right walk: probes columns c + T(k): a column > W pushes 0; a nonzero value is pushed; column == W IS READ -- the
 *      first pixel of row r + 1 -- and if that byte is 0 the walk ends with NOTHING pushed;
 *   3. hole i receives list[i], not its own value: after one hole that pushed nothing, every later hole of the map
 *      receives the value found for a later pushing hole, and the last holes index past the list's end.
 * Two reads are undefined in the reference and defined here: the byte at (H - 1, W), one past the buffer, reads as 0;
 * a hole whose index is at or past the list's length keeps 0.
 * fix: 0, or SMT_ASW_FIX_FILL_ROW_END: column == W counts as outside and pushes 0 like every column past it.  Every
 * hole then pushes exactly once, nothing shifts and no row reads its neighbour.  Unknown bits: SMT_ERR_ARG.
 * counts: int32 [pairs][2], may be NULL: the holes that pushed nothing, and the holes left 0 for want of a list entry
 * (the two are equal by construction: the list is short by one entry per missing push).  (0, 0) means the reference's
 * own run was defined.
 * Three launches (per row the search and the row's counts; per map the scan of the row counts; per row the gather);
 * pairs * (H * W + 16 * H) bytes of scratch or so.
 * smt_fill_image_new_host: the same rules on HOST memory through csrc/fill_image_rules.h, no GPU. */
#define SMT_ASW_FIX_FILL_ROW_END 0x1u
int smt_fill_image_new_batch(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts,
                             void *stream);
int smt_fill_image_new_host(uint8_t *maps, int pairs, size_t stride, int H, int W, unsigned fix, int *counts);
/* ASWeight.cpp:73-78's arguments.  fix: SMT_ASW_FIX_* (a field of its own: the bits of SMT_QUIRK_FIX_* belong to other
 * handles). */
typedef struct smt_asw_post_params {
    int speckle_newval, speckle_max_size, speckle_max_diff;     /* 0, 40, 2   :73 */
    int median_first, median_last;                              /* 5, 3       :74, :78; each 3 or 5 */
    unsigned fix;                                               /* 0 */
} smt_asw_post_params;
void smt_asw_post_default_params(smt_asw_post_params *p);
/* :69 + :72 and :73-78 in place on `pairs` uint8 DEVICE maps (lastDisp as smt_asw_crosscheck wrote it), each step once
 * over the batch.  after_median / after_fill: optional uint8 copies, `stride` apart like lastDisp, of the states the
 * driver writes as speckle.png and filled.png.  fill_counts as smt_fill_image_new_batch's counts, err_dev as
 * smt_remove_speckles_batch's; post == NULL: the defaults.  pairs == 0 is a no-op.  SMT_ERR_ARG also for W > 65535,
 * medians other than 3 or 5 and unknown fix bits.  14 launches with both copies. */
int smt_asw_tail_batch(uint8_t *lastDisp, int pairs, size_t stride, int H, int W, const smt_asw_post_params *post,
                       uint8_t *after_median, uint8_t *after_fill, int *fill_counts, int *err_dev, void *stream);
/* smt_asw_flow_run_batch for all pairs, then :67-68 + :70-71 into dispL8 / dispR8 (uint8 [pairs][H][W], each optional
 * and then needing its float map: dispL8 without dispL is SMT_ERR_ARG), then smt_asw_tail_batch ONCE over the batch on
 * lastDisp (required, dense).  dispL / dispR stay the un-normalised float maps run_batch writes.  On the handle's
 * stream, with run_batch's asynchrony contract; pairs == 0 is a no-op.  A speckle kernel that hit its loop cap (never
 * expected) makes smt_asw_flow_status return SMT_ERR_STATE (synchronising, read-and-clear). */
int smt_asw_flow_run_batch_post(smt_asw_flow *h, const uint8_t *grayL, const uint8_t *grayR, int pairs, float *dispL,
                                float *dispR, uint8_t *lastDisp, uint8_t *dispL8, uint8_t *dispR8,
                                const smt_asw_post_params *post, uint8_t *after_median, uint8_t *after_fill,
                                int *fill_counts);
int smt_asw_flow_status(smt_asw_flow *h);

#ifdef __cplusplus
}
#endif
#endif /* SMT_H_ */
