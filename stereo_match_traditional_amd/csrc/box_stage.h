// The staged-row box-sum engine, once: the geometry of a staged row, the tap policies (what one dword group, the tail
// group and one sliding step add), box_steps -- the staging of two image rows per step, the horizontal window sums of a
// staged row and the step loop of a band --, the slot-count dispatch, the band rule of the grids and box_host<Tap>, the
// host restatement that the selftests of the SAD and NCC kernels run.  k_ncc_box (csrc/ncc_box.hip) and k_win_box
// (csrc/cblsm_window.hip) run box_steps and keep what they do with a finished box sum -- the emit step, the key rows.
// k_sad_box (csrc/sad_both.hip) uses everything here but box_steps: its own copy of that skeleton compiles to the code it
// had, box_steps did not.
#pragma once
#include "smt_common.h"
#include <algorithm>
#include <type_traits>
#include <vector>

#ifdef __HIPCC__
#define BOX_HD __host__ __device__
#else
#define BOX_HD
#endif

namespace {

// Staged row geometry, shared by the kernels and the host restatement.  A row of either image sits in LDS expanded to one
// dword per BYTE offset (entry A = bytes A .. A + 3, as k_sad2 stages its rows): the initial window sum of a row reads
// aligned dwords for v_sad_u8 / v_dot4 whatever the hypothesis, the sliding sum reads the low byte of an entry, and lanes
// with consecutive d touch consecutive dwords (one bank each; the first image's entry is one address for the wave, a
// broadcast).  bsw: columns per workgroup.  The first image's entries start Tap::LEAD columns before the strip, the
// second's 64 KT columns before it (or, indexed by +d, where the first's start): the base columns a kernel hands to
// box_steps.  Columns outside the image are clamped into the row, for the entering and the leaving row alike: the clamped
// bytes are only read by hypotheses whose cost is replaced -- the chain of Sad.h:125-129, the sentinel of NCC.h:88.
BOX_HD inline int box_lwe(int side, int bsw) { return (bsw + side + 3) & ~3; }
BOX_HD inline int box_rwe(int side, int KT, int bsw) { return (64 * KT + bsw + side + 3) & ~3; }

// Tap policies.  acc4: one dword group of a window's first sum.  The side & 3 columns that the full groups leave are one
// more dword, at entry tail_at(at, side) for a window that starts at entry `at`, its first-image operand masked with
// tail_mask, its second-image operand passed through tail_b.  slide: the window moves one column (N enters, O leaves;
// one byte each).  The kernels' address arithmetic is sensitive to how these sums are associated: keep the forms.
// sum |a - b|: k_win_box.  k_sad_box's own row_pass states the same rule with the builtin (through this struct its streams
// are no longer the parent's)
struct box_tap_sad {
    static constexpr int LEAD = 1;                             // the masked tail dword of a 3-wide window starts one byte before it
    BOX_HD static unsigned acc4(unsigned a, unsigned b, unsigned acc)
    {
#ifdef __HIP_DEVICE_COMPILE__
        return __builtin_amdgcn_sad_u8(a, b, acc);
#else
        for (int q = 0; q < 4; q++) acc += (unsigned)abs((int)((a >> (8 * q)) & 255) - (int)((b >> (8 * q)) & 255));
        return acc;
#endif
    }
    // the last dword ends at the window's last byte; the bytes already counted are masked out of both operands
    BOX_HD static int tail_at(int at, int side) { return at + side - 4; }
    BOX_HD static unsigned tail_mask(int rem) { return rem ? (0xffffffffu << (8 * (4 - rem))) : 0u; }
    BOX_HD static unsigned tail_b(unsigned b, unsigned mask) { return b & mask; }
    BOX_HD static unsigned slide(unsigned aN, unsigned bN, unsigned aO, unsigned bO, unsigned run)
    {
        return acc4(aN, bN, run) - acc4(aO, bO, 0u);
    }
};

struct box_tap_dot {                                           // sum a b, exact modulo 2^32: k_ncc_box
    static constexpr int LEAD = 0;
    BOX_HD static unsigned acc4(unsigned a, unsigned b, unsigned acc)
    {
#ifdef __HIP_DEVICE_COMPILE__
        return __builtin_amdgcn_udot4(a, b, acc, false);
#else
        for (int q = 0; q < 4; q++) acc += ((a >> (8 * q)) & 255u) * ((b >> (8 * q)) & 255u);
        return acc;
#endif
    }
    // the window's last rem columns are the low bytes of one more dword; a zero byte on the left takes the right one out
    // of the sum
    BOX_HD static int tail_at(int at, int side) { return at + 4 * (side >> 2); }
    BOX_HD static unsigned tail_mask(int rem) { return (1u << (8 * rem)) - 1u; }
    BOX_HD static unsigned tail_b(unsigned b, unsigned) { return b; }
    BOX_HD static unsigned slide(unsigned aN, unsigned bN, unsigned aO, unsigned bO, unsigned run)
    {
        // one byte per operand: two single products, through the intrinsic on purpose.  Written as plain multiplies, the
        // compiler (ROCm 7.2) folds the products of neighbouring columns into v_dot4 of v_perm-packed bytes, and in the
        // KT = 1 instantiation the packed operands take in a leaving pair (aO, bO), whose product is then added instead
        // of subtracted (tools/dot4_fold_probe.hip)
        return acc4(aN, bN, run) - acc4(aO, bO, 0u);
    }
};

#ifdef __HIPCC__
#define BOX_DEV __device__ __forceinline__

// bytes x .. x + 7 of an image row of Wp columns as two dwords, columns clamped into the row
BOX_DEV void box_load8(const uint8_t *__restrict__ row, int x, int Wp, unsigned &lo, unsigned &hi)
{
    if (x >= 0 && x + 7 <= Wp - 1) {
        __builtin_memcpy(&lo, row + x, 4);
        __builtin_memcpy(&hi, row + x + 4, 4);
    } else {
        lo = hi = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            int xa = x + b, xb = x + 4 + b;
            xa = xa < 0 ? 0 : (xa > Wp - 1 ? Wp - 1 : xa);
            xb = xb < 0 ? 0 : (xb > Wp - 1 ? Wp - 1 : xb);
            lo |= (unsigned)row[xa] << (8 * b);
            hi |= (unsigned)row[xb] << (8 * b);
        }
    }
}

struct box_no_hook {
    template <class... T> BOX_DEV void operator()(T &&...) const {}
};

// One workgroup's band: output rows i0 .. i1 - 1 of the strip of BS (NT / 64) columns at x0, image rows A and B of `pitch`
// bytes, ncols output columns in all.  A lane owns the hypotheses d = lane + 64 k, k < nk, and reads image B at column
// x - d (DIR < 0) or x + d (DIR > 0).  Step t brings in image row i0 + t, takes out image row i0 + t - side (once there is
// one) and, from t = side - 1 on, emits output row io = i0 + t - side + 1.  The two rows of step t + 1 are fetched into
// registers before step t computes and written to the other half of the LDS row buffer s_rows ([2 halves][entering,
// leaving][box_lwe entries of A from column xAb + box_rwe entries of B from column xBb]) after it; one barrier per step.
// The kernel's parts are closures, inlined by force (the compiler inlines the closures below, called from here alone,
// as it did in the kernels); the running sums C stay in registers:
//   pre(half, io)             every thread, after the fetch and before the row passes
//   acc(t, leaving)           live waves, after the row passes
//   emit(half, io, x, C[j])   live waves, per column x < ncols of an output row: C[j][k] is the box sum of slot k
// Two things keep the code the kernels had before they shared this function (DESIGN.md section 5.16 has the register
// counts).  The base columns come from the kernel as values: written here as x0 - Tap::LEAD, their constants are folded
// into every entry index and k_win_box<2, 0, *> loses a wave per SIMD.  And a closure that needs the lane takes
// threadIdx.x & 63 itself: a captured `lane` is known to be below 64 only late, its comparisons against x are rewritten
// per column and hoisted, and k_win_box<8, 0, *> loses a wave per SIMD.
template <int KT, int BS, int NT, class Tap, int DIR, class Pre, class Acc, class Emit>
BOX_DEV void box_steps(unsigned *s_rows, const uint8_t *A, const uint8_t *B, int pitch, int xAb, int xBb, int x0, int i0, int i1,
                       int ncols, int side, int nk, const Pre &pre, const Acc &acc, const Emit &emit)
{
    constexpr int BSW = BS * (NT / 64);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int LWE = box_lwe(side, BSW), RWE = box_rwe(side, KT, BSW), ROWE = LWE + RWE;

    // staging: one item = four consecutive entries (two unaligned dword loads, three v_alignbyte, one 16-byte store).
    // Items of a step: entering row of A, entering row of B, leaving row of A, leaving row of B; at most 2 per thread.
    const int nL4 = LWE >> 2, nR4 = RWE >> 2, nrow4 = nL4 + nR4;
    unsigned slo[2], shi[2];
    auto fetch = [&](int t) {
        const int rE = i0 + t, rL = rE - side;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * NT;
            slo[q] = shi[q] = 0;
            if (e < 2 * nrow4) {
                const int which = e >= nrow4, f = e - which * nrow4;
                const int r = which ? rL : rE;
                if (!which || rL >= i0) {
                    const bool second = f >= nL4;
                    const int x = second ? xBb + 4 * (f - nL4) : xAb + 4 * f;
                    box_load8((second ? B : A) + (size_t)r * pitch, x, pitch, slo[q], shi[q]);
                }
            }
        }
    };
    auto commit = [&](int half) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int e = threadIdx.x + q * NT;
            if (e < 2 * nrow4)
                *reinterpret_cast<u4v *>(s_rows + (size_t)half * 2 * ROWE + 4 * e) =
                    u4v{slo[q], __builtin_amdgcn_alignbyte(shi[q], slo[q], 1), __builtin_amdgcn_alignbyte(shi[q], slo[q], 2),
                        __builtin_amdgcn_alignbyte(shi[q], slo[q], 3)};
        }
    };
    fetch(0);
    commit(0);
    __syncthreads();

    const int xw = x0 + BS * wv;                               // this wave's first column
    const bool live = xw < ncols;
    const int nfull = side >> 2, rem = side & 3;
    const unsigned tmask = Tap::tail_mask(rem);
    const int la = xw - xAb;                                   // A's entry of column xw
    int ra[KT];                                                // B's entry of column xw - d / xw + d
    unsigned C[BS][KT];
#pragma unroll
    for (int k = 0; k < KT; k++) {
        ra[k] = DIR < 0 ? xw - xBb - (lane + 64 * k) : xw - xBb + (lane + 64 * k);
#pragma unroll
        for (int j = 0; j < BS; j++) C[j][k] = 0;
    }
    // horizontal window sums of one staged row over the wave's BS columns, added to (SUB = false) or taken from C
    auto row_pass = [&](const unsigned *Arow, const unsigned *Brow, auto sub) {
        constexpr bool SUB = decltype(sub)::value;
        unsigned run[KT];
#pragma unroll
        for (int k = 0; k < KT; k++) run[k] = 0;
        for (int g = 0; g < nfull; g++) {
            const unsigned a4 = Arow[la + 4 * g];
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = Tap::acc4(a4, Brow[ra[k] + 4 * g], run[k]);
        }
        if (rem) {
            const unsigned a4 = Arow[Tap::tail_at(la, side)] & tmask;
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) run[k] = Tap::acc4(a4, Tap::tail_b(Brow[Tap::tail_at(ra[k], side)], tmask), run[k]);
        }
        const uint8_t *Ab = reinterpret_cast<const uint8_t *>(Arow), *Bb = reinterpret_cast<const uint8_t *>(Brow);
#pragma unroll
        for (int j = 0; j < BS; j++) {
            if (j > 0) {
                const unsigned aN = Ab[4 * (la + j - 1 + side)], aO = Ab[4 * (la + j - 1)];
#pragma unroll
                for (int k = 0; k < KT; k++)
                    if (k < nk) {
                        const unsigned bN = Bb[4 * (ra[k] + j - 1 + side)], bO = Bb[4 * (ra[k] + j - 1)];
                        run[k] = Tap::slide(aN, bN, aO, bO, run[k]);
                    }
            }
#pragma unroll
            for (int k = 0; k < KT; k++)
                if (k < nk) C[j][k] = SUB ? C[j][k] - run[k] : C[j][k] + run[k];
        }
    };

    const int nsteps = side - 1 + (i1 - i0);
    for (int t = 0; t < nsteps; t++) {
        const int half = t & 1;
        const int io = i0 + t - side + 1;                      // output row of this step (>= i0: there is one)
        const bool leaving = t >= side;
        if (t + 1 < nsteps) fetch(t + 1);
        pre(half, io);
        if (live) {
            const unsigned *rows = s_rows + (size_t)half * 2 * ROWE;
            row_pass(rows, rows + LWE, std::false_type());
            if (leaving) row_pass(rows + ROWE, rows + ROWE + LWE, std::true_type());
            acc(t, leaving);
            if (io >= i0) {
#pragma unroll
                for (int j = 0; j < BS; j++) {
                    const int x = xw + j;
                    if (x >= ncols) break;
                    emit(half, io, x, C[j]);
                }
            }
        }
        if (t + 1 < nsteps) commit(half ^ 1);
        __syncthreads();
    }
}
#endif  // __HIPCC__

// The slot count KT in {1, 2, 4, 8} that serves D hypotheses, and f(std::integral_constant<int, KT>()) for it
inline int box_kt(int D)
{
    const int K = (D + 63) / 64;
    return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : 8;
}
template <class F>
inline int box_dispatch_kt(int D, F &&f)
{
    switch (box_kt(D)) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// Rows per band of an H x W output grid cut into strips of `bsw` columns.  The cost model counts row passes per
// workgroup -- one per step while a band only adds (its first side - 1 steps), two once a row leaves: 2 band + side - 1 --
// times the rounds the grid needs if the device holds 1024 workgroups at a time.  That 1024 (256 CUs x 4) is an
// assumption, not a measurement: the KT >= 4 instantiations run one workgroup per CU, so for D > 128 the model
// over-estimates the residency four times.
inline int box_band(int H, int W, int side, int bsw)
{
    const long strips = (W + bsw - 1) / bsw;
    int best = H;
    long best_cost = -1;
    for (int band = 1; band <= H; band++) {
        const long wgs = strips * ((H + band - 1) / band);
        const long cost = (2L * band + side - 1) * ((wgs + 1023) / 1024);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = band; }
    }
    return best;
}
// the band of a launch: a test hook's override (> 0) clamped to the row count, else box_band's choice
inline int box_band_rule(int override_rows, int H, int W, int side, int bsw)
{
    return override_rows > 0 ? (override_rows < H ? override_rows : H) : box_band(H, W, side, bsw);
}

struct host_rng {
    uint64_t s;
    explicit host_rng(unsigned seed) : s(0x9E3779B97F4A7C15ull ^ ((uint64_t)seed * 0xD1342543DE82EF95ull + 1)) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }
};

// box_steps on the host, hypothesis by hypothesis, for 16 columns per wave and 256 threads (k_sad_box, k_ncc_box): the same
// strips, bands, steps, staged entries (clamped columns included), sliding sums and entering and leaving rows, the dword
// groups and the tail rule through Tap's host form, all in uint32.  A, B: image rows of `pitch` bytes; the second image
// at x - d.  out: [nrows][ncols][D] box sums, no chain applied.
template <class Tap>
void box_host(const uint8_t *A, const uint8_t *B, int pitch, int nrows, int ncols, int D, int side, int band, unsigned *out)
{
    constexpr int BS = 16, BSW = 64;
    const int KT = box_kt(D);
    const int LWE = box_lwe(side, BSW), RWE = box_rwe(side, KT, BSW);
    const int nfull = side >> 2, rem = side & 3;
    const unsigned tmask = Tap::tail_mask(rem);
    std::vector<unsigned> eL(LWE), eR(RWE), lL(LWE), lR(RWE), C((size_t)BS * 64 * KT);
    auto stage = [&](std::vector<unsigned> &dst, const uint8_t *row, int xb) {
        for (size_t e = 0; e < dst.size(); e++) {
            unsigned v = 0;
            for (int b = 0; b < 4; b++) {
                int x = xb + (int)e + b;
                x = x < 0 ? 0 : (x > pitch - 1 ? pitch - 1 : x);
                v |= (unsigned)row[x] << (8 * b);
            }
            dst[e] = v;
        }
    };
    for (int i0 = 0; i0 < nrows; i0 += band) {
        const int i1 = i0 + band < nrows ? i0 + band : nrows;
        for (int x0 = 0; x0 < ncols; x0 += BSW) {
            const int xLb = x0 - Tap::LEAD, xRb = x0 - 64 * KT;
            for (int xw = x0; xw < x0 + BSW && xw < ncols; xw += BS) {
                std::fill(C.begin(), C.end(), 0u);
                const int la = xw - xLb;
                const int nsteps = side - 1 + (i1 - i0);
                for (int t = 0; t < nsteps; t++) {
                    const int rE = i0 + t, rL = rE - side, io = rE - side + 1;
                    stage(eL, A + (size_t)rE * pitch, xLb);
                    stage(eR, B + (size_t)rE * pitch, xRb);
                    if (rL >= i0) { stage(lL, A + (size_t)rL * pitch, xLb); stage(lR, B + (size_t)rL * pitch, xRb); }
                    for (int d = 0; d < D; d++) {
                        const int ra = xw - xRb - d;
                        for (int pass = 0; pass < (rL >= i0 ? 2 : 1); pass++) {
                            const unsigned *Lrow = pass ? lL.data() : eL.data(), *Rrow = pass ? lR.data() : eR.data();
                            unsigned run = 0;
                            for (int g = 0; g < nfull; g++) run = Tap::acc4(Lrow[la + 4 * g], Rrow[ra + 4 * g], run);
                            if (rem)
                                run = Tap::acc4(Lrow[Tap::tail_at(la, side)] & tmask, Tap::tail_b(Rrow[Tap::tail_at(ra, side)], tmask), run);
                            for (int j = 0; j < BS; j++) {
                                if (j > 0)
                                    run = Tap::slide(Lrow[la + j - 1 + side] & 255u, Rrow[ra + j - 1 + side] & 255u,
                                                     Lrow[la + j - 1] & 255u, Rrow[ra + j - 1] & 255u, run);
                                unsigned &c = C[(size_t)j * 64 * KT + d];
                                c = pass ? c - run : c + run;
                            }
                        }
                    }
                    if (io < i0) continue;
                    for (int j = 0; j < BS && xw + j < ncols; j++)
                        for (int d = 0; d < D; d++) out[((size_t)io * ncols + xw + j) * D + d] = C[(size_t)j * 64 * KT + d];
                }
            }
        }
    }
}

}  // namespace

#undef BOX_HD
#undef BOX_DEV
