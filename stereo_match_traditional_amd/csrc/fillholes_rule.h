// FillHolesInDispMap (SAD/Sad.h:317-400; include/smt_fill_holes.h has the rule in words) as host/device inline
// functions: the one text that the kernel of fillholes.hip and the host twin run -- the sixteen constants, the ray step,
// the collection along the eight rays and the choice among the collected values.
#pragma once
#include <stdint.h>

namespace fhrule {

#if defined(__HIPCC__)
#define FH_HD __host__ __device__ __forceinline__
#else
#define FH_HD static inline
#endif

constexpr int RAYS = 8;
constexpr int SKEW = 2;                      // pixel (i, j) of a pass runs at wavefront step SKEW * i + j

// Sad.h:326-327, 363-364: pi = 3.1415926f, angle1 = {pi, 3*pi/4, pi/2, pi/4, 0, 7*pi/4, 3*pi/2, 5*pi/4} evaluated in
// float32, sina = sinf(angle), cosa = cosf(angle) (std::sin / std::cos of a float).  The values are glibc's, which are
// correctly rounded here; against MSVC's libm the last ulp is unpinned.  angle2 (Sad.h:328) holds the same eight angles
// in another order.
//   ray   0 left   1 down-left   2 down   3 down-right   4 right   5 up-right   6 up   7 up-left
FH_HD float sina(int ray)
{
    switch (ray) {
    case 0: return 0x1.4442d2p-23f;          // sinf(pi) > 0: the ray stays on its row
    case 1: return 0x1.6a09e6p-1f;
    case 2: return 0x1p+0f;
    case 3: return 0x1.6a09e6p-1f;
    case 4: return 0x0p+0f;
    case 5: return -0x1.6a09eap-1f;
    case 6: return -0x1p+0f;
    default: return -0x1.6a09ep-1f;
    }
}
FH_HD float cosa(int ray)
{
    switch (ray) {
    case 0: return -0x1p+0f;
    case 1: return -0x1.6a09e6p-1f;
    case 2: return 0x1.4442d2p-24f;          // cosf(pi/2) > 0: the ray stays on its column
    case 3: return 0x1.6a09e8p-1f;
    case 4: return 0x1p+0f;
    case 5: return 0x1.6a09e2p-1f;
    case 6: return 0x1.99bc5cp-27f;          // cosf(3*pi/2) > 0
    default: return -0x1.6a09eep-1f;
    }
}

// Sad.h:366-367: `const int yy = y + n * sina` is (int)((float)y + (float)n * sina): one float32 product and one float32
// sum, each rounded on its own (no fused multiply-add: the library is built with contraction off, and the pragma says
// it again where the compiler knows it), then truncation toward zero.
FH_HD int probe(int at, int n, float dir)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float prod = (float)n * dir;
    const float sum = (float)at + prod;
    return (int)sum;
}

FH_HD bool outside(int yy, int xx, int H, int W) { return yy < 0 || yy >= H || xx < 0 || xx >= W; }   // Sad.h:368

// Sad.h:361-378 for the pixel (y, x) on the map in its current state.  The eight rays advance together, n = 1, 2, ...:
// a ray ends when it leaves the image (nothing collected) or at its first pixel != invalid, whose value goes to v[ray]
// and whose bit is set in the result.  The rays do not depend on each other, so walking them side by side collects what
// walking them one after the other collects.  A ray that has ended costs nothing more.  (A form that reads all eight
// pixels of a step at once, ended rays included, was measured slower: profiles/fill_holes_unconditional_reads.txt.)
// A collected -0.0f is stored as +0.0f (see choose).  Every ray has
// |sina| or |cosa| above 0.7, so it leaves an H x W image after fewer than 1.5 * max(H, W) steps.
FH_HD unsigned collect(const float *M, int H, int W, int y, int x, float invalid, float (&v)[RAYS])
{
    unsigned active = (1u << RAYS) - 1, has = 0;
    for (int n = 1; active; n++) {
#pragma unroll
        for (int r = 0; r < RAYS; r++) {
            if (!(active >> r & 1u)) continue;
            const int yy = probe(y, n, sina(r)), xx = probe(x, n, cosa(r));
            if (outside(yy, xx, H, W)) { active &= ~(1u << r); continue; }
            const float d = M[(size_t)yy * W + xx];
            if (d != invalid) {
                v[r] = d + 0.0f;
                has |= 1u << r;
                active &= ~(1u << r);
            }
        }
    }
    return has;
}

// Sad.h:379-397 on the values of `collect` (has != 0): sorted ascending, pass 0 takes element 1 when there are at least
// two values and element 0 otherwise, passes 1 and 2 take element size / 2.  The element of rank k is found by counting:
// value i has rank #{j : v[j] < v[i]} + #{j < i : v[j] == v[i]}.  std::sort leaves the order of -0.0f and +0.0f open;
// collect has made every zero +0.0f, so equal values have equal bits and the result does not depend on that order.
// No value is a NaN (a map with one is not processed).
FH_HD float choose(const float (&v)[RAYS], unsigned has, int pass)
{
    const int c = __builtin_popcount(has);
    const int k = pass == 0 ? (c > 1 ? 1 : 0) : c / 2;
    float out = 0.0f;
#pragma unroll
    for (int i = 0; i < RAYS; i++) {
        if (!(has >> i & 1u)) continue;
        int rank = 0;
#pragma unroll
        for (int j = 0; j < RAYS; j++)
            if ((has >> j & 1u) && (v[j] < v[i] || (j < i && v[j] == v[i]))) rank++;
        if (rank == k) out = v[i];
    }
    return out;
}

// the class of a pass's targets in a map as smt_lrcheck writes it: pass 0 visits the occlusions (1), pass 1 the
// mismatches (2); pass 2 visits the pixels that are == invalid when it starts.  A target of pass 2 stays == invalid until
// its own turn (only targets are written, and a written value is != invalid), so "== invalid at its turn" is the same
// set and needs no list.
FH_HD bool is_target(int pass, uint8_t cls, float value, float invalid)
{
    return pass == 2 ? value == invalid : cls == (uint8_t)(pass + 1);
}

// wavefront step of pixel (i, j) and the number of steps of a pass
FH_HD long long step_of(int i, int j) { return (long long)SKEW * i + j; }
FH_HD long long steps(int H, int W) { return (long long)SKEW * (H - 1) + W; }

}  // namespace fhrule
