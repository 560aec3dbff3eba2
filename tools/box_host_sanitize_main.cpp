// smt_sad_selftest_box and smt_ncc_selftest_box under AddressSanitizer and UBSan, on the CPU, as a stand-alone program:
// box_host<Tap> (csrc/box_stage.h), the host restatement of the staged-row box-sum engine, on heap buffers of exactly the
// images' size, at shapes with a 3-wide window (the tail dword that starts before the window), every side & 3, strips
// that end inside and at a workgroup's 64 columns, D on both sides of a slot count and bands of 1, 3 and the launch's
// choice, so that an entry index that leaves a staged row would be reported.  Build and run (host code sanitized, no GPU
// used; the build takes about two minutes, so no test runs it):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=all -x hip stereo_match_traditional_amd/csrc/sad_both.hip
//         -x hip stereo_match_traditional_amd/csrc/ncc_box.hip -x hip tools/box_host_sanitize_main.cpp
//         -o box_host_sanitize && ./box_host_sanitize
// The device entry points of the two files are linked but never called; what they need from the rest of the library is
// stubbed below.
#include <cstdio>
#include <cstdlib>
#include "../stereo_match_traditional_amd/csrc/smt_common.h"

thread_local int g_smt_last_hip = 0;
int g_smt_ncc_last_form = 0;
hipError_t smt_scratch_alloc(void **, size_t, hipStream_t) { abort(); }
void smt_scratch_free(void *, hipStream_t) { abort(); }
int smt_ncc_loop_enqueue(const uint8_t *, const uint8_t *, int, int, int, int, int, int32_t *, double *, hipStream_t) { abort(); }
int smt_ncc_dot4_enqueue(const uint8_t *, const uint8_t *, int, int, int, int, int, const int *, const double *, const int *,
                         const double *, int32_t *, double *, hipStream_t, unsigned long long *)
{
    abort();
}
int smt_lrncc_enqueue(int, const uint8_t *, const uint8_t *, int, int, int, int, int, int *, double *, int *, double *, int32_t *,
                      int32_t *, double *, double *, hipStream_t)
{
    abort();
}
extern "C" int smt_malloc(void **, size_t) { abort(); }
extern "C" int smt_sad(const uint8_t *, const uint8_t *, int, int, int, int, int, int32_t *, void *) { abort(); }
extern "C" int smt_sad_crosscheck(const int32_t *, const int32_t *, int, int, int32_t *, uint8_t *, void *) { abort(); }
extern "C" int smt_pad_replicate(const uint8_t *, int, int, int, uint8_t *, void *) { abort(); }

int main()
{
    // H, W, D, window parameter (SAD: winsize, side 2 winsize + 3; NCC: winSize, side 2 winSize + 1)
    static const int shapes[][4] = {{3, 5, 4, 0},   {4, 64, 64, 0},  {4, 65, 65, 1},  {5, 70, 130, 2}, {6, 33, 20, 3},
                                    {9, 17, 9, 4},  {2, 130, 3, 5},  {7, 63, 260, 1}, {12, 40, 64, 6}, {3, 129, 128, 0}};
    int bad = 0;
    for (const auto &s : shapes) {
        int rc = smt_sad_selftest_box(s[0], s[1], s[2], s[3], 7u + (unsigned)s[1]);
        if (rc != SMT_OK) { printf("sad %dx%d D=%d winsize %d: status %d\n", s[0], s[1], s[2], s[3], rc); bad++; }
        const int H = s[0] + 2 * s[3] + 2, W = s[1] + 2 * s[3] + 2;           // an interior of the SAD shape's size
        rc = smt_ncc_selftest_box(H, W, s[2], s[3] + 1, 7u + (unsigned)s[1]);
        if (rc != SMT_OK) { printf("ncc %dx%d D=%d winSize %d: status %d\n", H, W, s[2], s[3] + 1, rc); bad++; }
    }
    printf(bad ? "FAILED\n" : "ok: %zu shapes, SAD and NCC\n", sizeof(shapes) / sizeof(shapes[0]));
    return bad ? 1 : 0;
}
