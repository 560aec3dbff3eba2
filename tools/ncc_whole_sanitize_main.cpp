// smt_whole_ncc_selftest_box under AddressSanitizer and UBSan, on the CPU, as a stand-alone program: the host twin of the
// integer form's recurrences (csrc/ncc_whole.hip) on heap buffers of exactly the images' and tables' size, at shapes with
// every clamp, the fill columns, max_offset == W and the two sides of a tile edge, so that an index rule of
// csrc/ncc_whole_rules.h that leaves an image row or a prefix table would be reported.  Build and run (host code
// sanitized, no GPU used; the build takes about a minute, so no test runs it):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=all -x hip stereo_match_traditional_amd/csrc/ncc_whole.hip
//         -x hip tools/ncc_whole_sanitize_main.cpp -o ncc_whole_sanitize && ./ncc_whole_sanitize
// The device entry points of ncc_whole.hip are linked but never called; what they need from the rest of the library is
// stubbed below.
#include <cstdio>
#include <cstdlib>
#include "../stereo_match_traditional_amd/csrc/smt_common.h"

thread_local int g_smt_last_hip = 0;
hipError_t smt_scratch_alloc(void **, size_t, hipStream_t) { abort(); }
void smt_scratch_free(void *, hipStream_t) { abort(); }
extern "C" int smt_sad_crosscheck(const int32_t *, const int32_t *, int, int, int32_t *, uint8_t *, void *) { abort(); }

int main()
{
    // H, W, kernel_size, max_offset
    static const int shapes[][4] = {{2, 2, 1, 1}, {2, 9, 5, 4}, {7, 9, 5, 9}, {5, 33, 1, 12}, {4, 20, 3, 20}, {3, 90, 2, 86},
                                    {2, 246, 5, 3}, {2, 247, 5, 3}, {19, 21, 5, 10}, {9, 83, 5, 79}, {3, 80, 35, 3}, {12, 300, 7, 9}};
    int bad = 0;
    for (const auto &s : shapes)
        for (int view = SMT_VIEW_LEFT; view <= SMT_VIEW_RIGHT; view++) {
            const int rc = smt_whole_ncc_selftest_box(s[0], s[1], s[2], s[3], view, 11u + (unsigned)s[1]);
            if (rc != SMT_OK) { printf("%dx%d k=%d O=%d view %d: status %d\n", s[0], s[1], s[2], s[3], view, rc); bad++; }
        }
    printf(bad ? "FAILED\n" : "ok: %zu shapes, both views\n", sizeof(shapes) / sizeof(shapes[0]));
    return bad ? 1 : 0;
}
