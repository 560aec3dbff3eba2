// smt_fill_image_new_host under AddressSanitizer and UBSan, on the CPU, as a stand-alone program: the crafted maps of
// tests/asw_tail_cases.py on heap buffers of exactly the maps' size, so that a read of the byte behind a map -- the
// reference's own read at (H - 1, W) -- or an index past the list's end would be reported.  Build and run (host code
// sanitized, no GPU used; the build takes about a minute, so no test runs it):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=all -x hip stereo_match_traditional_amd/csrc/asw_tail.hip
//         -x hip tools/fill_image_new_sanitize_main.cpp -o fill_image_new_sanitize && ./fill_image_new_sanitize
// The device entry points of asw_tail.hip are linked but never called; what they need from the rest of the library is
// stubbed below.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../stereo_match_traditional_amd/csrc/smt_common.h"

thread_local int g_smt_last_hip = 0;
hipError_t smt_scratch_alloc(void **, size_t, hipStream_t) { abort(); }
void smt_scratch_free(void *, hipStream_t) { abort(); }
size_t smt_speckle_scratch_bytes(int, int, int) { abort(); }
int smt_speckle_u8_enqueue(uint8_t *, int, size_t, int, int, int, int, int, void *, int *, hipStream_t) { abort(); }

struct Map { int H, W; std::vector<uint8_t> px; };

static Map zeros(int H, int W) { return Map{H, W, std::vector<uint8_t>((size_t)H * W, 0)}; }

static std::vector<Map> crafted()
{
    std::vector<Map> v;
    Map a = zeros(4, 7);                                   // all-zero rows above a row starting with 0
    for (int c = 1; c < 7; c++) a.px[3 * 7 + c] = 5;
    v.push_back(a);
    Map b = zeros(4, 7);                                   // ... and above a row starting with 9
    b.px[2 * 7] = 9; b.px[3 * 7 + 3] = 4;
    v.push_back(b);
    Map c = zeros(5, 11);                                  // a missing push in row 0 shifts the rest
    c.px[11] = 9; c.px[2 * 11 + 4] = 3; c.px[4 * 11 + 10] = 8;
    v.push_back(c);
    v.push_back(zeros(6, 9));
    v.push_back(zeros(1, 7));                              // H = 1: the row-end read is the undefined one
    v.push_back(zeros(1, 1));
    v.push_back(zeros(7, 1));
    Map full = zeros(9, 13);
    for (auto &p : full.px) p = 200;
    v.push_back(full);
    Map w = zeros(3, 137);                                 // walks of 16 probes
    w.px[136] = 200; w.px[137] = 17; w.px[2 * 137 + 70] = 1;
    v.push_back(w);
    Map r = zeros(33, 65);                                 // pseudo-random, 70 % holes
    unsigned s = 12345u;
    for (auto &p : r.px) { s = s * 1664525u + 1013904223u; p = (s >> 24) % 10 < 7 ? 0 : (uint8_t)(1 + (s >> 16) % 255); }
    v.push_back(r);
    return v;
}

int main()
{
    unsigned long long sum = 0;
    int runs = 0;
    for (const Map &m : crafted())
        for (unsigned fix = 0; fix <= SMT_ASW_FIX_FILL_ROW_END; fix++)
            for (int pairs = 1; pairs <= 3; pairs += 2)
                for (int gap = 0; gap <= 5; gap += 5) {
                    const size_t n = (size_t)m.H * m.W, stride = n + gap;
                    // exactly the bytes the call may touch: the last map has no gap behind it
                    const size_t bytes = (size_t)(pairs - 1) * stride + n;
                    uint8_t *buf = (uint8_t *)malloc(bytes);
                    int *counts = (int *)malloc(sizeof(int) * 2 * pairs);
                    if (!buf || !counts) return 2;
                    memset(buf, 0xA5, bytes);
                    for (int b = 0; b < pairs; b++) memcpy(buf + b * stride, m.px.data(), n);
                    const int rc = smt_fill_image_new_host(buf, pairs, gap ? stride : 0, m.H, m.W, fix, gap ? counts : nullptr);
                    if (rc != SMT_OK) { fprintf(stderr, "status %d at %dx%d\n", rc, m.H, m.W); return 1; }
                    for (int b = 0; b < pairs; b++) {
                        if (memcmp(buf + b * stride, buf, n)) { fprintf(stderr, "maps of one batch differ\n"); return 1; }
                        if (gap && fix && (counts[2 * b] || counts[2 * b + 1])) { fprintf(stderr, "fixed mode counted\n"); return 1; }
                        if (gap && b + 1 < pairs)
                            for (int g = 0; g < gap; g++)
                                if (buf[b * stride + n + g] != 0xA5) { fprintf(stderr, "gap written\n"); return 1; }
                    }
                    for (size_t i = 0; i < n; i++) sum = sum * 1099511628211ull + buf[i];
                    free(buf); free(counts);
                    runs++;
                }
    printf("clean: %d runs, checksum %016llx\n", runs, sum);
    return 0;
}
