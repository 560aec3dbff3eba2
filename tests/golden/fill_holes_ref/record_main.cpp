// Driver of tests/golden/make_fill_holes_golden.py: runs the reference's FillHolesInDispMap (SAD/Sad.h, included
// unmodified from the reference tree given with -I) on the maps of an input file and writes the map after every pass.
// Test infrastructure; this file is our own text and is never part of the library.
//
// in:  int32 count; per map: int32 H, W, n_occ, n_mis; float32 invalid; float32 M[H*W]; int32 occ[n_occ][2], mis[n_mis][2]
// out: per map float32 pass0[H*W], pass1[H*W], pass2[H*W]
// The function has no pass-by-pass output.  The map after pass 1 is what the map holds when the third pass's scan -- H*W
// reads in raster order, the only such sequence for H >= 2 -- has completed; the map after pass 0 is the same moment of
// a call with an empty mismatch list.
#include <algorithm>
#include <cassert>   // Sad.h uses assert without including it
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>
#include "Sad.h"

static int g_H, g_W, g_next;
static const cv::Mat* g_map;
static std::vector<float> g_snap;
static bool g_have;

static void on_access(int i, int j)
{
    const int at = i * g_W + j;
    g_next = at == g_next ? g_next + 1 : (at == 0 ? 1 : 0);
    if (g_next == g_H * g_W) {
        std::memcpy(g_snap.data(), g_map->data(), g_snap.size() * sizeof(float));
        g_have = true;
        g_next = 0;
    }
}

template <typename T> static T rd(FILE* f)
{
    T v;
    if (std::fread(&v, sizeof(T), 1, f) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}

static std::vector<float> run(const std::vector<float>& M, int H, int W, const std::vector<std::pair<int, int>>& occ,
                              const std::vector<std::pair<int, int>>& mis, float invalid, std::vector<float>& at_scan)
{
    cv::Mat m(H, W, sizeof(float));
    std::memcpy(m.data(), M.data(), M.size() * sizeof(float));
    g_H = H; g_W = W; g_next = 0; g_map = &m; g_have = false;
    g_snap.assign(M.size(), 0.0f);
    cv::shim_on_access = on_access;
    FillHolesInDispMap(W, H, m, occ, mis, invalid);
    cv::shim_on_access = nullptr;
    if (!g_have) { std::fprintf(stderr, "the third pass's scan was not seen\n"); std::exit(3); }
    at_scan = g_snap;
    return std::vector<float>(reinterpret_cast<float*>(m.data()), reinterpret_cast<float*>(m.data()) + M.size());
}

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 1;
    const int count = rd<int32_t>(in);
    for (int k = 0; k < count; k++) {
        const int H = rd<int32_t>(in), W = rd<int32_t>(in), no = rd<int32_t>(in), nm = rd<int32_t>(in);
        const float invalid = rd<float>(in);
        if (H < 2) { std::fprintf(stderr, "H >= 2 needed\n"); return 2; }
        std::vector<float> M((size_t)H * W);
        for (float& v : M) v = rd<float>(in);
        std::vector<std::pair<int, int>> occ(no), mis(nm);
        for (auto& p : occ) { p.first = rd<int32_t>(in); p.second = rd<int32_t>(in); }
        for (auto& p : mis) { p.first = rd<int32_t>(in); p.second = rd<int32_t>(in); }
        std::vector<float> pass0, pass1, unused;
        run(M, H, W, occ, {}, invalid, pass0);
        const std::vector<float> pass2 = run(M, H, W, occ, mis, invalid, pass1);
        std::fwrite(pass0.data(), sizeof(float), pass0.size(), out);
        std::fwrite(pass1.data(), sizeof(float), pass1.size(), out);
        std::fwrite(pass2.data(), sizeof(float), pass2.size(), out);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 1;
}
