// Stand-alone driver of the host-only selftests of csrc/adcensus_selftest.hip, for sanitizer builds of the host code (no
// GPU, no HIP, no Python); tests/test_adcensus_rules_cpu.py builds and runs it:
//   g++ -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -x c++ stereo_match_traditional_amd/csrc/adcensus_selftest.hip tools/adcensus_selftest_main.cpp
//       -o adcensus_selftest && ./adcensus_selftest
// Exit status 0 iff every selftest returned SMT_OK on every shape (and the sanitizers stayed silent).
#include <cstdio>
#include <cstdlib>

extern "C" {
int smt_adcensus_selftest_fused_grid(int ncost, int nprep);
int smt_adcensus_selftest_maps_grid(int nbx, int H, int K, int nprep);
int smt_adcensus_selftest_shared_keys(int H, int W, int D, int K, unsigned seed);
int smt_adcensus_selftest_shared_aux_grid(int ncost, int nprep, int nedge, int nconv);
int smt_adcensus_selftest_shared_aux(int H, int W, int D, int K, int first, int last);
int smt_adcensus_selftest_spans(long nb, int K, int n2, int n1);
int smt_adcensus_selftest_chains(int pairs, int chains, long c0, long c1, long c2, int order, unsigned flags);
}

int main()
{
    static const int shapes[][3] = {{1, 70, 64}, {1, 500, 192}, {3, 70, 64}, {5, 198, 192}, {4, 262, 256}, {7, 133, 64},
                                    {6, 261, 192}, {32, 128, 64}, {16, 128, 62}, {64, 140, 100}, {65, 330, 192},
                                    {6, 259, 192}, {7, 129, 33}, {40, 700, 192}, {128, 96, 20}, {3, 1030, 192},
                                    {3, 69, 64}, {9, 70, 256}, {3, 257, 192}, {3, 258, 192}, {3, 304, 192}, {4, 1030, 192},
                                    {6, 530, 128}, {2, 1536, 192}, {2, 1920, 192}};
    static const int grids[][4] = {{8, 5, 3, 2}, {8, 0, 3, 2}, {8, 5, 0, 2}, {8, 5, 3, 0}, {8, 0, 0, 0}, {8, 40, 30, 20},
                                   {8104, 1110, 256, 507}, {8104, 0, 256, 0}, {1000, 17, 5, 333}};
    static const int Ks[] = {1, 3, 4, 64};
    int bad = 0;
    for (const auto &g : grids) {
        if (smt_adcensus_selftest_shared_aux_grid(g[0], g[1], g[2], g[3]) != 0) { printf("aux_grid %d %d %d %d\n", g[0], g[1], g[2], g[3]); bad++; }
        if (g[1] > 0 && smt_adcensus_selftest_fused_grid(g[0], g[1]) != 0) { printf("fused_grid %d %d\n", g[0], g[1]); bad++; }
    }
    for (const auto &s : shapes)
        for (int K : Ks) {
            const bool served = s[1] - 3 - s[2] >= 3;        // the identity set is not empty
            for (unsigned seed = 0; seed < 8; seed++)
                if (smt_adcensus_selftest_shared_keys(s[0], s[1], s[2], K, seed) != 0) { printf("shared_keys %d %d %d K=%d seed=%u\n", s[0], s[1], s[2], K, seed); bad++; }
            for (int fl = 0; served && fl < 4; fl++)
                if (smt_adcensus_selftest_shared_aux(s[0], s[1], s[2], K, fl & 1, fl >> 1) != 0) { printf("shared_aux %d %d %d K=%d %d\n", s[0], s[1], s[2], K, fl); bad++; }
            if (smt_adcensus_selftest_maps_grid((s[1] + 63) / 64, s[0], K, 5) != 0) { printf("maps_grid %d %d K=%d\n", s[0], s[1], K); bad++; }
        }
    // the span rule of the tapered tail, tails longer than the slice included
    static const long nbs[] = {1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 80, 2000, 2047, 32400};
    static const int spanKs[] = {1, 2, 3, 4, 5, 8, 64};
    static const int tails[][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 2}, {3, 3}, {7, 50}, {1000, 1000}};
    for (long nb : nbs)
        for (int K : spanKs)
            for (const auto &t : tails)
                if (smt_adcensus_selftest_spans(nb, K, t[0], t[1]) != 0) { printf("spans %ld K=%d %d,%d\n", nb, K, t[0], t[1]); bad++; }
    // the shared form's walk and its auxiliary placement under forced tapers (SMT_MAPS_TAPER is read at every call)
    static const char *forced[] = {"0", "0,2", "1,2", "3,1", "7,50"};
    for (const char *f : forced) {
        setenv("SMT_MAPS_TAPER", f, 1);
        for (const auto &s : shapes)
            for (int K : Ks) {
                if (smt_adcensus_selftest_shared_keys(s[0], s[1], s[2], K, 3u) != 0) { printf("shared_keys %d %d %d K=%d taper %s\n", s[0], s[1], s[2], K, f); bad++; }
                if (s[1] - 3 - s[2] >= 3 && smt_adcensus_selftest_shared_aux(s[0], s[1], s[2], K, 0, 0) != 0) { printf("shared_aux %d %d %d K=%d taper %s\n", s[0], s[1], s[2], K, f); bad++; }
            }
    }
    unsetenv("SMT_MAPS_TAPER");
    // the chained schedule's order: every order and flag set, every parity of the chains' counters
    for (int pairs = 1; pairs <= 12; pairs++)
        for (int chains = 1; chains <= 3; chains++)
            for (int order = 0; order < 4; order++)
                for (unsigned flags = 0; flags < 16; flags++)
                    for (int par = 0; par < 8; par++)
                        if (smt_adcensus_selftest_chains(pairs, chains, par & 1, 2 + ((par >> 1) & 1), 5 - (par >> 2), order, flags) != 0) {
                            printf("chains %d %d order %d flags %u parity %d\n", pairs, chains, order, flags, par); bad++;
                        }
    if (smt_adcensus_selftest_chains(0, 2, 0, 0, 0, 0, 0) != -1 || smt_adcensus_selftest_chains(4, 4, 0, 0, 0, 0, 0) != -1 ||
        smt_adcensus_selftest_chains(4, 2, 0, -1, 0, 0, 0) != -1 || smt_adcensus_selftest_chains(4, 2, 0, 0, 0, 4, 0) != -1 ||
        smt_adcensus_selftest_chains(4, 2, 0, 0, 0, 0, 16) != -1) { printf("chains: bad arguments accepted\n"); bad++; }
    printf("%s: %d failures\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
