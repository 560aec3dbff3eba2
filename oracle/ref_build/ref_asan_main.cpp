// Runs every admitted case of tests/golden/ref_pin_cases.py once through the two reference wrappers
// built with AddressSanitizer (`make -C oracle ref-asan`): a case on which the reference's own code
// reads or writes out of bounds must leave the case list.  Inputs come from
// `make_golden.py ref-pin-dump DIR` (manifest.txt + raw arrays); every buffer here has its exact
// size.  Host code only.  Test infrastructure; no algorithm.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

extern "C" {
int ref_adcensus(float*, float*, int, int, int, float, float, float*, float*, float*, float*);
int ref_arms(unsigned char*, int, int, int, int, const int*, int, int*, int*);
int ref_aggregate(const int*, float*, int, int, int, int, float*, float*);
int ref_scanline(float*, float*, int, int, int, int, int, float*, float*, float*, float*, float*, float*);
int ref_lrcheck(float*, float*, int, int, int, int*, int*, int*, int*);
int ref_lrcheck_variant(float*, float*, float*, int, int, float, int*, int*, int*, int*);
int ref_fill_the_hole(float*, int, int, int, const int*, int, const int*, int, int*, int*);
int ref_remove_speckles(float*, int, int, int, unsigned, int);
int ref_median(const float*, float*, int, int, int);
int ref_cblsm_arm(unsigned char*, int, int, int, int, int, int, int, int*);
int ref_cblsm_ad(unsigned char*, unsigned char*, int, int, int, int, float*);
int ref_cblsm_aggregate_v5(float*, float*, int*, int*, int*, int*, int, int, int);
int ref_cblsm_disp(float*, float*, int, int, int);
int ref_cblsm_choose_lr(int, int*, int*, int*, int*, int, int*, int, int);
int ref_cblsm_choose_ud(int, int*, int*, int*, int*, int*, int*, int, int*, int, int);
}

template <typename T> static std::vector<T> load(const std::string& path, size_t want)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    const size_t bytes = size_t(f.tellg());
    if (bytes != want * sizeof(T)) { std::fprintf(stderr, "%s: %zu bytes, expected %zu\n", path.c_str(), bytes, want * sizeof(T)); std::exit(2); }
    std::vector<T> v(want);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), std::streamsize(bytes));
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    std::ifstream man(dir + "manifest.txt");
    if (!man) { std::fprintf(stderr, "no manifest in %s\n", argv[1]); return 2; }
    std::string line;
    int ran = 0;
    while (std::getline(man, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string kind, name;
        int p[9], nf;
        is >> kind >> name;
        for (int& v : p) is >> v;
        is >> nf;
        std::vector<std::string> f(nf);
        for (auto& s : f) { is >> s; s = dir + s; }
        const size_t n = size_t(p[0]) * p[1], nd = n * p[2];
        typedef std::vector<float> VF;
        typedef std::vector<int> VI;
        typedef std::vector<unsigned char> VB;
        if (kind == "adcensus") {
            VF L = load<float>(f[0], n), R = load<float>(f[1], n), a(nd), b(nd), c(n), d(n);
            ref_adcensus(L.data(), R.data(), p[0], p[1], p[2], 10.0f, 30.0f, a.data(), b.data(), c.data(), d.data());
        } else if (kind == "arms") {
            VB img = load<unsigned char>(f[0], n * p[2]);
            VI maps(4 * n);
            int t;
            ref_arms(img.data(), p[0], p[1], p[2], p[3], &p[5], p[4], maps.data(), &t);
        } else if (kind == "agg") {
            VF vol = load<float>(f[0], nd), out(nd), disp(n);
            VI maps;
            for (int k = 1; k <= 4; k++) { VI m = load<int>(f[k], n); maps.insert(maps.end(), m.begin(), m.end()); }
            if (p[3] == 1)
                ref_cblsm_aggregate_v5(vol.data(), out.data(), &maps[0], &maps[n], &maps[2 * n], &maps[3 * n], p[2], p[0], p[1]),
                ref_cblsm_disp(out.data(), disp.data(), p[2], p[0], p[1]);
            else
                ref_aggregate(maps.data(), vol.data(), p[0], p[1], p[2], p[3], out.data(), disp.data());
        } else if (kind == "scan") {
            VF cost = load<float>(f[0], nd), gray = load<float>(f[1], n), l(nd), r(nd), u(nd), d(nd), s(nd), disp(n);
            ref_scanline(cost.data(), gray.data(), p[0], p[1], p[2], p[3], p[4], l.data(), r.data(), u.data(), d.data(),
                         s.data(), disp.data());
        } else if (kind == "lrcheck" || kind == "lrvariant") {
            VF dL = load<float>(f[0], n), dR = load<float>(f[1], n), last(n);
            VI occ(2 * n), mis(2 * n);
            int no, nm;
            if (kind == "lrcheck") ref_lrcheck(dL.data(), dR.data(), p[0], p[1], p[2], occ.data(), &no, mis.data(), &nm);
            else ref_lrcheck_variant(dL.data(), dR.data(), last.data(), p[0], p[1], float(p[2]), occ.data(), &no, mis.data(), &nm);
        } else if (kind == "fill") {
            VF disp = load<float>(f[0], n);
            VI occ = load<int>(f[1], 2 * size_t(p[3])), mis = load<int>(f[2], 2 * size_t(p[4])), after(2 * (n + p[4]));
            int na;
            ref_fill_the_hole(disp.data(), p[0], p[1], p[2], occ.data(), p[3], mis.data(), p[4], after.data(), &na);
        } else if (kind == "speckle") {
            VF disp = load<float>(f[0], n);
            ref_remove_speckles(disp.data(), p[1], p[0], p[2], unsigned(p[3]), p[4]);
        } else if (kind == "median") {
            VF in = load<float>(f[0], n), out(n);
            ref_median(in.data(), out.data(), p[1], p[0], p[2]);
        } else if (kind == "cblsm_arms") {
            VB img = load<unsigned char>(f[0], n * p[2]);
            for (int dir = 0; dir < 4; dir++) {
                VI arm(n);
                ref_cblsm_arm(img.data(), p[0], p[1], p[2], dir, p[3], 34, 17, arm.data());
            }
        } else if (kind == "cblsm_ad") {
            VB L = load<unsigned char>(f[0], n), R = load<unsigned char>(f[1], n);
            for (int view = 0; view < 2; view++) {
                VF vol(nd);
                ref_cblsm_ad(L.data(), R.data(), p[0], p[1], p[2], view, vol.data());
            }
        } else if (kind == "cblsm_disp") {
            VF vol = load<float>(f[0], nd), disp(n);
            ref_cblsm_disp(vol.data(), disp.data(), p[2], p[0], p[1]);
        } else if (kind == "choose") {
            std::vector<VI> m;
            for (int k = 0; k < 8; k++) m.push_back(load<int>(f[k], n));   // LL LR RL RR LU LD RU RD
            VI vol(nd);
            ref_cblsm_choose_lr(0, m[0].data(), m[0].data(), m[2].data(), m[3].data(), p[2], vol.data(), p[0], p[1]);
            ref_cblsm_choose_lr(1, m[1].data(), m[1].data(), m[2].data(), m[3].data(), p[2], vol.data(), p[0], p[1]);
            ref_cblsm_choose_ud(2, m[4].data(), m[4].data(), m[6].data(), m[6].data(), m[2].data(), m[3].data(), p[2], vol.data(), p[0], p[1]);
            ref_cblsm_choose_ud(3, m[5].data(), m[5].data(), m[7].data(), m[7].data(), m[2].data(), m[3].data(), p[2], vol.data(), p[0], p[1]);
        } else {
            std::fprintf(stderr, "unknown kind %s\n", kind.c_str());
            return 2;
        }
        ran++;
    }
    std::printf("reference sanitizer run clean (%d cases)\n", ran);
    return 0;
}
