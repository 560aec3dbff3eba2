// mirror_main <case> <dir> <ints...> -- one entry of the C++ host mirror (smt_host.hpp) on raw files, for
// tests/test_cpp_mirror_gpu.py.  Reads <dir>/in_<name>.bin, calls the mirror with host buffers, writes <dir>/out_<name>.bin
// for every buffer (inputs too: they must come back unchanged) and <dir>/status.txt (list lengths, exceptions caught).
//
// Host guard bands: the buffers of a case are carved from one allocation with a band on both sides of each at least as
// large as the largest of them, filled with 0xA5; a changed band ends the program with exit code 3 and the buffer's name.
// Every case runs twice, with its outputs prefilled by the two patterns of tests/arena.py (every byte below 0x80; every
// aligned word a NaN): outputs or status that differ between the two runs end the program with exit code 4, so an
// element the mirror leaves unwritten shows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>

#include "smt_host.hpp"

namespace {

std::string g_dir;

std::vector<unsigned char> read_file(const std::string &name, bool *found = nullptr)
{
    std::vector<unsigned char> v;
    FILE *f = fopen((g_dir + "/in_" + name + ".bin").c_str(), "rb");
    if (found) *found = f != nullptr;
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read of %s\n", name.c_str()); exit(2); }
    fclose(f);
    return v;
}
void write_file(const std::string &name, const void *p, size_t bytes)
{
    FILE *f = fopen((g_dir + "/out_" + name + ".bin").c_str(), "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { fprintf(stderr, "cannot write %s\n", name.c_str()); exit(2); }
    fclose(f);
}

unsigned char prefill_byte(size_t k, int which)        // tests/arena.py pattern(), seeds 0x2A and 0xD5
{
    const unsigned h = (unsigned)((k * 167 + (which ? 0xD5 : 0x2A)) & 0xFF);
    if (!which) return (unsigned char)(h & 0x7F);
    if (k % 4 == 3) return 0xFF;
    if (k % 8 == 6) return (unsigned char)(0xF0 | (h & 0x0F));
    return (unsigned char)(0x80 | (h & 0x3F));
}

class Arena {
public:
    explicit Arena(int which) : which_(which) {}
    ~Arena() { free(base_); }
    Arena(const Arena &) = delete;
    // declare: inputs come from in_<name>.bin (exactly `bytes` long), everything else is prefilled
    void add(const std::string &name, size_t bytes) { order_.push_back(name); bytes_[name] = bytes; }
    void build()
    {
        band_ = 256;
        for (auto &kv : bytes_) if (kv.second > band_) band_ = kv.second;
        band_ = (band_ + 63) / 64 * 64;
        size_t total = band_;
        for (const std::string &n : order_) { off_[n] = total; total += (bytes_[n] + 63) / 64 * 64 + band_; }
        base_ = static_cast<unsigned char *>(malloc(total));
        total_ = total;
        memset(base_, 0xA5, total);
        for (const std::string &n : order_) {
            bool found = false;
            const std::vector<unsigned char> v = read_file(n, &found);
            if (found && v.size() != bytes_[n]) { fprintf(stderr, "in_%s.bin has %zu bytes, the case wants %zu\n", n.c_str(), v.size(), bytes_[n]); exit(2); }
            for (size_t k = 0; k < bytes_[n]; k++) base_[off_[n] + k] = found ? v[k] : prefill_byte(k, which_);
        }
    }
    template <class T> T *p(const std::string &name) { return reinterpret_cast<T *>(base_ + off_.at(name)); }
    // the name of the first buffer with a changed band beside it, or ""
    std::string bands() const
    {
        std::vector<bool> data(total_, false);
        for (const std::string &n : order_) for (size_t k = 0; k < bytes_.at(n); k++) data[off_.at(n) + k] = true;
        for (size_t k = 0; k < total_; k++)
            if (!data[k] && base_[k] != 0xA5) {
                std::string near = order_.front();
                for (const std::string &n : order_) if (off_.at(n) <= k + band_) near = n;
                return near;
            }
        return "";
    }
    std::map<std::string, std::vector<unsigned char>> contents() const
    {
        std::map<std::string, std::vector<unsigned char>> m;
        for (const std::string &n : order_) m[n].assign(base_ + off_.at(n), base_ + off_.at(n) + bytes_.at(n));
        return m;
    }
private:
    int which_;
    std::vector<std::string> order_;
    std::map<std::string, size_t> bytes_, off_;
    unsigned char *base_ = nullptr;
    size_t band_ = 0, total_ = 0;
};

struct Run {
    Arena A;
    std::string status;
    std::map<std::string, std::vector<unsigned char>> extra;       // lists and buffers the mirror owns
    explicit Run(int which) : A(which) {}
    void note(const std::string &k, long long v) { status += k + " " + std::to_string(v) + "\n"; }
    void guarded(const char *what, const std::function<void()> &f)
    {
        try { f(); status += std::string(what) + " ok\n"; }
        catch (const std::runtime_error &e) { status += std::string(what) + " threw " + e.what() + "\n"; }
    }
    template <class T> void keep(const std::string &name, const T *p, size_t n)
    {
        const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
        extra[name].assign(b, b + n * sizeof(T));
    }
};

using List = std::vector<std::pair<int, int>>;
List read_list(const std::string &name)
{
    const std::vector<unsigned char> v = read_file(name);
    List l(v.size() / 8);
    for (size_t k = 0; k < l.size(); k++) { int a[2]; memcpy(a, v.data() + 8 * k, 8); l[k] = {a[0], a[1]}; }
    return l;
}
void keep_list(Run &r, const std::string &name, const List &l)
{
    std::vector<int> flat;
    for (auto &p : l) { flat.push_back(p.first); flat.push_back(p.second); }
    r.keep(name, flat.data(), flat.size());
    r.note("len_" + name, (long long)l.size());
}

typedef void (*CaseFn)(Run &, const std::vector<int> &);

// lar H W gate_milli: LeftAndRightConsistency on pre-populated lists
void c_lar(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1);
    const size_t n = (size_t)H * W;
    r.A.add("dispL", n * 4); r.A.add("dispR", n * 4); r.A.add("last", n * 4);
    r.A.build();
    List occ = read_list("occ"), mis = read_list("mis");
    r.guarded("LeftAndRightConsistency", [&] {
        smt::LeftAndRightConsistency(r.A.p<float>("dispL"), r.A.p<float>("dispR"), r.A.p<float>("last"), W, H, a.at(2) / 1000.0f, occ, mis);
    });
    keep_list(r, "occ", occ); keep_list(r, "mis", mis);
}
// fill_image H W fix
void c_fill_image(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1);
    r.A.add("map", (size_t)H * W); r.A.add("counts", 8); r.A.add("map_nocounts", (size_t)H * W);
    r.A.build();
    r.guarded("FillImageNew", [&] { smt::FillImageNew(r.A.p<unsigned char>("map"), H, W, (unsigned)a.at(2), r.A.p<int>("counts")); });
    r.guarded("FillImageNew", [&] { smt::FillImageNew(r.A.p<unsigned char>("map_nocounts"), H, W, (unsigned)a.at(2)); });
}
// median H W wnd: MedianFilterInPlace, and MedianFilter(d, d) on a second copy
void c_median(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1);
    r.A.add("map", (size_t)H * W * 4); r.A.add("aliased", (size_t)H * W * 4);
    r.A.build();
    r.guarded("MedianFilterInPlace", [&] { smt::MedianFilterInPlace(r.A.p<float>("map"), W, H, a.at(2)); });
    r.guarded("MedianFilter", [&] { smt::MedianFilter(r.A.p<float>("aliased"), r.A.p<float>("aliased"), W, H, a.at(2)); });
}
// grey H W
void c_grey(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1);
    r.A.add("bgr", (size_t)H * W * 3); r.A.add("grey", (size_t)H * W);
    r.A.build();
    r.guarded("bgr_to_grey", [&] { smt::bgr_to_grey(r.A.p<unsigned char>("bgr"), H, W, r.A.p<unsigned char>("grey")); });
}
// choose H W D: the four chooseArmLength* from the eight arm maps (L: LL LR LUp LDown, R: RL RR RUp RDown)
void c_choose(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t n = (size_t)H * W * 4;
    for (const char *m : {"LL", "LR", "LUp", "LDown", "RL", "RR", "RUp", "RDown"}) r.A.add(m, n);
    for (const char *m : {"volL", "volR", "volUp", "volDown"}) r.A.add(m, n * D);
    r.A.build();
    auto P = [&](const char *m) { return r.A.p<int>(m); };
    r.guarded("chooseArmLengthLeft", [&] { smt::chooseArmLengthLeft(P("LL"), P("LR"), P("RL"), P("RR"), D, P("volL"), H, W); });
    r.guarded("chooseArmLengthRight", [&] { smt::chooseArmLengthRight(P("LL"), P("LR"), P("RL"), P("RR"), D, P("volR"), H, W); });
    r.guarded("chooseArmLengthUp", [&] { smt::chooseArmLengthUp(P("LUp"), P("LDown"), P("RUp"), P("RDown"), P("RL"), P("RR"), D, P("volUp"), H, W); });
    r.guarded("chooseArmLengthDown", [&] { smt::chooseArmLengthDown(P("LUp"), P("LDown"), P("RUp"), P("RDown"), P("RL"), P("RR"), D, P("volDown"), H, W); });
}
// v4 H W D
void c_v4(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t V = (size_t)H * W * D * 4;
    for (const char *m : {"vol", "aL", "aR", "aUp", "aDown", "out"}) r.A.add(m, V);
    r.A.build();
    r.guarded("costAggregationV4", [&] {
        smt::costAggregationV4(r.A.p<float>("vol"), r.A.p<float>("out"), r.A.p<int>("aL"), r.A.p<int>("aR"), r.A.p<int>("aUp"), r.A.p<int>("aDown"), D, H, W, 0);
    });
}
// dispv4 H W D ws: ComputeDispV4 on padded 3-channel images
void c_dispv4(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2), ws = a.at(3), w = ws + 1;
    smt::Image L, R;
    L.rows = R.rows = H + 2 * w; L.cols = R.cols = W + 2 * w; L.channels = R.channels = 3;
    L.data = read_file("Lp"); R.data = read_file("Rp");
    r.A.add("vol", (size_t)H * W * D * 4);
    r.A.build();
    r.guarded("ComputeDispV4", [&] { smt::ComputeDispV4(r.A.p<float>("vol"), L, R, ws, D, H, W); });
    r.keep("Lp", L.data.data(), L.data.size()); r.keep("Rp", R.data.data(), R.data.size());
}
// sad H W D ws (inner sizes): GetPointDepthLeft, Right and Both
void c_sad(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2), ws = a.at(3), w = ws + 1, rows = H + 2 * w, cols = W + 2 * w;
    r.A.add("Lp", (size_t)rows * cols); r.A.add("Rp", (size_t)rows * cols);
    for (const char *m : {"left", "right", "bothL", "bothR"}) r.A.add(m, (size_t)H * W * 4);
    r.A.build();
    auto I = [&](const char *m) { return r.A.p<unsigned char>(m); };
    r.guarded("GetPointDepthLeft", [&] { smt::GetPointDepthLeft(r.A.p<int>("left"), I("Lp"), I("Rp"), rows, cols, D, ws); });
    r.guarded("GetPointDepthRight", [&] { smt::GetPointDepthRight(r.A.p<int>("right"), I("Lp"), I("Rp"), rows, cols, D, ws); });
    r.guarded("GetPointDepthBoth", [&] { smt::GetPointDepthBoth(r.A.p<int>("bothL"), r.A.p<int>("bothR"), I("Lp"), I("Rp"), rows, cols, D, ws); });
}
// asw H W D ws T: the single-view AdaptiveSupportWeight under both values of left_view
void c_asw(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2), ws = a.at(3), w = ws + 1, rows = H + 2 * w, cols = W + 2 * w;
    r.A.add("Lp", (size_t)rows * cols); r.A.add("Rp", (size_t)rows * cols);
    r.A.add("left", (size_t)H * W * 4); r.A.add("right", (size_t)H * W * 4);
    r.A.build();
    std::vector<double> sp, cm;
    smt::getMasks(sp, cm, ws, 50.0, 30.0);
    auto I = [&](const char *m) { return r.A.p<unsigned char>(m); };
    r.guarded("AdaptiveSupportWeight", [&] { smt::AdaptiveSupportWeight(r.A.p<float>("left"), I("Lp"), I("Rp"), rows, cols, ws, D, sp, cm, a.at(4)); });
    r.guarded("AdaptiveSupportWeight", [&] { smt::AdaptiveSupportWeight(r.A.p<float>("right"), I("Lp"), I("Rp"), rows, cols, ws, D, sp, cm, a.at(4), false); });
}
// crossagg W H D iters: SetParams before Initialize, as CBLSM.cpp:138-143 may order them
void c_crossagg(Run &r, const std::vector<int> &a)
{
    const int W = a.at(0), H = a.at(1), D = a.at(2);
    const size_t n = (size_t)W * H;
    r.A.add("img", n * 3); r.A.add("cost", n * D * 4);
    r.A.build();
    r.guarded("CrossAggregator", [&] {
        smt::CrossAggregator c;
        c.SetParams(34, 17, 20, 6);
        r.note("initialize", c.Initialize(W, H, 0, D));
        r.note("cost_before_aggregate", c.get_cost_ptr() != nullptr);
        c.SetData(r.A.p<uint8_t>("img"), nullptr, r.A.p<float>("cost"));
        c.Aggregate(a.at(3));
        r.keep("agg", c.get_cost_ptr(), n * D);
        r.keep("arms", reinterpret_cast<uint8_t *>(c.get_arms_ptr()), n * 4);
    });
}
// subpixel H W D min_den_bits
void c_subpixel(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    float md;
    memcpy(&md, &a.at(3), 4);
    r.A.add("vol", (size_t)H * W * D * 4); r.A.add("disp", (size_t)H * W * 4); r.A.add("disp_default", (size_t)H * W * 4);
    r.A.build();
    r.guarded("WTASubpixel", [&] { smt::WTASubpixel(r.A.p<float>("vol"), r.A.p<float>("disp"), D, H, W, md); });
    r.guarded("WTASubpixel", [&] { smt::WTASubpixel(r.A.p<float>("vol"), r.A.p<float>("disp_default"), D, H, W); });
}
// pipeline H W D quirks: one handle, batches of 2, 1 and 3 pairs; integer maps, sub-pixel maps, integer maps again
void c_pipeline(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t n = (size_t)H * W;
    r.A.add("L", 3 * n); r.A.add("R", 3 * n);
    for (const char *s : {"int", "sub", "again"})
        for (int pairs : {2, 1, 3}) {
            const std::string t = std::string(s) + std::to_string(pairs);
            r.A.add("dl_" + t, pairs * n * 4); r.A.add("dr_" + t, pairs * n * 4); r.A.add("cls_" + t, pairs * n);
        }
    r.A.build();
    r.guarded("Pipeline", [&] {
        smt::Pipeline p(H, W, D);
        p.setQuirks((unsigned)a.at(3));
        for (const char *s : {"int", "sub", "again"}) {
            p.setSubpixel(!strcmp(s, "sub") ? 1.0f : 0.0f);
            for (int pairs : {2, 1, 3}) {
                const std::string t = std::string(s) + std::to_string(pairs);
                p.RunBatch(r.A.p<unsigned char>("L"), r.A.p<unsigned char>("R"), pairs, r.A.p<float>("dl_" + t), r.A.p<float>("dr_" + t),
                           r.A.p<unsigned char>("cls_" + t));
            }
        }
    });
}
// crossarm H W D sub_milli: Aggregation, AggregationVertical, setSubpixel and WTA of CrossArmAggregation
void c_crossarm(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t n = (size_t)H * W, V = n * D * 4;
    r.A.add("img", n); r.A.add("vol", V); r.A.add("vertical", V); r.A.add("exclusive", V);
    r.A.add("wta", n * 4); r.A.add("wta_sub", n * 4); r.A.add("wta_again", n * 4);
    r.A.build();
    r.guarded("CrossArmAggregation", [&] {
        smt::CrossArmAggregation c;
        c.Initialize(H, W, nullptr, nullptr, 30, D);
        c.ComputeArmLengths(r.A.p<unsigned char>("img"), 1);
        c.AggregationVertical(r.A.p<float>("vol"), r.A.p<float>("vertical"));
        c.WTA(r.A.p<float>("vertical"), r.A.p<float>("wta"));
        c.setSubpixel(a.at(3) / 1000.0f);
        c.WTA(r.A.p<float>("vertical"), r.A.p<float>("wta_sub"));
        c.setSubpixel(0.0f);
        c.WTA(r.A.p<float>("vertical"), r.A.p<float>("wta_again"));
    });
    // exclusive bounds: an empty rectangle is the reference's 0 / 0, reported as SMT_ERR_REF_UB after the volume is written
    r.guarded("Aggregation", [&] {
        smt::CrossArmAggregation c;
        c.Initialize(H, W, nullptr, nullptr, 30, D);
        c.ComputeArmLengths(r.A.p<unsigned char>("img"), 1);
        c.Aggregation(r.A.p<float>("vol"), r.A.p<float>("exclusive"));
    });
}
// scanline H W D sub_milli: ScanLine, then WTA with the sub-pixel switch off, on and off again
void c_scanline(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t n = (size_t)H * W;
    r.A.add("vol", n * D * 4); r.A.add("gray", n * 4); r.A.add("wta", n * 4); r.A.add("wta_sub", n * 4); r.A.add("wta_again", n * 4);
    r.A.build();
    r.guarded("ScanlineOptimizer", [&] {
        smt::ScanlineOptimizer s;
        s.Initialize(H, W, D, nullptr, 10, 150);
        s.ScanLine(r.A.p<float>("vol"), r.A.p<float>("gray"));
        s.WTA(r.A.p<float>("wta"));
        s.setSubpixel(a.at(3) / 1000.0f);
        s.WTA(r.A.p<float>("wta_sub"));
        s.setSubpixel(0.0f);
        s.WTA(r.A.p<float>("wta_again"));
    });
}
// adcensus H W D: both views' host volumes, then the same object initialised with the second pair
void c_adcensus(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2);
    const size_t n = (size_t)H * W;
    for (const char *m : {"L0", "R0", "L1", "R1"}) r.A.add(m, n * 4);
    r.A.build();
    r.guarded("AD_Census", [&] {
        smt::AD_Census c;
        for (int k = 0; k < 2; k++) {
            const std::string t = std::to_string(k);
            c.Initialize(r.A.p<float>("L" + t), r.A.p<float>("R" + t), D, H, W, 10.0f, 30.0f);
            c.ComputeADcensus();
            c.ComputeADcensusRight();
            r.keep("right" + t, c.GetPtrRight(), n * D);
            r.keep("left" + t, c.GetPtrLeft(), n * D);
        }
    });
}

// ncc_form H W D win form pairs: NCCFlow::set_form, run and runBoth; which cost kernel ran
void c_ncc_form(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2), pairs = a.at(5);
    const size_t n = (size_t)H * W * pairs;
    r.A.add("L", n); r.A.add("R", n); r.A.add("disp", n * 4);
    r.A.add("bothL", n * 4); r.A.add("bothR", n * 4); r.A.add("last", n * 4); r.A.add("cls", n);
    r.A.build();
    r.guarded("NCCFlow", [&] {
        smt::NCCFlow f(H, W, D, a.at(3));
        f.set_form(a.at(4));
        f.run(r.A.p<unsigned char>("L"), r.A.p<unsigned char>("R"), pairs, r.A.p<int>("disp"));
        r.note("form", smt_ncc_last_form());
        f.runBoth(r.A.p<unsigned char>("L"), r.A.p<unsigned char>("R"), pairs, r.A.p<int>("bothL"), r.A.p<int>("bothR"), r.A.p<int>("last"),
                  r.A.p<unsigned char>("cls"));
    });
}
// whole_form H W k O form pairs: NCCWholeFlow::set_form and run
void c_whole_form(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), pairs = a.at(5);
    const size_t n = (size_t)H * W * pairs;
    r.A.add("L", n); r.A.add("R", n); r.A.add("depthL", n); r.A.add("depthR", n);
    r.A.add("offL", n * 4); r.A.add("offR", n * 4); r.A.add("lastdisp", n * 4);
    r.A.build();
    r.guarded("NCCWholeFlow", [&] {
        smt::NCCWholeFlow f(H, W, a.at(2), a.at(3));
        f.set_form(a.at(4));
        f.run(r.A.p<unsigned char>("L"), r.A.p<unsigned char>("R"), pairs, r.A.p<unsigned char>("depthL"), r.A.p<unsigned char>("depthR"),
              r.A.p<int>("offL"), r.A.p<int>("offR"), r.A.p<int>("lastdisp"));
        r.note("form", smt_whole_ncc_last_form());
    });
}
// window_flow H W D ws pairs: CBLSMFlow::runWindow
void c_window_flow(Run &r, const std::vector<int> &a)
{
    const int H = a.at(0), W = a.at(1), D = a.at(2), pairs = a.at(4);
    const size_t n = (size_t)H * W * pairs;
    r.A.add("L", n); r.A.add("R", n); r.A.add("dispL", n * 4); r.A.add("dispR", n * 4);
    r.A.build();
    r.guarded("CBLSMFlow", [&] {
        smt::CBLSMFlow f(H, W, D);
        f.runWindow(r.A.p<unsigned char>("L"), r.A.p<unsigned char>("R"), pairs, a.at(3), r.A.p<float>("dispL"), r.A.p<float>("dispR"));
    });
}

const std::map<std::string, CaseFn> CASES = {
    {"ncc_form", c_ncc_form}, {"whole_form", c_whole_form}, {"window_flow", c_window_flow},
    {"lar", c_lar}, {"fill_image", c_fill_image}, {"median", c_median}, {"grey", c_grey}, {"choose", c_choose}, {"v4", c_v4},
    {"dispv4", c_dispv4}, {"sad", c_sad}, {"asw", c_asw}, {"crossagg", c_crossagg}, {"subpixel", c_subpixel}, {"pipeline", c_pipeline},
    {"crossarm", c_crossarm}, {"scanline", c_scanline}, {"adcensus", c_adcensus},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3 || !CASES.count(argv[1])) {
        fprintf(stderr, "usage: %s <case> <dir> <ints...>; cases:", argv[0]);
        for (auto &kv : CASES) fprintf(stderr, " %s", kv.first.c_str());
        fprintf(stderr, "\n");
        return 2;
    }
    g_dir = argv[2];
    std::vector<int> ints;
    for (int k = 3; k < argc; k++) ints.push_back((int)strtol(argv[k], nullptr, 0));
    std::map<std::string, std::vector<unsigned char>> first;
    std::string first_status;
    for (int which = 0; which < 2; which++) {
        Run r(which);
        try { CASES.at(argv[1])(r, ints); }
        catch (const std::out_of_range &) { fprintf(stderr, "%s: too few integer arguments\n", argv[1]); return 2; }
        const std::string bad = r.A.bands();
        if (!bad.empty()) { fprintf(stderr, "guard band beside %s changed (prefill %d)\n", bad.c_str(), which); return 3; }
        std::map<std::string, std::vector<unsigned char>> all = r.A.contents();
        for (auto &kv : r.extra) all[kv.first] = kv.second;
        if (which == 0) { first = all; first_status = r.status; continue; }
        for (auto &kv : all)
            if (first.at(kv.first) != kv.second) { fprintf(stderr, "%s depends on what the buffers held before the call\n", kv.first.c_str()); return 4; }
        if (first_status != r.status) { fprintf(stderr, "status depends on the prefill:\n%s---\n%s", first_status.c_str(), r.status.c_str()); return 4; }
    }
    for (auto &kv : first) write_file(kv.first, kv.second.data(), kv.second.size());
    FILE *f = fopen((g_dir + "/status.txt").c_str(), "w");
    if (!f) return 2;
    fputs(first_status.c_str(), f);
    fclose(f);
    return 0;
}
