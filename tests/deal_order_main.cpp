// Stand-alone checks of keynet_amd/csrc/kn_deal.h (tests/test_deal_order.py compiles this with the address and undefined-behaviour sanitizers and runs it).
// Base orders are row-major: kn::locality_order is not in the header, and the properties checked hold for any base order.  Prints one line per
// case and "FAIL ..." lines for every condition missed; exit status 1 if any.
#include "kn_deal.h"

#include <cstdio>
#include <random>
#include <string>

using kn::deal_imbalance;
using kn::deal_order;

static int g_failures = 0;

static void fail(const std::string& name, const char* what) {
    std::printf("FAIL %s: %s\n", name.c_str(), what);
    g_failures++;
}

// slots of a 3x3 / pad-1 conv per output pixel of an H x W image
static std::vector<int32_t> conv3_weights(int H, int W) {
    std::vector<int32_t> w((size_t)(H * W));
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const int ny = 1 + (y > 0) + (y < H - 1), nx = 1 + (x > 0) + (x < W - 1);
            w[(size_t)(y * W + x)] = ny * nx;
        }
    return w;
}

static std::vector<int32_t> row_major(size_t n) {
    std::vector<int32_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = (int32_t)i;
    return o;
}

// (a) permutation, (d) heavy first inside every segment, (f) a class keeps its relative order inside every segment
static void check_structure(const std::string& name, const std::vector<int32_t>& base, const std::vector<int32_t>& w, const std::vector<int32_t>& deal) {
    const int64_t n = (int64_t)base.size();
    if ((int64_t)deal.size() != n) return fail(name, "(a) length differs");
    std::vector<int64_t> pos_in_base(w.size(), -1);
    for (int64_t p = 0; p < n; p++) pos_in_base[(size_t)base[(size_t)p]] = p;
    std::vector<char> seen(w.size(), 0);
    for (int32_t o : deal) {
        if (o < 0 || (size_t)o >= w.size() || pos_in_base[(size_t)o] < 0 || seen[(size_t)o]) return fail(name, "(a) not a permutation of the input");
        seen[(size_t)o] = 1;
    }
    for (int k = 0; k < 8; k++) {
        // positions wholly inside [k n / 8, (k + 1) n / 8): p >= k n / 8 and p + 1 <= (k + 1) n / 8; the pixel straddling either end is left out
        const int64_t first = (k * n + 7) / 8, last = (k + 1) * n / 8;       // [first, last)
        for (int64_t p = first + 1; p < last; p++) {
            const int32_t a = deal[(size_t)p - 1], b = deal[(size_t)p];
            if (w[(size_t)a] < w[(size_t)b]) fail(name, "(d) a heavier pixel follows a lighter one inside a segment");
            if (w[(size_t)a] == w[(size_t)b] && pos_in_base[(size_t)a] > pos_in_base[(size_t)b]) fail(name, "(f) a class lost its input order inside a segment");
        }
    }
}

static double run_case(const std::string& name, const std::vector<int32_t>& base, const std::vector<int32_t>& w) {
    const std::vector<int32_t> deal = deal_order(base, w);
    check_structure(name, base, w, deal);
    const double before = deal_imbalance(base, w), after = deal_imbalance(deal, w);
    std::printf("%-22s n=%-5zu imbalance %.4f -> %.4f\n", name.c_str(), base.size(), before, after);
    return after;
}

int main() {
    // (a), (d), (f) on every grid; (c) balance on the three VGG-16 sizes
    const int grids[][2] = {{1, 1}, {2, 2}, {3, 3}, {5, 5}, {14, 14}, {28, 28}, {56, 56}, {9, 7}, {13, 1}};
    for (const auto& g : grids) {
        const std::string name = "conv3x3 " + std::to_string(g[0]) + "x" + std::to_string(g[1]);
        const double imb = run_case(name, row_major((size_t)(g[0] * g[1])), conv3_weights(g[0], g[1]));
        const double bound = g[0] == 14 && g[1] == 14 ? 1.02 : (g[0] == 28 ? 1.005 : (g[0] == 56 ? 1.002 : 0.0));
        if (bound > 0.0 && !(imb <= bound)) fail(name, "(c) imbalance above the bound");
    }
    // a base order that is not the identity: the permutation and order conditions are about the INPUT order, not about pixel ids
    {
        std::vector<int32_t> base = row_major(14 * 14);
        std::mt19937 rng(7);
        std::shuffle(base.begin(), base.end(), rng);
        const double imb = run_case("conv3x3 14x14 shuffled", base, conv3_weights(14, 14));
        if (!(imb <= 1.02)) fail("conv3x3 14x14 shuffled", "(c) imbalance above the bound");
    }
    // (b) uniform weights: the input comes back element for element (also for n < 8 and n % 8 != 0)
    for (int n : {0, 1, 5, 8, 100, 197}) {
        std::vector<int32_t> base = row_major((size_t)n);
        std::reverse(base.begin(), base.end());
        const std::vector<int32_t> w((size_t)n, 9);
        if (deal_order(base, w) != base) fail("uniform n=" + std::to_string(n), "(b) output differs from input");
        if (deal_imbalance(base, w) > 1.0 + 1e-12) fail("uniform n=" + std::to_string(n), "uniform weights are not balanced by the measure");
    }
    // (e) float-key case: weights 1 .. 19 on 784 pixels, fixed seed
    {
        std::mt19937 rng(12345);
        std::vector<int32_t> w(784);
        for (auto& v : w) v = 1 + (int32_t)(rng() % 19);
        const std::vector<int32_t> base = row_major(784);
        const double before = deal_imbalance(base, w);
        const double after = run_case("random 1..19 on 784", base, w);
        if (!(after <= before)) fail("random 1..19 on 784", "(e) imbalance grew");
        if (!(after <= 1.01)) fail("random 1..19 on 784", "(e) imbalance above 1.01");
    }
    // the measure itself: eight pixels of weight 1 .. 8 -> max / mean = 8 / 4.5; a pixel straddling a boundary counts by its fractions
    {
        const std::vector<int32_t> w = {1, 2, 3, 4, 5, 6, 7, 8};
        const double imb = deal_imbalance(row_major(8), w);
        if (imb < 8 / 4.5 - 1e-12 || imb > 8 / 4.5 + 1e-12) fail("measure", "eight single-pixel segments");
        const std::vector<int32_t> w4 = {8, 0, 0, 0};          // n = 4: the first pixel covers segments 0 and 1, half each -> max 4, mean 1
        const double imb4 = deal_imbalance(row_major(4), w4);
        if (imb4 < 4.0 - 1e-12 || imb4 > 4.0 + 1e-12) fail("measure", "fractional count of a straddling pixel");
    }
    if (g_failures) std::printf("%d condition(s) failed\n", g_failures);
    else std::printf("all conditions hold\n");
    return g_failures ? 1 : 0;
}
