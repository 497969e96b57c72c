// wino_host_main.cpp -- the host derivation of KN_MODIFIER_WINO (keynet_amd/csrc/kn_wino.h: plain C++17) as a stand-alone program, compiled under the address and
// undefined-behaviour sanitizers by tests/test_wino_host.py.  For every geometry it builds the entry table of a zero-padded 3 x 3 convolution under a pixel permutation
// on either side, derives the form, expands the original operator and T_out . U . T_in to dense double matrices (Cin = Cout = 2, U kept in double) and compares them.
// It prints a line per case and exits 1 when a condition is missed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>
#include "kn_wino.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd64() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static float rnd() { return (float)((rnd64() >> 11) % 2001) / 1000.0f - 1.0f; }

struct Entries {
    std::vector<int32_t> eo, ei, et;
};

// k x k convolution with zero padding of an H x W image, tap = k * i + j, output pixel po[y * W + x], input pixel pi[..]
static Entries conv_entries(int H, int W, int k, const std::vector<int32_t>& po, const std::vector<int32_t>& pi) {
    Entries e;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            for (int i = 0; i < k; i++)
                for (int j = 0; j < k; j++) {
                    const int yy = y + i - k / 2, xx = x + j - k / 2;
                    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    e.eo.push_back(po[(size_t)(y * W + x)]);
                    e.ei.push_back(pi[(size_t)(yy * W + xx)]);
                    e.et.push_back(k * i + j);
                }
    return e;
}

static std::vector<int32_t> permutation(int n, bool shuffle) {
    std::vector<int32_t> p((size_t)n);
    std::iota(p.begin(), p.end(), 0);
    if (shuffle)
        for (int i = n - 1; i > 0; i--) std::swap(p[(size_t)i], p[(size_t)(rnd64() % (uint64_t)(i + 1))]);
    return p;
}

static int bad = 0;
static void expect(bool cond, const std::string& what) {
    std::printf("%s %s\n", cond ? "ok  " : "FAIL", what.c_str());
    if (!cond) bad = 1;
}

static void eligible_case(int H, int W, bool shuffle) {
    const int C = 2, HW = H * W;
    const std::string name = std::to_string(H) + "x" + std::to_string(W) + (shuffle ? " permuted" : "");
    const Entries e = conv_entries(H, W, 3, permutation(HW, shuffle), permutation(HW, shuffle));
    const kn::WinoTables t = kn::wino_derive(HW, HW, 9, true, false, e.eo, e.ei, e.et);
    expect(t.ok, name + ": eligible" + (t.ok ? "" : " (" + t.why + ")"));
    if (!t.ok) return;
    expect((int)t.in_d.size() / 4 == HW / 2 && (int)t.out_pair.size() / 2 == HW / 2, name + ": HiWi / 2 pseudo input pixels per j");
    std::vector<float> taps((size_t)(9 * C * C));
    for (float& v : taps) v = rnd();
    const std::vector<double> u = kn::wino_taps(taps, C * C);
    const int R = C * HW, Q = C * 2 * HW;                      // rows of the operator, rows of V and of M
    std::vector<double> Worig((size_t)R * R, 0.0), Tin((size_t)Q * R, 0.0), U((size_t)Q * Q, 0.0), Tout((size_t)R * Q, 0.0);
    for (size_t k = 0; k < e.eo.size(); k++)
        for (int co = 0; co < C; co++)
            for (int ci = 0; ci < C; ci++) Worig[(size_t)(co * HW + e.eo[k]) * R + (size_t)(ci * HW + e.ei[k])] += taps[(size_t)((e.et[k] * C + co) * C + ci)];
    const double sin_[4][4] = {{1, 0, -1, 0}, {0, 1, 1, 0}, {0, -1, 1, 0}, {0, 1, 0, -1}};      // V_j in terms of d0 .. d3
    for (int ci = 0; ci < C; ci++)
        for (int p = 0; p < HW / 2; p++)
            for (int j = 0; j < 4; j++)
                for (int d = 0; d < 4; d++) {
                    const int32_t in = t.in_d[(size_t)(4 * p + d)];
                    if (in >= 0 && sin_[j][d] != 0.0) Tin[(size_t)(ci * 2 * HW + 4 * p + j) * R + (size_t)(ci * HW + in)] += sin_[j][d];
                }
    for (size_t k = 0; k < t.ent_out.size(); k++)
        for (int co = 0; co < C; co++)
            for (int ci = 0; ci < C; ci++) U[(size_t)(co * 2 * HW + t.ent_out[k]) * Q + (size_t)(ci * 2 * HW + t.ent_in[k])] += u[(size_t)((t.ent_tap[k] * C + co) * C + ci)];
    const double sout[2][4] = {{1, 1, 1, 0}, {0, 1, -1, -1}};
    for (int co = 0; co < C; co++)
        for (int P = 0; P < HW / 2; P++)
            for (int side = 0; side < 2; side++)
                for (int j = 0; j < 4; j++)
                    if (sout[side][j] != 0.0) Tout[(size_t)(co * HW + t.out_pair[(size_t)(2 * P + side)]) * Q + (size_t)(co * 2 * HW + 4 * P + j)] += sout[side][j];
    std::vector<double> UT((size_t)Q * R, 0.0);
    for (int a = 0; a < Q; a++)
        for (int b = 0; b < Q; b++) {
            const double v = U[(size_t)a * Q + b];
            if (v != 0.0)
                for (int c = 0; c < R; c++) UT[(size_t)a * R + c] += v * Tin[(size_t)b * R + c];
        }
    double worst = 0.0;
    for (int a = 0; a < R; a++)
        for (int c = 0; c < R; c++) {
            double s = 0.0;
            for (int b = 0; b < Q; b++) s += Tout[(size_t)a * Q + b] * UT[(size_t)b * R + c];
            worst = std::fmax(worst, std::fabs(s - Worig[(size_t)a * R + c]));
        }
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.3g", worst);
    expect(worst <= 1e-12, name + ": T_out . U . T_in equals the operator (worst element " + buf + ")");
}

static void refused(const std::string& name, const kn::WinoTables& t) {
    expect(!t.ok && !t.why.empty(), name + ": not eligible (" + t.why + ")");
}

int main() {
    eligible_case(6, 4, false);
    eligible_case(2, 2, false);
    eligible_case(1, 2, false);
    eligible_case(4, 6, true);
    {
        const Entries e = conv_entries(4, 3, 3, permutation(12, false), permutation(12, false));
        refused("4x3 (odd width)", kn::wino_derive(12, 12, 9, true, false, e.eo, e.ei, e.et));
    }
    {
        Entries e = conv_entries(6, 4, 3, permutation(24, false), permutation(24, false));
        e.eo.push_back(e.eo[5]);                                // a second entry on one (pixel, tap) pair, on another input pixel
        e.ei.push_back((e.ei[5] + 7) % 24);
        e.et.push_back(e.et[5]);
        refused("two entries on one (pixel, tap) pair", kn::wino_derive(24, 24, 9, true, false, e.eo, e.ei, e.et));
    }
    {
        const Entries e = conv_entries(6, 4, 3, permutation(24, false), permutation(24, false));
        refused("a coefficient other than 1", kn::wino_derive(24, 24, 9, false, false, e.eo, e.ei, e.et));
        Entries m = e;                                          // one entry moved to another input pixel: only the set comparison or the pair checks can see it
        m.ei[17] = (m.ei[17] + 11) % 24;
        refused("an entry moved to another input pixel", kn::wino_derive(24, 24, 9, true, false, m.eo, m.ei, m.et));
    }
    {
        const Entries e = conv_entries(6, 6, 5, permutation(36, false), permutation(36, false));
        refused("5x5 operator", kn::wino_derive(36, 36, 25, true, false, e.eo, e.ei, e.et));
    }
    if (bad) return 1;
    std::puts("all conditions hold");
    return 0;
}
