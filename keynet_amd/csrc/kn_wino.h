// kn_wino.h -- KN_MODIFIER_WINO on the host: is a conv-taps operator a keyed 3 x 3 convolution of an image of even width, and if so, which operator is its 1-D Winograd
// F(2,3) form along the image rows?  Plain C++17 (no HIP): kn_conv_wino.hip derives the form of a handle from it, tests/wino_host_main.cpp runs it under the host sanitizers.
//
// One output row, output columns 2c and 2c + 1, kernel row r with weights g0 g1 g2, input pixels d0 .. d3 at columns 2c - 1 .. 2c + 2 of input row y + r - 1 (a pixel
// outside the image is zero):
//     V0 = d0 - d2       V1 = d1 + d2            V2 = d2 - d1            V3 = d1 - d3
//     U0 = g0            U1 = (g0 + g1 + g2)/2   U2 = (g0 - g1 + g2)/2   U3 = g2             (per (r, Cin, Cout); formed in double, rounded once to f32)
//     Mj = sum over r, ci of Uj[r] * Vj(row y + r - 1, pair c)                                 (four products with K = 3 * Cin instead of two with K = 9 * Cin)
//     y(2c) = M0 + M1 + M2        y(2c + 1) = M1 - M2 - M3
// Vj depends on the input row and the pair, not on r: V is [Cin][HiWi / 2 pairs][4], twice the activation block, and the products are a conv-taps operator of its own --
// 2 * HoWo pseudo output pixels (4 P + j), at most 3 slots each, on 2 * HiWi pseudo input pixels (4 p + j), 12 tap matrices (3 j + r), unit coefficients, no last column.
//
// Everything is read off the operator's OWN entry table (output pixel, input pixel, tap = 3 * i + j as keynet_amd/direct.py emits it): the key permutes pixels on both
// sides, so no pixel index means a position.  The centre tap gives an output pixel its input position, the pixel whose tap (1, 0) reads that position is its right
// neighbour, pixels without a tap (1, 0) start a row, and the finished tables are expanded again and compared with the whole entry table as a set: whatever the walk assumed
// wrongly shows there, and the operator is then not eligible (wino_derive says why; nothing throws).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace kn {

struct WinoTables {
    bool ok = false;
    std::string why;                        // the reason when !ok
    std::vector<int32_t> out_pair;          // [HoWo / 2][2] the output pixels (even column, odd column) of pair P
    std::vector<int32_t> in_d;              // [HiWi / 2][4] the input pixels d0 .. d3 of input pair p (-1: outside the image)
    std::vector<int32_t> ent_out, ent_in, ent_tap;      // the derived operator: pseudo output pixel 4 P + j, pseudo input pixel 4 p + j, tap 3 j + r
};

inline WinoTables wino_refuse(const std::string& why) {
    WinoTables t;
    t.why = why;
    return t;
}

// eo / ei / et: the operator's entries; `unit_coef`: every coefficient is 1; `has_dups`: some (output pixel, input pixel) pair is hit twice
inline WinoTables wino_derive(int64_t HoWo, int64_t HiWi, int64_t ntaps, bool unit_coef, bool has_dups, const std::vector<int32_t>& eo, const std::vector<int32_t>& ei,
                              const std::vector<int32_t>& et) {
    if (ntaps != 9) return wino_refuse("not a 3 x 3 operator (" + std::to_string(ntaps) + " taps)");
    if (!unit_coef) return wino_refuse("entries carry coefficients other than 1");
    if (has_dups) return wino_refuse("an (output pixel, input pixel) pair is hit by more than one entry");
    if (HoWo != HiWi || HoWo <= 0) return wino_refuse("output and input images differ in size");
    if (HoWo % 2) return wino_refuse("odd number of pixels: the image width is odd");
    const size_t nent = eo.size();
    std::vector<int32_t> tab((size_t)HoWo * 9, -1);             // [o][tap] -> input pixel
    for (size_t e = 0; e < nent; e++) {
        if (eo[e] < 0 || eo[e] >= HoWo || ei[e] < 0 || ei[e] >= HiWi || et[e] < 0 || et[e] >= 9) return wino_refuse("entry out of range");
        int32_t& slot = tab[(size_t)eo[e] * 9 + (size_t)et[e]];
        if (slot >= 0) return wino_refuse("an (output pixel, tap) pair holds more than one entry");
        slot = ei[e];
    }
    // the centre tap: output pixel -> its input position, one to one
    std::vector<int32_t> at((size_t)HiWi, -1);                  // input position -> output pixel
    for (int64_t o = 0; o < HoWo; o++) {
        const int32_t c = tab[(size_t)o * 9 + 4];
        if (c < 0) return wino_refuse("an output pixel has no centre tap");
        if (at[(size_t)c] >= 0) return wino_refuse("two output pixels share a centre position");
        at[(size_t)c] = (int32_t)o;
    }
    // the right neighbour of o: the pixel whose tap (1, 0) reads o's position
    std::vector<int32_t> right((size_t)HoWo, -1);
    for (int64_t o = 0; o < HoWo; o++) {
        const int32_t l = tab[(size_t)o * 9 + 3];
        if (l < 0) continue;
        const int32_t left = at[(size_t)l];
        if (right[(size_t)left] >= 0) return wino_refuse("two pixels claim one left neighbour");
        right[(size_t)left] = (int32_t)o;
    }
    WinoTables t;
    std::map<std::pair<int32_t, int32_t>, int32_t> pair_of;    // (d1, d2) -> input pair
    int64_t walked = 0;
    for (int64_t start = 0; start < HoWo; start++) {
        if (tab[(size_t)start * 9 + 3] >= 0) continue;          // not a row start
        for (int32_t a = (int32_t)start; a >= 0;) {
            const int32_t b = right[(size_t)a];
            if (b < 0) return wino_refuse("a row of odd width");
            walked += 2;
            if (walked > HoWo) return wino_refuse("the rows do not partition the pixels");
            const int32_t P = (int32_t)(t.out_pair.size() / 2);
            t.out_pair.push_back(a);
            t.out_pair.push_back(b);
            for (int r = 0; r < 3; r++) {
                const int32_t* ta = &tab[(size_t)a * 9 + 3 * (size_t)r];
                const int32_t* tb = &tab[(size_t)b * 9 + 3 * (size_t)r];
                const int32_t d0 = ta[0], d1 = ta[1], d2 = ta[2], d3 = tb[2];
                if (tb[0] != d1 || tb[1] != d2) return wino_refuse("the overlapping taps of a pixel pair disagree");
                if ((d1 < 0) != (d2 < 0)) return wino_refuse("the padding patterns of a pixel pair disagree");
                if (d1 < 0) {
                    if (d0 >= 0 || d3 >= 0) return wino_refuse("the padding patterns of a pixel pair disagree");
                    continue;                                   // the kernel row lies outside the image
                }
                auto it = pair_of.find({d1, d2});
                if (it == pair_of.end()) {
                    it = pair_of.emplace(std::make_pair(d1, d2), (int32_t)(t.in_d.size() / 4)).first;
                    t.in_d.insert(t.in_d.end(), {d0, d1, d2, d3});
                } else {
                    const int32_t* d = &t.in_d[(size_t)it->second * 4];
                    if (d[0] != d0 || d[3] != d3) return wino_refuse("one input pair is seen with different neighbours");
                }
                for (int j = 0; j < 4; j++) {
                    t.ent_out.push_back(4 * P + j);
                    t.ent_in.push_back(4 * it->second + j);
                    t.ent_tap.push_back(3 * j + r);
                }
            }
            a = right[(size_t)b];
        }
    }
    if (walked != HoWo) return wino_refuse("the rows do not partition the pixels");
    if ((int64_t)t.in_d.size() / 4 != HiWi / 2) return wino_refuse("the input pairs number " + std::to_string(t.in_d.size() / 4) + ", not HiWi / 2");
    // the set comparison: the tables, expanded, are the entry table
    std::vector<std::array<int32_t, 3>> mine, theirs(nent);
    mine.reserve(nent);
    for (size_t k = 0; k < t.ent_out.size(); k += 4) {          // one (pair, kernel row) per four derived entries
        const int32_t P = t.ent_out[k] / 4, p = t.ent_in[k] / 4, r = t.ent_tap[k] % 3;
        const int32_t* d = &t.in_d[(size_t)p * 4];
        for (int side = 0; side < 2; side++)
            for (int c = 0; c < 3; c++)
                if (d[side + c] >= 0) mine.push_back({t.out_pair[(size_t)P * 2 + (size_t)side], d[side + c], 3 * r + c});
    }
    for (size_t e = 0; e < nent; e++) theirs[e] = {eo[e], ei[e], et[e]};
    std::sort(mine.begin(), mine.end());
    std::sort(theirs.begin(), theirs.end());
    if (mine != theirs) return wino_refuse("the derived tables do not reproduce the entry table");
    t.ok = true;
    return t;
}

// The 12 tap matrices [3 j + r][Cout][Cin] of the form, in double, from the operator's nine [3 r + c][Cout][Cin]
inline std::vector<double> wino_taps(const std::vector<float>& taps, int64_t msz) {
    std::vector<double> u((size_t)(12 * msz));
    for (int r = 0; r < 3; r++)
        for (int64_t k = 0; k < msz; k++) {
            const double g0 = taps[(size_t)((3 * r + 0) * msz + k)], g1 = taps[(size_t)((3 * r + 1) * msz + k)], g2 = taps[(size_t)((3 * r + 2) * msz + k)];
            u[(size_t)((0 + r) * msz + k)] = g0;
            u[(size_t)((3 + r) * msz + k)] = (g0 + g1 + g2) / 2;
            u[(size_t)((6 + r) * msz + k)] = (g0 - g1 + g2) / 2;
            u[(size_t)((9 + r) * msz + k)] = g2;
        }
    return u;
}

}  // namespace kn
