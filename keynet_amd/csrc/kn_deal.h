// kn_deal.h -- the order in which the output pixels of a conv-taps operator are dealt to the 8 XCDs (plain C++17, host only).
//
// The matrix-core kernels (convtaps_mfma_kernel, convtaps_bf16x3_kernel) give every XCD a contiguous chunk of ceil(n_items / 8) work items, items in the order
// of ConvArgs::pix_order.  An item's K loop is as long as its pixel's slot count (keyed 3x3 / pad 1: 9 interior, 6 edge, 4 corner), so equal COUNTS of the
// locality order are unequal WORK: an XCD whose eighth of it lies along the image border runs dry while the others finish.  deal_order re-arranges a
// processing order so that
//   * the eight segments [k n / 8, (k + 1) n / 8) carry equal slot weight at equal pixel counts (whatever n_bt x n_mt is, a chunk is a union of such
//     segments, give or take a straddling pixel),
//   * inside a segment the heavy pixels come first: the drain of a chunk and its quarter-tile tail are made of the light ones,
//   * inside a segment the pixels of one weight keep the order they came in, i.e. the locality that order was built for.
// The rule: the distinct weights are classes, heaviest first.  Each class's pixels, in the order they came, are cut into eight contiguous pieces of equal
// count (+-1); segment k is its piece of the heaviest class, then its piece of the next, and so on.  Which segments take a class's +1 remainders is the only
// freedom: segment k must end up with exactly ceil((k + 1) n / 8) - ceil(k n / 8) pixels, so a remainder goes to the segments that still need the most pixels
// (their needs never differ by more than one, which is why this never gets stuck) and, among equals, to those that carry the least weight so far.  With the
// heaviest classes dealt first, the lighter ones even out what the heavier ones left.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kn {

constexpr int DEAL_PARTS = 8;       // XCDs of the device = segments of a dealt order

// max / mean of the weights of the DEAL_PARTS segments [k n / 8, (k + 1) n / 8) of `order` (weight[o]: by pixel id); a pixel that straddles a boundary counts
// with the fraction on either side.  1.0 for an empty order or all-zero weights.
inline double deal_imbalance(const std::vector<int32_t>& order, const std::vector<int32_t>& weight) {
    const int64_t n = (int64_t)order.size();
    int64_t seg[DEAL_PARTS] = {0};                           // in eighths of a weight unit: position p covers [8 p, 8 p + 8) of a line cut at multiples of n
    int64_t total = 0;
    for (int64_t p = 0; p < n; p++) {
        const int64_t w = weight[(size_t)order[(size_t)p]];
        int64_t lo = 8 * p;
        const int64_t hi = lo + 8;
        while (lo < hi) {
            const int64_t k = lo / n;
            const int64_t end = std::min(hi, (k + 1) * n);
            seg[k] += w * (end - lo);
            lo = end;
        }
        total += 8 * w;
    }
    if (total <= 0) return 1.0;
    return (double)*std::max_element(seg, seg + DEAL_PARTS) * DEAL_PARTS / (double)total;
}

// `order` (a permutation of 0 .. n - 1, or any list of distinct pixel ids) re-arranged as described above.  All weights equal: `order` itself.
inline std::vector<int32_t> deal_order(const std::vector<int32_t>& order, const std::vector<int32_t>& weight) {
    const int64_t n = (int64_t)order.size();
    std::vector<int32_t> classes;                            // the distinct weights, heaviest first
    for (int32_t o : order) classes.push_back(weight[(size_t)o]);
    std::sort(classes.begin(), classes.end(), [](int32_t a, int32_t b) { return a > b; });
    classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
    if (classes.size() <= 1) return order;
    const size_t n_cls = classes.size();
    auto class_of = [&](int32_t o) { return (size_t)(std::lower_bound(classes.begin(), classes.end(), weight[(size_t)o], [](int32_t a, int32_t b) { return a > b; }) - classes.begin()); };
    std::vector<std::vector<int32_t>> members(n_cls);       // each class's pixels in the order they came
    for (int32_t o : order) members[class_of(o)].push_back(o);

    int64_t need[DEAL_PARTS], load[DEAL_PARTS] = {0};        // pixels a segment still has to take beyond the whole eighths; weight dealt to it so far
    for (int k = 0; k < DEAL_PARTS; k++) need[k] = ((k + 1) * n + 7) / 8 - (k * n + 7) / 8;
    for (size_t j = 0; j < n_cls; j++)
        for (int k = 0; k < DEAL_PARTS; k++) need[k] -= (int64_t)members[j].size() / DEAL_PARTS;
    std::vector<int64_t> piece(n_cls * DEAL_PARTS);
    for (size_t j = 0; j < n_cls; j++) {
        const int64_t base = (int64_t)members[j].size() / DEAL_PARTS, rem = (int64_t)members[j].size() % DEAL_PARTS;
        int by_need[DEAL_PARTS];
        for (int k = 0; k < DEAL_PARTS; k++) by_need[k] = k;
        std::stable_sort(by_need, by_need + DEAL_PARTS, [&](int a, int b) { return need[a] != need[b] ? need[a] > need[b] : load[a] < load[b]; });
        for (int k = 0; k < DEAL_PARTS; k++) piece[j * DEAL_PARTS + (size_t)k] = base;
        for (int64_t r = 0; r < rem; r++) {
            piece[j * DEAL_PARTS + (size_t)by_need[r]]++;
            need[by_need[r]]--;
        }
        for (int k = 0; k < DEAL_PARTS; k++) load[k] += piece[j * DEAL_PARTS + (size_t)k] * classes[j];
    }

    std::vector<int32_t> deal;
    deal.reserve((size_t)n);
    std::vector<size_t> taken(n_cls, 0);                     // piece k of a class starts where its piece k - 1 ended
    for (int k = 0; k < DEAL_PARTS; k++)
        for (size_t j = 0; j < n_cls; j++) {
            const size_t cnt = (size_t)piece[j * DEAL_PARTS + (size_t)k];
            deal.insert(deal.end(), members[j].begin() + (std::ptrdiff_t)taken[j], members[j].begin() + (std::ptrdiff_t)(taken[j] + cnt));
            taken[j] += cnt;
        }
    return deal;
}

}  // namespace kn
