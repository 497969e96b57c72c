// conv_choice_sanitize.cpp -- the conv-taps packers (kn_convtaps_create: slot lists, small-K descriptors) and the dispatch choices of kn_conv.hip (conv_regime, mfma_choice,
// narrow_choice, exact_choice) under the host sanitizers, as a stand-alone program: it creates, plans and destroys the conv-taps operators of tools/plan_grid.py (conv_cases)
// through the C ABI.  Built together with the library sources in the CPU-only diagnostic form (host heap stands in for device memory, nothing is launched), so it runs on a
// machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -DKN_HOST_PACK_ONLY -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/conv_choice_sanitize.cpp keynet_amd/csrc/*.hip -o conv_choice_sanitize
//   ./conv_choice_sanitize            (prints CONV_CHOICE_SANITIZE_OK and exits 0; a sanitizer report aborts it)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/keynet_hip.h"

static uint64_t rng_state = 88172645463325252ull;
static float rnd() {      // xorshift64: the same operators on every run; values in [-1, 1)
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (float)((rng_state >> 11) % 2001) / 1000.0f - 1.0f;
}

// plan_grid.py's factored(): `per_pixel` entries per output pixel of an hw x hw image on scattered input pixels (dup: on three input pixels only), nine taps
struct Conv {
    int64_t cin, cout, hw;
    int per_pixel = 9;
    bool coef = false, dup = false;
};

static int check(int rc, const char* what) {
    if (rc != KN_OK && rc != KN_ERR_UNSUPPORTED) std::fprintf(stderr, "%s: rc=%d %s\n", what, rc, kn_last_error());      // (a narrow call beyond 32-bit offsets is refused: expected)
    return (rc != KN_OK && rc != KN_ERR_UNSUPPORTED) ? rc : 0;
}

// create under the defaults and under each switch, plan every flag word at narrow and wide batches and at leading dimensions beyond 32-bit offsets, destroy
static int run(const char* name, const Conv& c) {
    const int64_t HW = c.hw * c.hw, ntaps = 9;
    std::vector<int32_t> eo, ei, et;
    for (int64_t o = 0; o < HW; o++)
        for (int k = 0; k < c.per_pixel; k++) {
            eo.push_back((int32_t)o);
            ei.push_back((int32_t)(c.dup ? o % 3 : (o + 7 * k) % HW));
            et.push_back((int32_t)(k % ntaps));
        }
    std::vector<float> taps((size_t)(ntaps * c.cout * c.cin)), ec(eo.size()), lastcol((size_t)(c.cout * HW + 1));
    for (float& v : taps) v = rnd();
    for (float& v : ec) v = 1.0f + 0.5f * rnd();
    for (float& v : lastcol) v = rnd();
    lastcol.back() = 1.0f;
    const int64_t inshape[3] = {c.cin, c.hw, c.hw}, outshape[3] = {c.cout, c.hw, c.hw};
    const char* switches[][2] = {{nullptr, nullptr}, {"KN_NO_SPTR", "1"}, {"KN_NO_SMALLK_PIPE", "1"}};
    for (const auto& sw : switches) {
        if (sw[0]) setenv(sw[0], sw[1], 1);
        kn_handle_t h = nullptr;
        const int rc = check(kn_convtaps_create(inshape, outshape, ntaps, taps.data(), (int64_t)eo.size(), eo.data(), ei.data(), et.data(), c.coef ? ec.data() : nullptr, lastcol.data(), &h), name);
        if (sw[0]) unsetenv(sw[0]);
        if (rc) return rc;
        char buf[4096];
        for (int64_t n : {1, 3, 5, 8, 9, 16, 17, 32, 128, 130, 256})
            for (int64_t ld : {n, n + 1, (int64_t)1 << 21, (int64_t)1 << 22, (int64_t)1 << 26})
                for (uint32_t fl : {0u, KN_FLAG_RELU, KN_FLAG_EXACT, KN_FLAG_BF16X3, KN_FLAG_NARROW, KN_FLAG_NARROW | KN_FLAG_NARROW32, KN_FLAG_NARROW_MFMA,
                                    KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW32, KN_FLAG_NARROW | KN_FLAG_EXACT | KN_FLAG_BF16X3})
                    if (check(kn_spmm_plan(h, n, ld, ld, fl, buf, sizeof buf), name)) return 1;
        if (check(kn_destroy(h), name)) return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    bad |= run("cin=3 cout=64 (small-K descriptors)", {3, 64, 6});
    bad |= run("cin=3 cout=128", {3, 128, 6});
    bad |= run("cin=3 cout=64, ten slots", {3, 64, 6, 10});
    bad |= run("cin=5 cout=128", {5, 128, 6});
    bad |= run("cin=16 cout=64", {16, 64, 6});
    bad |= run("cin=16 cout=128 coef", {16, 128, 6, 9, true});
    bad |= run("cin=32 cout=128", {32, 128, 6});
    bad |= run("cin=32 cout=64, 70 slots", {32, 64, 9, 70});
    bad |= run("cin=16 cout=64 dup coef", {16, 64, 6, 9, true, true});
    bad |= run("cin=256 cout=256", {256, 256, 6});
    if (bad) return 1;
    std::puts("CONV_CHOICE_SANITIZE_OK");
    return 0;
}
