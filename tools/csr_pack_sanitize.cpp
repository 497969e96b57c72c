// csr_pack_sanitize.cpp -- the CSR packer (csr_build_groups and its steps, kn_csr.hip) and the dispatch choice (csr_choice) under the host sanitizers, as a
// stand-alone program: it creates, plans and destroys the mixed CSR shapes of tools/plan_grid.py (csr_cases) through the C ABI.  Built together with the library
// sources in the CPU-only diagnostic form (host heap stands in for device memory, nothing is launched), so it runs on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -DKN_HOST_PACK_ONLY -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/csr_pack_sanitize.cpp keynet_amd/csrc/*.hip -o csr_pack_sanitize
//   ./csr_pack_sanitize            (prints CSR_PACK_SANITIZE_OK and exits 0; a sanitizer report aborts it)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "../include/keynet_hip.h"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) {      // xorshift64: the same operators on every run
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

struct Csr {
    int64_t cols;
    std::vector<int32_t> indptr{0}, indices;
    std::vector<float> data;
    void row(const std::vector<int32_t>& seq) {
        for (int32_t c : seq) {
            indices.push_back(c);
            data.push_back((float)rnd(2001) / 1000.0f - 1.0f);
        }
        indptr.push_back((int32_t)indices.size());
    }
    std::vector<int32_t> sequence(int len) {      // `len` distinct columns in random order (a partial shuffle)
        std::vector<int32_t> all((size_t)cols);
        std::iota(all.begin(), all.end(), 0);
        for (int k = 0; k < len; k++) std::swap(all[(size_t)k], all[(size_t)k + rnd((uint32_t)(cols - k))]);
        all.resize((size_t)len);
        return all;
    }
    void group(int members, int len) {
        const std::vector<int32_t> seq = sequence(len);
        for (int m = 0; m < members; m++) row(seq);
    }
};

static int check(int rc, const char* what) {
    if (rc != KN_OK) std::fprintf(stderr, "%s: rc=%d %s\n", what, rc, kn_last_error());
    return rc;
}

// create under the defaults and under each switch, plan narrow and wide calls, destroy
static int run(const char* name, const Csr& m) {
    const char* switches[][2] = {{nullptr, nullptr}, {"KN_MF_NRB", "3"}, {"KN_NO_BIG_GROUPS", "1"}, {"KN_GROUP_MFMA", "1"}, {"KN_BIG_MFMA16", "1"}};
    for (const auto& sw : switches) {
        if (sw[0]) setenv(sw[0], sw[1], 1);
        kn_handle_t h = nullptr;
        const int rc = check(kn_csr_create((int64_t)m.indptr.size() - 1, m.cols, (int64_t)m.indices.size(), m.indptr.data(), m.indices.data(), m.data.data(), &h), name);
        if (sw[0]) unsetenv(sw[0]);
        if (rc) return rc;
        char buf[4096];
        for (int64_t n : {1, 3, 8, 128, 384, 4096})
            for (uint32_t fl : {0u, KN_FLAG_RELU, KN_FLAG_NARROW_ROWS})
                if (check(kn_spmm_plan(h, n, n, n, fl, buf, sizeof buf), name)) return 1;
        if (check(kn_destroy(h), name)) return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    {   // matrix-pipe groups (chunks of 1, 2, 3 row blocks), small groups beside them, loose and empty rows
        Csr m{4096};
        for (int g = 0; g < 30; g++) m.group(32, 256);
        for (int n : {64, 96, 40, 2, 5, 9, 16, 23}) m.group(n, n >= 24 ? 256 : 64);
        for (int r = 0; r < 10; r++) m.row(m.sequence(5 + (int)rnd(25)));
        for (int r = 0; r < 3; r++) m.row({});
        bad |= run("matrix-pipe groups", m);
    }
    {   // a keyed Linear: one big group
        Csr m{2100};
        m.group(300, 2100);
        bad |= run("linear 300x2100", m);
    }
    {   // patched rows, long rows, loose rows too long for a lane, empty rows
        Csr m{3000};
        const std::vector<int32_t> seq = m.sequence(48);
        for (int r = 0; r < 30; r++) m.row(seq);
        for (int miss = 1; miss <= 5; miss++) m.row(std::vector<int32_t>(seq.begin() + miss, seq.end()));      // (5 missing: not patched)
        m.group(3, 20);
        m.group(17, 20);
        for (int r = 0; r < 2; r++) m.row(m.sequence(1024 + (int)rnd(6)));
        for (int r = 0; r < 12; r++) m.row(m.sequence(70 + (int)rnd(30)));
        for (int r = 0; r < 3; r++) m.row({});
        bad |= run("mixed", m);
    }
    {   // 4 096 short loose rows: the locality order
        Csr m{4100};
        for (int32_t r = 0; r < 4096; r++) m.row({r, r + 1, r + 2});
        bad |= run("pool 4096x4100", m);
    }
    {   // nothing at all, and rows without entries only
        Csr m{7};
        bad |= run("0 rows", m);
        for (int r = 0; r < 5; r++) m.row({});
        bad |= run("empty rows", m);
    }
    if (bad) return 1;
    std::puts("CSR_PACK_SANITIZE_OK");
    return 0;
}
