// chain_pack_sanitize.cpp -- the whole-net packer (chain_create and its steps, kn_chain.hip) under the host sanitizers, as a stand-alone program: it creates, plans and
// destroys the operator stacks of tools/plan_grid.py (chain_cases: the shapes, from its own generator) through the C ABI, under the defaults and under each
// KN_CHAIN_NO_* knob.  Built together with the library sources in the CPU-only diagnostic form (host heap stands in for device memory, nothing is launched), so it runs
// on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -DKN_HOST_PACK_ONLY -DKN_ABLATION -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined tools/chain_pack_sanitize.cpp keynet_amd/csrc/*.hip -o chain_pack_sanitize
//   ./chain_pack_sanitize          (prints CHAIN_PACK_SANITIZE_OK and exits 0; a sanitizer report aborts it)
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
static float rnd_value() { return (float)rnd(2001) / 1000.0f - 1.0f; }

struct Csr {
    int64_t cols;
    uint32_t relu;
    std::vector<int32_t> indptr{0}, indices;
    std::vector<float> data;
    int64_t rows() const { return (int64_t)indptr.size() - 1; }
    void row(const std::vector<int32_t>& seq, const float* vals = nullptr) {
        for (size_t k = 0; k < seq.size(); k++) {
            indices.push_back(seq[k]);
            data.push_back(vals ? vals[k] : rnd_value());
        }
        indptr.push_back((int32_t)indices.size());
    }
    std::vector<int32_t> any(int len) {            // `len` random columns, duplicates allowed
        std::vector<int32_t> s((size_t)len);
        for (int32_t& c : s) c = (int32_t)rnd((uint32_t)cols);
        return s;
    }
    std::vector<int32_t> distinct(int len) {       // `len` distinct columns in random order (a partial shuffle)
        std::vector<int32_t> all((size_t)cols);
        std::iota(all.begin(), all.end(), 0);
        for (int k = 0; k < len; k++) std::swap(all[(size_t)k], all[(size_t)k + rnd((uint32_t)(cols - k))]);
        all.resize((size_t)len);
        return all;
    }
};

// conv-like: groups of `group` rows over one sequence of `nnz` columns, `tail_loose` short rows of their own at the end
static Csr grouped(int rows, int cols, int group, int nnz, int tail_loose, uint32_t relu) {
    Csr m{cols, relu};
    std::vector<int32_t> shared;
    for (int r = 0; r < rows; r++) {
        if (r >= rows - tail_loose) {
            m.row(m.any(1 + (int)rnd(5)));
            continue;
        }
        if (r % group == 0) shared = m.any(nnz);
        m.row(shared);
    }
    return m;
}
// a keyed Linear: rows - n_other rows over one sequence of seq_len distinct columns, n_other rows of 1 .. 3 columns behind them
static Csr dense(int rows, int cols, int n_other, uint32_t relu, int seq_len = 0) {
    Csr m{cols, relu};
    const std::vector<int32_t> seq = m.distinct(seq_len ? seq_len : cols);
    for (int r = 0; r < rows - n_other; r++) m.row(seq);
    for (int r = 0; r < n_other; r++) m.row(m.distinct(1 + (int)rnd(3)));
    return m;
}
// unrelated rows of 0 .. 13 columns, a row in thirteen empty
static Csr loose(int rows, int cols, uint32_t relu) {
    Csr m{cols, relu};
    for (int r = 0; r < rows; r++) m.row(m.any(r % 13 == 5 ? 0 : 1 + (int)rnd(13)));
    return m;
}
// `pixels` column sequences of `ch` rows each; shared_values: every pixel carries the same `ch` value sequences, rotated per pixel
static Csr pixels(int n_pixels, int ch, int nnz, int cols, bool shared_values) {
    Csr m{cols, 1};
    std::vector<float> base((size_t)(ch * nnz));
    for (float& v : base) v = rnd_value();
    for (int p = 0; p < n_pixels; p++) {
        const std::vector<int32_t> seq = m.any(nnz);
        const int rot = (int)rnd((uint32_t)ch);
        for (int c = 0; c < ch; c++) m.row(seq, shared_values ? base.data() + (size_t)((c + rot) % ch) * (size_t)nnz : nullptr);
    }
    return m;
}

static int check(int rc, const char* what) {
    if (rc != KN_OK) std::fprintf(stderr, "%s: rc=%d %s\n", what, rc, kn_last_error());
    return rc;
}

// the operators and the chain created under the defaults and under each knob (read when an operator is created), planned, destroyed
static int run(const char* name, const std::vector<Csr>& stack) {
    const char* knobs[] = {nullptr, "KN_CHAIN_NO_CL", "KN_CHAIN_NO_RPL2", "KN_CHAIN_NO_EARLY", "KN_CHAIN_NO_SEQ", "KN_CHAIN_NO_SHARE"};
    for (const char* knob : knobs) {
        if (knob) setenv(knob, "1", 1);
        std::vector<kn_handle_t> ops(stack.size(), nullptr);
        std::vector<uint32_t> flags;
        int rc = 0;
        for (size_t l = 0; l < stack.size() && !rc; l++) {
            const Csr& m = stack[l];
            rc = check(kn_csr_create(m.rows(), m.cols, (int64_t)m.indices.size(), m.indptr.data(), m.indices.data(), m.data.data(), &ops[l]), name);
            flags.push_back(m.relu ? KN_FLAG_RELU : 0u);
        }
        if (knob) unsetenv(knob);
        kn_handle_t chain = nullptr;
        if (!rc) rc = check(kn_chain_create((int64_t)ops.size(), ops.data(), flags.data(), &chain), name);
        char buf[4096];
        for (int64_t n : {1, 3, 4, 5, 37, 1024})
            if (!rc) rc = check(kn_spmm_plan(chain, n, n, n, KN_FLAG_EXACT, buf, sizeof buf), name);
        if (chain) rc |= check(kn_destroy(chain), name);
        for (kn_handle_t h : ops)
            if (h) rc |= check(kn_destroy(h), name);
        if (rc) return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    bad |= run("random", {grouped(301, 97, 7, 23, 0, 1), loose(150, 301, 0), dense(70, 150, 6, 1), dense(33, 70, 3, 1), dense(9, 33, 1, 0)});
    bad |= run("pattern pools", {grouped(645, 200, 6, 11, 5, 1), grouped(130, 645, 16, 50, 2, 0), dense(70, 130, 0, 1), dense(10, 70, 0, 0)});
    bad |= run("keyed linears", {grouped(645, 200, 6, 11, 5, 1), grouped(131, 645, 16, 50, 2, 0), dense(121, 131, 1, 1), dense(85, 121, 3, 1), dense(11, 85, 1, 0)});
    bad |= run("linear first", {dense(70, 130, 0, 1), dense(10, 70, 1, 0)});
    bad |= run("pool does not fit", {grouped(4100, 4200, 6, 110, 2, 1), grouped(64, 4100, 8, 9, 0, 0)});
    bad |= run("two rows per lane 6 16", {grouped(2051, 300, 6, 11, 5, 1), grouped(1300, 2051, 1, 7, 0, 0), grouped(1609, 1300, 16, 50, 9, 1), dense(90, 1609, 0, 1), dense(10, 90, 0, 0)});
    bad |= run("two rows per lane 11", {grouped(1500, 257, 11, 13, 1, 0), dense(33, 1500, 0, 0)});
    bad |= run("linear 336x2184 first", {dense(336, 2184, 9, 0), dense(50, 336, 1, 1)});
    bad |= run("thin pool does not fit", {dense(70, 9000, 0, 0, 2800)});
    bad |= run("thin pool fits", {dense(70, 8600, 0, 0, 2800)});
    bad |= run("pixels, shared values", {pixels(600, 8, 22, 500, true)});
    bad |= run("pixels, own values", {pixels(600, 8, 22, 500, false)});
    {   // nothing at all, and rows without entries only
        Csr m{7, 0};
        bad |= run("0 rows", {m});
        for (int r = 0; r < 5; r++) m.row({});
        bad |= run("empty rows", {m});
    }
    if (bad) return 1;
    std::puts("CHAIN_PACK_SANITIZE_OK");
    return 0;
}
