// kn_internal.h -- private to libkeynet_hip.so (gfx950 only; no CUDA / multi-backend paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <mutex>
#include <map>
#include <new>
#include <stdexcept>
#include <memory>
#include <type_traits>
#include "../../include/keynet_hip.h"

#ifdef KN_HOST_PACK_ONLY
// DIAGNOSTIC BUILD ONLY (tests/test_host_sanitize.py; never the product library): the HOST side of this library -- validation of
// caller-sized arrays, the std::vector index work that packs the reference's containers into the device formats, export, destroy --
// compiled with -fsanitize=address,undefined and run on a box WITHOUT a GPU.  "Device" memory is host heap here, so every create path
// runs to completion under the sanitizers (the packing loops, the copies INTO the packed buffers and the frees included); every compute
// entry point returns KN_ERR_NODEVICE before touching anything.
#include <cstdio>
#include <cstdlib>
#include <cstring>
namespace kn {
namespace hostonly {
// KN_UPLOAD_TRACE=<file>: every host-to-"device" copy appends one line -- element size, element count, 64-bit FNV-1a of the bytes -- and every kn_*_create
// entry (they all open with a device query) one blank line, so two builds pack an operator alike when the blocks between blank lines are equal as multisets
// (profiles/csr_host_before_after.txt).  An empty array (upload() zero-fills one element for it) is a line with count 0.  What reaches a kernel BY VALUE is
// appended as text (trace_text: kn_chain.hip writes the scalars of its ChainArgs, one line per layer record and one for the chain).
template <typename T> inline size_t elem_size(T*) { return sizeof(T); }
inline size_t elem_size(void*) { return 1; }
inline size_t elem_size(const void*) { return 1; }
inline void trace_write(bool blank, size_t elem, size_t count, const void* p) {
    static bool after_blank = true;
    const char* path = std::getenv("KN_UPLOAD_TRACE");
    if (!path || !*path || (blank && after_blank)) return;
    std::FILE* f = std::fopen(path, "a");
    if (!f) return;
    if (blank) {
        std::fputc('\n', f);
    } else {
        uint64_t h = 14695981039346656037ull;
        for (size_t i = 0; i < elem * count; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
        std::fprintf(f, "%zu %zu %016llx\n", elem, count, (unsigned long long)h);
    }
    std::fclose(f);
    after_blank = blank;
}
inline void trace_text(const std::string& line) {
    const char* path = std::getenv("KN_UPLOAD_TRACE");
    if (!path || !*path) return;
    if (std::FILE* f = std::fopen(path, "a")) {
        std::fprintf(f, "%s\n", line.c_str());
        std::fclose(f);
    }
}
inline hipError_t Malloc(void** p, size_t n) {
    *p = std::malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t Free(void* p) {
    std::free(p);
    return hipSuccess;
}
inline hipError_t Memcpy(void* d, const void* s, size_t n, hipMemcpyKind k, size_t elem) {
    std::memcpy(d, s, n);
    if (k == hipMemcpyHostToDevice) trace_write(false, elem, n / elem, s);
    return hipSuccess;
}
inline hipError_t Memset(void* d, int v, size_t n, size_t elem) {
    std::memset(d, v, n);
    trace_write(false, elem, 0, d);
    return hipSuccess;
}
inline hipError_t GetDeviceCount(int* n) {
    *n = 1;
    trace_write(true, 0, 0, nullptr);
    return hipSuccess;
}
inline hipError_t GetDevice(int* d) {
    *d = 0;
    trace_write(true, 0, 0, nullptr);
    return hipSuccess;
}
inline hipError_t DeviceGetAttribute(int* v, hipDeviceAttribute_t, int) {
    *v = 160 * 1024;
    return hipSuccess;
}
inline hipError_t Ok() { return hipSuccess; }
}  // namespace hostonly
}  // namespace kn
#define hipMalloc(p, n) kn::hostonly::Malloc((void**)(p), (n))
#define hipFree(p) kn::hostonly::Free((void*)(p))
#define hipMemcpy(d, s, n, k) kn::hostonly::Memcpy((void*)(d), (const void*)(s), (n), (k), kn::hostonly::elem_size(d))
#define hipMemset(d, v, n) kn::hostonly::Memset((void*)(d), (v), (n), kn::hostonly::elem_size(d))
#define hipGetDeviceCount(n) kn::hostonly::GetDeviceCount(n)
#define hipGetDevice(d) kn::hostonly::GetDevice(d)
#define hipDeviceGetAttribute(v, a, d) kn::hostonly::DeviceGetAttribute((v), (a), (d))
#define hipFuncSetAttribute(f, a, v) kn::hostonly::Ok()
#define hipGetLastError() kn::hostonly::Ok()
#define KN_HOST_ONLY_GUARD() return kn::fail(KN_ERR_NODEVICE, "KN_HOST_PACK_ONLY diagnostic build: no compute entry point runs")
#else
#define KN_HOST_ONLY_GUARD() do { } while (0)
#endif

namespace kn {

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define KN_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            return kn::fail(KN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
        }                                                                                              \
    } while (0)

#define KN_REQUIRE(cond, code, msg)                                                                    \
    do {                                                                                               \
        if (!(cond)) return kn::fail((code), std::string(msg) + " [" #cond "]");                       \
    } while (0)

// Every extern "C" body runs inside guarded(): the create functions do std::vector work on caller-sized inputs, and no C++ exception
// may unwind through the C ABI into ctypes / cgo / JNI (include/keynet_hip.h: "no C++ exception crosses the boundary").
template <typename F>
static inline int guarded(F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        try { return fail(KN_ERR_NOMEM, "host allocation failed (std::bad_alloc)"); } catch (...) { return KN_ERR_NOMEM; }
    } catch (const std::length_error& e) {
        try { return fail(KN_ERR_NOMEM, std::string("host allocation of an impossible size (std::length_error: ") + e.what() + ")"); } catch (...) { return KN_ERR_NOMEM; }
    } catch (const std::exception& e) {
        try { return fail(KN_ERR_INVALID, std::string("C++ exception: ") + e.what()); } catch (...) { return KN_ERR_INVALID; }
    } catch (...) {
        try { return fail(KN_ERR_INVALID, "unknown C++ exception"); } catch (...) { return KN_ERR_INVALID; }
    }
}

// kn_spmm_plan: the dispatch logic runs exactly as in kn_spmm, but every launch site describes itself into the sink instead of launching.
struct PlanSink {
    std::string text;
    int launches = 0;
};
PlanSink*& plan_sink();   // thread-local; null outside kn_spmm_plan

#define KN_LAUNCH(desc, kernel, grid, block, lds, stream, ...)                                                   \
    do {                                                                                                         \
        if (kn::PlanSink* _ps = kn::plan_sink()) {                                                               \
            if (_ps->launches) _ps->text += "; ";                                                                \
            _ps->text += (desc);                                                                                 \
            _ps->text += " grid=" + std::to_string((unsigned long long)(grid).x);                                \
            _ps->launches++;                                                                                     \
        } else {                                                                                                 \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                   \
        }                                                                                                        \
    } while (0)

// Options of an operator handle.  The environment is read ONCE, when a handle is created (tuning_from_env, kn_api.hip: the library's only
// getenv), the values are recorded in the handle and kn_spmm_plan prints the ones that differ from the defaults: a handle is immutable after
// create, kn_spmm's dispatch depends on the handle and the call's arguments only.  The first block are the switches the parity tests use to put
// two formulations of one product side by side; the second block are measured tuning constants that only the diagnostic build (-DKN_ABLATION,
// tools/ablate_conv.sh) reads from the environment -- in the product library they are the defaults below.
// One line per knob: X(field, environment variable, default, read from the environment by the diagnostic build only).  struct Tuning, tuning_from_env and
// Tuning::describe (in this order) are generated from this list.
#define KN_TUNING_KNOBS(X) \
    X(no_sptr, "KN_NO_SPTR", 0, false)               /* =1         conv-taps matrix-core kernel: per-thread pointers / generic loader instead of wave-uniform pointers */ \
    X(no_smallk_pipe, "KN_NO_SMALLK_PIPE", 0, false) /* =1         first-layer operators: the one-shot small-K kernel instead of the persistent pipeline */ \
    X(no_group_pipe, "KN_NO_GROUP_PIPE", 0, false)   /* =1         CSR pattern groups: the plain grouped kernel instead of the software-pipelined one */ \
    X(no_big_groups, "KN_NO_BIG_GROUPS", 0, false)   /* =1         a keyed Linear's rows as ordinary 16-row bundles instead of the LDS-staged workgroup kernel */ \
    X(no_exact_table, "KN_NO_EXACT_TABLE", 0, false) /* =1         factored untiled conv under KN_FLAG_EXACT: the conv pipeline instead of the stored-column table kernel */ \
    X(group_mfma, "KN_GROUP_MFMA", -1, false)        /* =0|1       CSR pattern groups with their products on the matrix pipe: never / always (-1: the dispatch rule) */ \
    X(big_mfma16, "KN_BIG_MFMA16", -1, false)        /* =0|1       a keyed Linear's 16-row chunks on the matrix pipe: never / always (-1: the dispatch rule) */ \
    X(mf_nrb, "KN_MF_NRB", 1, false)                 /* =1|2|3     32-row blocks per chunk of the matrix-pipe grouped kernel */ \
    X(table_nrb, "KN_TABLE_NRB", 0, false)           /* =1|2|3     32-channel blocks per workgroup of the table kernel (0: the rule) */ \
    X(no_fill_exact, "KN_NO_FILL_EXACT", 0, false)   /* =1         filled-in conv operators (> 64 slots per pixel, or several slots on one (output, input) pixel pair) under KN_FLAG_EXACT: the generic kernel instead of convtaps_exact_fill_kernel */ \
    X(no_fill_tiles2, "KN_NO_FILL_TILES2", 0, false) /* =1         ... on batches of whole 128-column tiles: one 64-column tile per wavefront instead of two */ \
    X(no_deal, "KN_NO_DEAL", 0, false)               /* =1         conv-taps matrix-core kernels: the XCD chunks cut from the locality order itself instead of the slot-balanced, heavy-first dealing order (kn_deal.h) */ \
    /* ---- diagnostic build only ---- */ \
    X(occ, "KN_OCC", 0, true)                        /* workgroups per CU cap of the 128 x 128 conv-taps launch (0: the rule) */ \
    X(no_tail_split, "KN_NO_TAIL_SPLIT", 0, true) \
    X(no_smallk, "KN_NO_SMALLK", 0, true) \
    X(exact_pipe, "KN_EXACT_PIPE", 16, true)         /* 0 = plain exact conv kernel, 8 / 16 = channels per wavefront of the pipeline */ \
    X(exact_cob_groups, "KN_EXACT_COB_GROUPS", 0, true) /* (0: the rule) */ \
    X(exact_xd, "KN_EXACT_XD", 0, true)              /* 2 | 4 activation rows in flight (0: the rule) */ \
    X(exact_vec, "KN_EXACT_VEC", 0, true)            /* 2 | 4 batch columns per lane of the exact conv pipeline (0: the rule) */ \
    X(mf_pf, "KN_MF_PF", 8, true)                    /* operand columns in flight of the matrix-pipe grouped kernel */ \
    X(table_window, "KN_TABLE_WINDOW", 0, true)      /* (0: the rule) */ \
    X(table_strip, "KN_TABLE_STRIP", -1, true)       /* (-1: best of the candidates, 0: keep the ball order) */ \
    X(no_patch, "KN_NO_PATCH", 0, true) \
    X(conv_ball, "KN_CONV_BALL", 64, true)           /* output pixels per breadth-first ball of a conv-taps operator's processing order */ \
    X(no_row_order, "KN_NO_ROW_ORDER", 0, true) \
    X(chain_no_cl, "KN_CHAIN_NO_CL", 0, true) \
    X(chain_no_rpl2, "KN_CHAIN_NO_RPL2", 0, true)    /* whole-net kernel: one output row per lane in the pattern walk */ \
    X(chain_no_early, "KN_CHAIN_NO_EARLY", 0, true)  /* whole-net kernel: column pools staged at the start of their own layer */ \
    X(chain_no_seq, "KN_CHAIN_NO_SEQ", 0, true)      /* whole-net kernel: thin layers read their columns from the staged pool instead of walking a re-ordered input sequentially */ \
    X(chain_no_share, "KN_CHAIN_NO_SHARE", 0, true)  /* whole-net kernel: every lane streams its own copy of its row's values (no shared value blocks) */ \
    X(narrow32_nv, "KN_NARROW32_NV", 0, true)        /* convtaps_narrow32_kernel: 8 | 16 | 32 columns per block (0: the rule, narrow_choice) */ \
    X(mfma64_mt, "KN_MFMA64_MT", 0, true)            /* 64-column f32 tiles (KN_FLAG_NARROW64_MFMA): 64 | 128 (| 256: no product form) output channels per tile (0: the rule, mfma64_choice) */ \
    X(fill_form, "KN_FILL_FORM", 0, true)            /* filled-in order-preserving kernel: 0 = the dispatch rule, 1 / 2 = 32 / 64 channels x one column tile, 3 / 4 = 32 / 64 channels x two tiles */ \
    X(abl, "KN_ABL", 0, true)                        /* kernel ablation mask (kn_conv.hip, KN_ABLATION code paths) */
struct Tuning {
#define KN_KNOB_FIELD(name, env, def, diag) int name = def;
    KN_TUNING_KNOBS(KN_KNOB_FIELD)
#undef KN_KNOB_FIELD
    std::string describe() const;   // "" when everything is at its default, else " opts{name=value,...}"
};
Tuning tuning_from_env();

enum Kind { KIND_CSR = 0, KIND_CONVTAPS = 1, KIND_DENSE = 2, KIND_CHAIN = 3, KIND_CSR64 = 4 };
struct ChainDev;   // kn_chain.hip

// What a grouped kernel is launched over: n (pattern group, first member row) pairs, each a chunk of member rows whose height is the kernel's own.  The kernels
// take the two arrays and the count as separate parameters.
struct WorkList {
    int32_t* grp = nullptr;
    int32_t* r0 = nullptr;
    int64_t n = 0;
};

// Order-preserving CSR resident in HBM.
struct CsrDev {
    Tuning tune;                 // recorded at create
    int64_t rows = 0, cols = 0, nnz = 0;
    int32_t* indptr = nullptr;   // [rows+1]
    int32_t* indices = nullptr;  // [nnz]  stored order
    float* data = nullptr;       // [nnz]
    double* data64 = nullptr;    // [nnz] values of a float64 operator (KIND_CSR64: kn_csr_create_f64); `data` and the group lists are unused then
    // pattern groups (rows sharing one column sequence, e.g. the Cout rows of one conv output pixel, or all rows of a
    // dense Linear): see kn_csr.hip.  Rows not in any group are listed in `loose_rows`.
    int64_t n_groups = 0;
    int32_t* grp_colptr = nullptr;   // [n_groups+1] into grp_cols
    int32_t* grp_cols = nullptr;     // shared column sequence of each group
    int32_t* grp_rowptr = nullptr;   // [n_groups+1] into grp_rows
    int32_t* grp_rows = nullptr;     // member rows
    int64_t* grp_valptr = nullptr;   // [n_groups+1] into grp_vals (layout [col j][member r], r padded to RB)
    float* grp_vals = nullptr;
    // work lists of the grouped kernels: see WorkList (cut in one place, csr_cut_work_lists in kn_csr.hip)
    WorkList work;                   // every group but the big ones, in bundles of RB rows
    // big groups (a keyed nn.Linear: thousands of member rows over thousands of shared columns) run in the LDS-staged kernel:
    // chunks of 32 rows; their members are NOT in `work`
    WorkList big;
    // loose rows with thousands of non-zeros (a row of a keyed nn.Linear whose pattern lost an entry to an exact zero): one wave per
    // (row, 64 batch columns) with a deep gather queue, as extra workgroups of the big-group launch
    int32_t* long_rows = nullptr;
    int64_t n_long = 0;
    int32_t* loose_rows = nullptr;
    int64_t n_loose = 0;
    int64_t loose_max = 0;           // stored entries of the longest loose row (long rows are not loose rows)
    int64_t grouped_nnz = 0;
    // the row-lane kernel for 1 .. 8 batch columns (kn_csr_narrow.hip, KN_FLAG_NARROW_ROWS): EVERY pattern group, the big ones included, in chunks of 64
    // member rows (a last chunk may be partly filled); grp_cols carries NARROW_ROWS_COL_PAD entries of padding for its look-ahead
    WorkList nr;
    // the value-stream kernel for 1 .. 32 batch columns (kn_csr_stream.hip: KN_FLAG_NARROW_LINEAR, narrow_linear_call): sg = the 64-row chunks of the BIG groups, nrs = those of every other
    // group (nr = both, in group order): what the row-lane kernel keeps next to it
    WorkList sg, nrs;
    // matrix-pipe products (kn_csr_mfma.hip): pattern groups with >= MF_MIN_MEMBERS members cut into chunks of 32 * (k + 1) member rows, k = 0..2
    // (list k holds the chunks of k + 1 row blocks); ws = the 16-row bundles of the REMAINING (small) groups for the vector-ALU kernels
    WorkList mf[3];
    int64_t mf_rows = 0;             // member rows covered by the mf lists
    int64_t mf_nnz = 0;              // their stored entries (mf_nnz / mf_rows = mean stored columns per row: the dispatch rule of csr_choice)
    WorkList mf16;                   // big pattern groups (a keyed Linear) in chunks of 16 member rows: csr_group_mfma16_kernel on narrow batches
    WorkList ws;
    // PATCHED group members: rows whose stored column sequence is a group's sequence minus a few entries (a keyed conv row that lost a weight to an
    // exact zero) ride in the group with 0.0f at the missing positions; csr_patch_guard_kernel recomputes them in the reference's own sequence for
    // the batch columns whose activation at a missing position is not finite (see kn_csr.hip)
    int32_t* patch_rows = nullptr;   // [n_patch]
    int32_t* patch_ptr = nullptr;    // [n_patch+1] into patch_cols
    int32_t* patch_cols = nullptr;   // the missing column indices
    int64_t n_patch = 0;
};

// Record layouts that a host-side packer writes and a kernel of kn_conv.hip reads.
// Small-K descriptor (convtaps_smallk_desc, kn_api.hip -> convtaps_smallk_pipe_kernel): per output pixel SK_DESC_HDR header dwords, then cout_pad bias values.  Header:
// [SK_DESC_XROW + k] X row of contraction row k (-1 = none), [SK_DESC_PIX] output pixel, [SK_DESC_TAPOFF + k] LDS offset of its tap row, [SK_DESC_COEF + k] coefficient,
// k < SMALLK_MAX.  The kernel reads a header with one dword per lane and section.
static constexpr int SMALLK_MAX = 28;        // contraction rows (slots x Cin + bias row) of the small-K kernels
static constexpr int SK_DESC_HDR = 96;
static constexpr int SK_DESC_XROW = 0, SK_DESC_PIX = 31, SK_DESC_TAPOFF = 32, SK_DESC_COEF = 64;
static constexpr int SK_TAB_MAX = 61;        // tap-table rows that fit the LDS budget (+1 zero row, +2 bias rows = 16 KiB)
static constexpr int SK_TAB_ROW = 64;        // floats per tap-table row: the one 64-channel tile of an eligible layer
// (output pixel, tap) record of the matrix-core narrow kernel (convtaps_build_pt, kn_api.hip -> convtaps_narrow_mfma_kernel)
struct PtRec {
    int32_t in0;       // input pixel of the first slot of this (output pixel, tap), or -1
    float c0;
    int32_t in1;       // ... of the second one, or -1
    float c1;
};
static_assert(sizeof(PtRec) == 16, "one 16-byte load per record");
// slot record of a filled-in operator (convtaps_fill_records_kernel -> convtaps_exact_fill_kernel)
struct FillRec {
    int32_t in, tapoff;     // tapoff: offset of the tap's plane in tapsT (floats), or the tap index (TREG)
    float coef;
    int32_t flags;          // bit 0: first slot of a stored column, bit 1: last
};

// Factored conv operator  W = sum_e coef_e * taps[tap_e] (x) E[out_e,in_e] + lastcol + e_last.
struct ConvTapsDev {
    Tuning tune;                        // recorded at create
    int64_t Cin = 0, Hin = 0, Win = 0, Cout = 0, Hout = 0, Wout = 0;
    int64_t ntaps = 0;
    int64_t cin_pad = 0, cout_pad = 0;  // padded dims of tapsT
    float* tapsT = nullptr;             // [ntaps][cin_pad][cout_pad]  (co contiguous; zero padded)
    int64_t nslots = 0;                 // compute entries (zero taps dropped)
    int32_t* pix_ptr = nullptr;         // [HoWo+1]
    int32_t* slot_in = nullptr;         // [nslots] input pixel
    int32_t* slot_tap = nullptr;        // [nslots]
    float* slot_coef = nullptr;         // [nslots]
    int32_t* pix_order = nullptr;       // [HoWo] processing order of output pixels (locality)
    int32_t* pix_deal = nullptr;        // [HoWo] the same order dealt to the 8 XCDs by slot weight, heavy pixels first (kn_deal.h): what the kernels that cut per-XCD chunks walk
    float* lastcol = nullptr;           // [Cout*HoWo+1] or null
    bool has_last = false;
    bool unit_coef = true;
    bool has_dups = false;              // some (output pixel, input pixel) pair is hit by more than one slot
    int max_slots = 0;
    // small-K pipeline (first layer of an image net: kn_conv.hip, convtaps_smallk_pipe_kernel): per-pixel descriptor records in
    // processing order, or null when the operator is not eligible
    int32_t* sk_desc = nullptr;
    int64_t sk_stride = 0, sk_tab_rows = 0;
    // kn_convtaps_drop_zero_entries: zero-valued tap entries (tap, co, ci) of taps that are not zero altogether -- absent from the reference's
    // untiled CSR; convtaps_zero_guard_kernel re-walks the affected output rows for batch columns with a non-finite activation there
    int32_t* zero_ent = nullptr;        // [n_zero][3]
    int64_t n_zero = 0;
    // ... and the stored-column table of the expansion (kn_csr_mfma.hip, TAPS): pixel o's columns ex_ptr[o] .. ex_ptr[o + 1], each (activation row, value row of tapsT)
    int32_t* ex_ptr = nullptr;          // [HoWo + 1]
    int32_t* ex_tab = nullptr;          // [ex_ptr[HoWo]][2]
    int32_t* ex_order = nullptr;        // [HoWo] processing order of the pixels for the table kernel (strips, kn_convtaps_drop_zero_entries)
    // filled-in operators under KN_FLAG_EXACT (kn_conv.hip, convtaps_exact_fill_kernel): per-pixel record lists {input pixel, tap offset, coefficient, first / last slot of
    // a stored column}, each padded to a multiple of 8 records; fill_ptr at create, the records on the device at the first kn_spmm that asks for them
    int32_t* fill_ptr = nullptr;        // [HoWo + 1] record offsets, or null when the operator is not eligible
    FillRec* fill_rec = nullptr;        // [fill_n]
    int64_t fill_n = 0;
    // bf16x3 path (kn_conv.hip, convtaps_bf16x3_kernel): the taps as three bf16 planes, built at the first kn_spmm that asks for them
    uint16_t* tapsB = nullptr;
    int64_t tapsB_plane = 0;
    // matrix-core path for 1 .. 8 columns (kn_conv.hip, convtaps_narrow_mfma_kernel): the slot lists seen per (output pixel, tap) -- 16-byte records
    // {input pixel, coefficient} x PT_MAX_SLOTS, -1 where a pair has fewer slots.  pt_ok at create (no pair holds more slots, the table stays small); the
    // records are built at the first kn_spmm that asks for them
    bool pt_ok = false;
    bool pt_two = false;                // some (pixel, tap) pair holds two slots
    PtRec* pt_rec = nullptr;            // [HoWo][ntaps]
};

}  // namespace kn

struct kn_operator {
    int kind = kn::KIND_CSR;
    int device = 0;
    int64_t rows = 0, cols = 0;
    int64_t nnz_stored = 0;     // what the reference's nnz() reports
    int64_t nnz_expanded = 0;   // nnz of tocsr()
    kn::CsrDev csr;
    kn::ConvTapsDev ct;
    // host description of a conv-taps operator (export, kn_convtaps_drop_zero_entries)
    std::vector<int32_t> h_ent_out, h_ent_in, h_ent_tap;
    std::vector<float> h_ent_coef, h_taps, h_last_vals;
    std::vector<int64_t> h_last_rows;   // with h_last_vals: the explicit entries of the last column (row, value), may hold explicit zeros
    std::vector<int32_t> h_pix_order;   // [HoWo] host copy of ConvTapsDev::pix_order
    std::mutex lazy_mu;
    // dense (Linear) operator: split-K conv-taps sub-operator + ordered reduction
    kn_operator* dense_sub = nullptr;
    int64_t dense_splits = 0;
    float* dense_lastcol = nullptr;   // [rows] bias column incl. the homogeneous 1
    // split-K partial sums [(rows-1) * splits, vecs]: ONE workspace PER STREAM (launches on one stream are ordered, launches on
    // different streams get different buffers, so concurrent kn_spmm calls on one handle never share partial sums).
    struct DenseWs {
        float* ptr = nullptr;
        int64_t vecs = 0;
    };
    std::map<hipStream_t, DenseWs> dense_ws;
    // an outgrown buffer is retired with an event recorded on its stream at that moment and freed by a later call once the event has
    // completed (every launch that could read it was queued before the event); kn_destroy frees what is left
    struct Retired {
        float* ptr = nullptr;
        hipEvent_t done = nullptr;
    };
    std::vector<Retired> dense_ws_retired;
    // a whole key-net of CSR operators as one launch (kn_chain.hip)
    kn::ChainDev* chain = nullptr;
    // KN_MODIFIER_WINO (kn_wino.h, kn_conv_wino.hip): the 1-D Winograd F(2,3) form of a keyed 3 x 3 conv, derived from the handle's host description at the first call that
    // asks (convtaps_build_wino under lazy_mu, kn_api.hip) and kept as a sub-operator like dense_sub: a conv-taps operator of 2 * HoWo pseudo output pixels over
    // 2 * HiWi pseudo input pixels and 12 taps, packed by the ordinary conv-taps packer.  wino_state: 0 not asked yet, 1 built, 2 the operator is not eligible (wino_why
    // says why; asked once).  kn_release_side_tables and kn_destroy free it.
    int wino_state = 0;
    std::string wino_why;
    kn_operator* wino_sub = nullptr;
    int32_t* wino_in = nullptr;       // [HiWi / 2][4] input pixels d0 .. d3 of an input pair (-1: outside the image): wino_in_kernel
    int32_t* wino_out = nullptr;      // [HoWo / 2][2] output pixels of an output pair: wino_out_kernel
};

namespace kn {
// kernels (kn_csr.hip / kn_conv.hip / kn_elementwise.hip)
int csr_build_groups(kn_operator* h, const int32_t* indptr, const int32_t* indices, const float* data);
int csr_spmm_planes(const CsrDev& A, const float* x, int64_t ldx, int64_t x_stride, int64_t n_planes, int64_t n_vecs, float* y, int64_t ldy, int64_t y_stride, uint32_t flags, hipStream_t s);
int csr_spmm(const CsrDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, uint32_t flags, hipStream_t s, float* absmax = nullptr,
             bool* absmax_fused = nullptr);
template <typename TOUT>
int csr_f64_spmm(const CsrDev& A, const float* x, int64_t ldx, int64_t n_vecs, TOUT* y, int64_t ldy, uint32_t flags, hipStream_t s);      // kn_csr_f64.hip
// the six group tables every grouped kernel takes, in the kernels' parameter order
#define KN_GROUP_TABLES(A) (A).grp_colptr, (A).grp_cols, (A).grp_rowptr, (A).grp_rows, (A).grp_valptr, (A).grp_vals
int csr_group_mfma_spmm(const CsrDev& A, const WorkList* mf, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, hipStream_t s);       // mf[0 .. 2]
int csr_group_mfma16_spmm(const CsrDev& A, const WorkList& chunks, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, hipStream_t s);
static constexpr int MF_MIN_MEMBERS = 24;   // a pattern group takes the matrix-pipe kernel when its members fill >= 3/4 of a 32-row block
// `absmax` (device float or null): when the launch takes a kernel whose epilogue can fold max |Y| into its stores, the slot is raised atomically
// and *absmax_fused is set; otherwise the caller runs absmax_pass over Y afterwards (kn_spmm_screen)
// KN_FLAG_NARROW: the widest batch of the channel-lane conv-taps kernel, and whether a call takes it (the one place that reads the flag)
static constexpr int64_t NARROW_MAX_VECS = 8;
// KN_FLAG_NARROW32, a modifier of the two flags above: their column range is 1 .. NARROW32_MAX_VECS instead (9 .. 32 columns: convtaps_narrow32_kernel, and the matrix-core
// kernel at NV = 16 | 32).  Alone, and on every handle kind but conv-taps, it changes nothing.  narrow_max is the one place that reads it.
static constexpr int64_t NARROW32_MAX_VECS = 32;
// KN_FLAG_NARROW64, a second modifier of the two flags: it opens the range NARROW32_MAX_VECS + 1 .. NARROW64_MAX_VECS (33 .. 64 columns: the order-preserving pipeline with one
// column per lane, ConvRegime NARROW64) and that range ALONE -- at 32 columns and fewer a call is what its other flags make it, KN_FLAG_NARROW32 included.  Without
// KN_FLAG_NARROW64_MFMA (narrow64_mfma_call below) KN_FLAG_NARROW_MFMA means KN_FLAG_NARROW at that width (narrow_mfma_call).  Read in narrow_max only: the widest batch a call of n_vecs columns may have.
static constexpr int64_t NARROW64_MAX_VECS = 64;
static inline int64_t narrow_max(uint32_t flags, int64_t n_vecs) {
    if ((flags & KN_FLAG_NARROW64) && n_vecs > NARROW32_MAX_VECS) return NARROW64_MAX_VECS;
    return (flags & KN_FLAG_NARROW32) ? NARROW32_MAX_VECS : NARROW_MAX_VECS;
}
static inline bool narrow_call(uint32_t flags, int64_t n_vecs) { return (flags & (KN_FLAG_NARROW | KN_FLAG_NARROW_MFMA)) && n_vecs <= narrow_max(flags, n_vecs); }
// The width a narrow launcher instantiates its kernel for: the next of 1 | 2 | 4 | 8 (| 16 | 32: KN_FLAG_NARROW32 calls only) columns, its log2, and whether the batch fills it
// (else the columns beyond n_vecs are masked)
struct NarrowWidth { int nv, log2; bool full; };
static inline NarrowWidth narrow_width(int64_t n_vecs) {
    const int l = n_vecs <= 1 ? 0 : (n_vecs <= 2 ? 1 : (n_vecs <= 4 ? 2 : (n_vecs <= 8 ? 3 : (n_vecs <= 16 ? 4 : 5))));
    return {1 << l, l, n_vecs == (1 << l)};
}
// KN_FLAG_NARROW_MFMA: the most slots one (output pixel, tap) pair may hold for the matrix-core narrow kernel, the largest record table built for it, and
// whether a narrow call takes that kernel (otherwise the flag means KN_FLAG_NARROW)
static constexpr int PT_MAX_SLOTS = 2;
static constexpr int64_t PT_MAX_RECORDS = (int64_t)1 << 22;
// The one SHAPE that stays on the channel-lane kernel (measured, profiles/r08_narrow_mfma.txt): a K unit of the matrix-core kernel is (one tap, 16 input
// channels), so with Cin <= 4 at least three quarters of its matrix instructions and value loads are padding, while the channel-lane kernel walks Cin
// channels only and carries 8 columns per lane for the price of one.  VGG-16 conv1_1 (Cin 3, 50 176 pixels): 0.73x at 5 .. 8 images (1.03x at 4, 1.25x
// at 2, 1.46x at 1).  Only where the channel-lane grid fills the chip (>= 1 024 workgroups of four (pixel, 64 channels) items); smaller layers were not
// measured slower and keep the kernel.
static inline bool narrow_mfma_loses(const ConvTapsDev& A, int64_t n_vecs) {
    return A.Cin <= 4 && n_vecs > 4 && A.Hout * A.Wout * ((A.Cout + 63) / 64) >= 4 * 1024;
}
static inline bool narrow_mfma_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_MFMA) && !(flags & KN_FLAG_EXACT) && n_vecs <= narrow_max(flags, n_vecs) && n_vecs <= NARROW32_MAX_VECS && A.pt_ok && !narrow_mfma_loses(A, n_vecs);
}
// KN_FLAG_NARROW_TAPS, a modifier of regime NARROW (conv_regime below: KN_FLAG_NARROW at 1 .. 8 columns, or KN_FLAG_NARROW_MFMA where that flag means KN_FLAG_NARROW): an
// ELIGIBLE operator runs convtaps_narrow_taps_kernel (kn_conv_narrow_taps.inc), bit for bit the channel-lane kernel's result.  Eligible, by what create recorded: no
// summed stored values, at most NARROW_TAPS_MAX_SLOTS slots per output pixel (a 3 x 3 window), 1 .. NARROW_TAPS_MAX_TAPS taps, with coefficients or without,
// value rows in whole 64-channel blocks.  Everywhere else -- alone, in every other regime, on an
// ineligible operator, on other handle kinds, in kn_spmm_planes -- the bit is not read.  narrow_taps_call is the one place that reads it; narrow_choice (kn_conv.hip)
// asks it and adds the per-call condition of the kernel's 32-bit byte offsets.
static constexpr int NARROW_TAPS_MAX_SLOTS = 9;
static constexpr int NARROW_TAPS_MAX_TAPS = 16;
static inline bool narrow_taps_ok(const ConvTapsDev& A) {
    return !A.has_dups && A.nslots > 0 && A.max_slots <= NARROW_TAPS_MAX_SLOTS && A.ntaps >= 1 && A.ntaps <= NARROW_TAPS_MAX_TAPS && A.cout_pad % 64 == 0;
}
// No shape or width is known to be slower than convtaps_narrow_kernel (profiles/r15_narrow_taps.txt); a measured one goes here, next to narrow_mfma_loses, from the kernel trace only
static inline bool narrow_taps_loses(const ConvTapsDev& A, int64_t n_vecs) { return false; }
static inline bool narrow_taps_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_TAPS) && n_vecs <= NARROW_MAX_VECS && narrow_taps_ok(A) && !narrow_taps_loses(A, n_vecs);
}
// KN_MODIFIER_NARROW_TAPS32, a modifier of KN_FLAG_NARROW_TAPS in regime NARROW32 (KN_FLAG_NARROW | KN_FLAG_NARROW32 at 9 .. 32 columns, or KN_FLAG_NARROW_MFMA where that
// flag means KN_FLAG_NARROW): an operator eligible for KN_FLAG_NARROW_TAPS (narrow_taps_ok) runs convtaps_narrow_taps32_kernel (kn_conv_narrow_taps32.inc) when the call
// carries BOTH bits, bit for bit convtaps_narrow32_kernel's result.  Everywhere else -- without KN_FLAG_NARROW_TAPS, in every other regime, at 8 columns or fewer, beyond
// 32, on an ineligible operator, on other handle kinds, in kn_spmm_planes, where KN_FLAG_NARROW_FILL takes the launch -- the bit is not read.  narrow_taps32_call is the one
// place that reads it; narrow_choice (kn_conv.hip) asks it and adds the per-call condition of the kernel's 32-bit byte offsets and whether the form is built.
// narrow_taps32_loses: the (shape, width) pairs whose launch is slower than convtaps_narrow32_kernel's in a kernel trace, each with its trace line.  None: of the 13 conv
// launches of keyed VGG-16 the slowest ratios are conv1_1 1.59x at 16 images and conv4_3 1.01x (3 468.4 -> 3 422.7 us) at 32 (profiles/r17_narrow_taps32.txt).
static inline bool narrow_taps32_loses(const ConvTapsDev& A, int64_t n_vecs) { return false; }
static inline bool narrow_taps32_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_TAPS) && (flags & KN_MODIFIER_NARROW_TAPS32) && n_vecs > NARROW_MAX_VECS && n_vecs <= NARROW32_MAX_VECS && narrow_taps_ok(A) &&
           !narrow_taps32_loses(A, n_vecs);
}
// KN_MODIFIER_NARROW_TAPS_PAIRS, a modifier of KN_FLAG_NARROW_TAPS in regime NARROW (1 .. 8 columns): an operator eligible for KN_FLAG_NARROW_TAPS (narrow_taps_ok) with more
// than 64 output channels runs convtaps_narrow_taps_pairs_kernel (kn_conv_narrow_taps_pairs.inc: two output channels per lane, packed f32) when the call carries BOTH
// bits, bit for bit convtaps_narrow_taps_kernel's result.  Everywhere else -- without KN_FLAG_NARROW_TAPS, beyond 8 columns, in regime NARROW_MFMA, where
// KN_FLAG_NARROW_FILL takes the launch, on operators of 64 output channels or fewer, on an ineligible operator, on other handle kinds, in kn_spmm_planes -- the bit is not
// read.  narrow_taps_pairs_call is the one place that reads it; narrow_choice (kn_conv.hip) asks it behind narrow_taps_call and the per-call offset condition, and adds
// whether the form is built.
// narrow_taps_pairs_loses: the (shape, width) pairs whose launch is not faster than convtaps_narrow_taps_kernel's in a kernel trace by more than the two min .. max
// spreads added (profiles/r18_narrow_taps_pairs.txt: keyed VGG-16, three launches a side, medians in us).  The kernel halves the instructions per channel AND the
// wavefronts of a launch; what it loses is shapes whose 128-channel blocks x pixels leave the 1 024 SIMDs few wavefronts each, the more so the shorter a step (NV):
//   conv5_x (512 -> 512 channels, 196 pixels: 784 wavefronts), every width:    1 image 207.1 -> 309.9, 2: 221.5 -> 337.8, 4: 277.8 -> 387.2, 8: 494.6 -> 568.2
//   conv4_x (256 | 512 -> 512, 784 pixels: 3 136 wavefronts), NV <= 4:         1 image 406.9 -> 428.1 (conv4_1 211.3 -> 219.2), 2: 410.4 -> 465.5, 4: 545.4 -> 651.9;
//                                                                              NV = 8 wins (1 214.9 -> 974.7)
//   conv3_x (128 | 256 -> 256, 3 136 pixels: 6 272 wavefronts), NV = 4:        278.7 -> 282.5, 567.2 -> 559.2, 572.1 -> 553.8 (gains inside the spreads);
//                                                                              NV = 1 | 2 | 8 win (1.07 - 1.32x)
//   conv2_x (64 | 128 -> 128, 12 544 pixels: 12 544 wavefronts) wins at every width (1.18 - 1.43x).
// The thresholds are the next powers of two above the measured counts.  Only operators of 128 input channels and more are listed: every measured shape has them, and
// a shorter channel loop (the operators of the tests, first layers) is not measured -- it stays on the kernel the caller asked for.  Widths 3, 5, 6, 7 take the row
// of the form they run (NV = 4, NV = 8, masked); not traced.
static inline bool narrow_taps_pairs_loses(const ConvTapsDev& A, int64_t n_vecs) {
    if (A.Cin < 128) return false;
    const int64_t waves = A.Hout * A.Wout * ((A.Cout + 127) / 128);
    const int nv = n_vecs <= 1 ? 1 : (n_vecs <= 2 ? 2 : (n_vecs <= 4 ? 4 : 8));
    return waves < 1024 || (waves < 4096 && nv <= 4) || (waves < 8192 && nv == 4);
}
static inline bool narrow_taps_pairs_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_TAPS) && (flags & KN_MODIFIER_NARROW_TAPS_PAIRS) && n_vecs <= NARROW_MAX_VECS && narrow_taps_ok(A) && A.Cout > 64 &&
           !narrow_taps_pairs_loses(A, n_vecs);
}
// KN_FLAG_NARROW_FILL, a modifier of regimes NARROW and NARROW32 (KN_FLAG_NARROW [| KN_FLAG_NARROW32] at 1 .. 32 columns, or KN_FLAG_NARROW_MFMA where that flag means
// KN_FLAG_NARROW): an ELIGIBLE operator runs convtaps_narrow_fill_kernel (kn_conv_narrow_fill.inc), bit for bit the channel-lane kernels' result.  Eligible: the handle has
// the record lists of the filled-in order-preserving kernel (convtaps_fill_ok: summed stored values, or more than 64 slots on some output pixel), 1 .. 16 taps (the records
// then hold tap indices, and a channel's value rows fit 16 registers), value rows in whole 64-channel blocks.
// narrow_fill_ok and narrow_taps_ok cannot both hold for one operator: the first needs has_dups or max_slots > 64 (what convtaps_fill_offsets lays lists out for), the
// second !has_dups and max_slots <= 9.  Everywhere else -- alone, in every other regime, on an ineligible operator, on other handle kinds, in kn_spmm_planes -- the bit is
// not read.  narrow_fill_call is the one place that reads it; narrow_choice (kn_conv.hip) asks it and adds the per-call conditions (32-bit byte offsets, records built);
// spmm_impl (kn_api.hip) asks it whether the call builds the records.
bool convtaps_fill_ok(const ConvTapsDev& A);      // kn_conv.hip
static constexpr int NARROW_FILL_MAX_TAPS = 16;
static inline bool narrow_fill_ok(const ConvTapsDev& A) { return convtaps_fill_ok(A) && A.ntaps >= 1 && A.ntaps <= NARROW_FILL_MAX_TAPS && A.cout_pad % 64 == 0; }
// The (shape, width) pairs where convtaps_narrow_fill_kernel does not beat the kernel the call runs without the bit by more than the boxes' 3 % spread: none.  Measured
// (profiles/r16_narrow_fill.txt; filled-in operators of the VGG-16 shapes, same process, gain over convtaps_narrow_kernel / convtaps_narrow32_kernel at 1 / 8 / 16 / 32 images):
// conv1_2 2.89x / 2.48x / 1.66x / 1.71x, conv2_1 3.00x / 2.38x / 1.64x / 1.61x, conv3_1 2.93x / 2.03x / 1.53x / 1.50x, conv4_1 2.68x / 1.70x / 1.30x / 1.25x,
// conv5_x 1.82x / 1.64x / 1.54x / 1.30x.  (Against the PADDED 128-column launch the deep layers lose from 16 images on -- DESIGN.md 8 -- which is the caller's choice of call, not this rule's.)
static inline bool narrow_fill_loses(const ConvTapsDev& A, int64_t n_vecs) { return false; }
static inline bool narrow_fill_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_FILL) && n_vecs <= NARROW32_MAX_VECS && narrow_fill_ok(A) && !narrow_fill_loses(A, n_vecs);
}
// The regime a call on a conv-taps handle takes: the one place that turns the flag word into one.  convtaps_spmm switches on it, kn_spmm asks it which side table
// the call reads.  BF16X3 is the REQUEST (its planes are built for it): operands that do not qualify run as MFMA (mfma_choice, kn_conv.hip).
// NARROW64 is the order-preserving product under every contract flag, launched by the order-preserving launcher (spmm_exact): an operator without the pipeline's shape
// runs what EXACT runs at that width, so the regime never refuses.
// MFMA64 (KN_FLAG_NARROW64_MFMA next to KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW64, without KN_FLAG_EXACT, at 33 .. 64 columns and there alone): the f32 tile product of MFMA on
// 64-column tiles (mfma64_choice, kn_conv.hip); KN_FLAG_BF16X3 next to it changes nothing.  In every other situation the bit is not read.
enum ConvRegime { NARROW_MFMA, NARROW, NARROW32, NARROW64, EXACT, BF16X3, MFMA, MFMA64 };
static inline bool narrow64_mfma_call(uint32_t flags, int64_t n_vecs) {
    const uint32_t all = KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW64 | KN_FLAG_NARROW64_MFMA;
    return (flags & all) == all && !(flags & KN_FLAG_EXACT) && n_vecs > NARROW32_MAX_VECS && n_vecs <= NARROW64_MAX_VECS;
}
static inline ConvRegime conv_regime(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs) {
    if (narrow_mfma_call(A, flags, n_vecs)) return NARROW_MFMA;
    if (narrow64_mfma_call(flags, n_vecs)) return MFMA64;
    if (narrow_call(flags, n_vecs))                                                            // (beyond 8 columns KN_FLAG_NARROW32 is in force, beyond 32 KN_FLAG_NARROW64)
        return n_vecs > NARROW32_MAX_VECS ? NARROW64 : (n_vecs > NARROW_MAX_VECS ? NARROW32 : NARROW);
    if (flags & KN_FLAG_EXACT) return EXACT;
    return (flags & KN_FLAG_BF16X3) ? BF16X3 : MFMA;
}
// KN_FLAG_NARROW_ROWS: an f32 CSR operator's pattern groups and loose rows on the row-lane kernel (kn_csr_narrow.hip) for at most NARROW_MAX_VECS columns, while the
// kernel's 32-bit BYTE offsets into X hold; else the flag is ignored (the other kernels give the same bits).  The one place that reads the flag.
static constexpr int NARROW_ROWS_COL_PAD = 80;
// The SHAPES that stay on the existing kernels (measured, profiles/r09_narrow_rows.txt): an operator with BIG pattern groups -- a keyed Linear, >= 256 rows over >= 2 048
// shared columns -- at more than two columns.  Its wavefronts sit alone on their SIMDs, the bytes in flight are bounded by the 48-step value rings, and each step's
// activations are a scalar-cache round trip that only 16 / NV steps of arithmetic cover, while csr_big_group_kernel carries 64 columns per lane for the price of one.
// Inside a VGG-16 forward (kernel trace, values cold): fc6 1.91x at 1 image and 1.42x at 2; fc7 1.86x / 1.39x, fc8 1.78x / 1.33x; at 4 images fc7 0.94x and fc8 0.91x
// (alone on a warm block 1.19x / 1.12x: not what a forward sees); alone: fc6 0.88x at 4 and 0.47x at 8, fc7 / fc8 0.95x / 0.93x at 3 (masked form) and 0.67x / 0.65x at 8.
// Operators without big groups (pools: 1.46x .. 5.1x at every width 1 .. 8; conv-like groups: not measured) keep the kernel.
static inline bool narrow_rows_loses(const CsrDev& A, int64_t n_vecs) { return A.big.n > 0 && n_vecs > 2; }
static inline bool narrow_rows_call(const CsrDev& A, uint32_t flags, int64_t n_vecs, int64_t ldx) {
    return (flags & KN_FLAG_NARROW_ROWS) && n_vecs <= NARROW_MAX_VECS && A.cols * ldx + NARROW_MAX_VECS < ((int64_t)1 << 30) && !narrow_rows_loses(A, n_vecs);
}
// Loose rows take a LANE each in that kernel, which walks a row with two dependent loads per four entries and nothing else in flight: right for pools and
// homogeneous rows (a handful of entries), wrong for a long ragged row, which csr_rows_kernel walks 64 entries at a time with a whole wavefront.  An operator
// whose longest loose row holds more entries than this keeps csr_rows_kernel for its loose rows (its pattern groups still take the row-lane kernel).
static constexpr int64_t NARROW_ROWS_LOOSE_MAX = 64;
static inline bool narrow_rows_loose(const CsrDev& A) { return A.loose_max <= NARROW_ROWS_LOOSE_MAX; }
int csr_narrow_rows_spmm(const CsrDev& A, const WorkList& groups, const int32_t* loose_rows, int64_t n_loose, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu,
                         hipStream_t s);      // kn_csr_narrow.hip
// KN_FLAG_NARROW_LINEAR: an f32 CSR operator's BIG pattern groups (a keyed Linear) on the value-stream kernel (kn_csr_stream.hip) for at most NARROW64_MAX_VECS columns,
// where the handle rule below does not keep the kernel they have; else the flag is ignored (the other kernels give the same bits).  Everything else the operator holds runs what the call's other flags make it.  The kernel forms
// every address in 64 bits: no condition on ldx.  The one place that reads the flag.
// The form of a width (at most STREAM_MAX_VECS columns): W wavefronts x NV running sums per lane, W * NV >= n_vecs, the fewest sums per lane that 8 wavefronts allow (a keyed Linear puts one workgroup
// on a CU -- VGG-16 fc6: 65 chunks on 256 CUs -- so a further wavefront costs nothing but its share of the issue slots, it takes its share of the fills, and every
// wavefront pays two LDS reads per step whatever its NV).  Chosen on the instruction counts of the compiled loop; the neighbouring forms of a width were not measured
// against it.
struct StreamForm { int w, nv; bool full; };
static inline StreamForm stream_form(int64_t n_vecs) {
    const int nv = n_vecs <= 8 ? 1 : (n_vecs <= 16 ? 2 : 4);
    const int64_t per = (n_vecs + nv - 1) / nv;
    const int w = per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : 8));
    return {w, nv, n_vecs == (int64_t)w * nv};
}
// Its ring: slots of one 16-step slab -- 16 x 256 bytes of values, 16 x cw activations (cw = W * NV; at least 256 bytes), 64 column indices -- as many as 64 KB of static
// LDS hold, at most 11; all but STREAM_SPARE_SLOTS of them in flight: 32 KB of values up to 16 columns, 28 KB (next to 14 KB of activations) at 32.
static constexpr int STREAM_SLAB_STEPS = 16, STREAM_SPARE_SLOTS = 3, STREAM_MAX_SLOTS = 11;
static constexpr int stream_slot_bytes(int cw) { return STREAM_SLAB_STEPS * 256 + (STREAM_SLAB_STEPS * cw * 4 < 256 ? 256 : STREAM_SLAB_STEPS * cw * 4) + 256; }
static constexpr int stream_ring_slots(int cw) { return 64 * 1024 / stream_slot_bytes(cw) < STREAM_MAX_SLOTS ? 64 * 1024 / stream_slot_bytes(cw) : STREAM_MAX_SLOTS; }
// The WIDTHS that stay on the kernels they have (measured, profiles/r13_narrow_linear.txt): a big-group operator beyond 32 columns.  The form built for them -- W = 8,
// NV = 8, where 64 KB of LDS hold 7 slots: 16 KB of values in flight next to 16 KB of activations -- issued 8 packed multiplies and adds and five LDS reads per step and
// wavefront, two wavefronts to a SIMD, and measured 0.69x of csr_big_group_kernel (which carries 64 columns per lane for the price of one) on VGG-16's fc6 at 33 and at 64
// columns (2 412 us against 1 671, values cold), 0.70x on fc7 and fc8 (407 / 402 us against 285 / 282); up to 32 columns the kernel measured 1.27x .. 3.59x on all three
// (fc6: 489 us at 1 column, 599 at 8, 880 at 16, 1 300 at 32, against 1 670 .. 1 684).  That form is not instantiated.
static constexpr int64_t STREAM_MAX_VECS = 32;
static inline bool narrow_linear_loses(const CsrDev& A, int64_t n_vecs) { return A.big.n > 0 && n_vecs > STREAM_MAX_VECS; }
static inline bool narrow_linear_call(const CsrDev& A, uint32_t flags, int64_t n_vecs) {
    return (flags & KN_FLAG_NARROW_LINEAR) && A.big.n > 0 && n_vecs <= NARROW64_MAX_VECS && !narrow_linear_loses(A, n_vecs);
}
int csr_stream_group_spmm(const CsrDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, hipStream_t s);      // kn_csr_stream.hip
int convtaps_spmm(const ConvTapsDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy,
                  uint32_t flags, hipStream_t s, float* absmax = nullptr, bool* absmax_fused = nullptr);
int absmax_pass(const float* y, int64_t rows, int64_t ld, int64_t n_vecs, float* absmax, hipStream_t s);
// the homogeneous row of a conv-taps operator's output on its own (kn_conv.hip, conv_lastrow_kernel), for a launcher outside that file
int convtaps_lastrow(const ConvTapsDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, float* absmax, hipStream_t s);
// KN_MODIFIER_WINO, a modifier of a plain kn_spmm (regimes MFMA and BF16X3: without KN_FLAG_EXACT and outside the narrow ranges) on a conv-taps handle: whole 128-column
// tiles of 16-byte aligned blocks on an eligible operator run the 1-D Winograd form -- wino_in_kernel, the derived operator's matrix-core launch, wino_out_kernel.  In
// every other case the bit is not read.  wino_call is the one place that reads it (the operands' half; eligibility is the handle's wino_state).
static inline bool wino_call(const ConvTapsDev& A, uint32_t flags, int64_t n_vecs, const float* x, int64_t ldx, const float* y, int64_t ldy) {
    if (!(flags & KN_MODIFIER_WINO) || n_vecs <= 0 || n_vecs % 128 != 0 || ldx % 4 != 0 || ldy % 4 != 0 || ((uintptr_t)x) % 16 != 0 || ((uintptr_t)y) % 16 != 0) return false;
    const ConvRegime r = conv_regime(A, flags, n_vecs);
    return r == MFMA || r == BF16X3;
}
int convtaps_build_wino(kn_operator* h);      // kn_api.hip (it reads the host description of the handle); the caller holds lazy_mu
void wino_free(kn_operator* h);               // kn_api.hip
int wino_spmm(const kn_operator* h, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, uint32_t flags, hipStream_t s, float* absmax);      // kn_conv_wino.hip
// the V and M blocks of a call: 2 * (Cin * HiWi + Cout * HoWo) * n_vecs floats from ONE pool per (device, stream), shared by all handles and grown to the largest request
int64_t wino_workspace_floats(const kn_operator* h, int64_t n_vecs);
int wino_workspace(int device, hipStream_t s, int64_t floats, float** out);
struct MfTaps;
int convtaps_exact_table_spmm(const ConvTapsDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, hipStream_t s);

// Raise *slot (a non-negative f32 kept as its bit pattern: for such values unsigned order == float order) to the wavefront's max of `m`.
// The slot is READ first and the atomic issued only when it would raise it -- after the first few tiles of a launch almost never.  Both
// alternatives were measured on the keyed VGG-16 forward (tools/ab_rescreen.py): an unconditional fire-and-forget atomic per tile (atomics on
// ONE address serialise at ~50 ns each: +20 ms per forward) and a scalar GLC load as the filter (same-address scalar loads serialise even
// harder: +54 ms).  The vector load's wait (vmcnt) also drains the wavefront's own stores, which is free where a workgroup ends with its tile
// and costly in the persistent first-layer kernel: that one carries its maximum across its pixels and commits once (kn_store_tile's `carry`).
__device__ __forceinline__ void kn_wave_absmax_commit(float m, float* slot, int lane) {
    auto step = [&](auto ctrl, auto row_mask) {               // DPP row shifts / broadcasts: vector ALU only, no LDS permute
        const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, m), __builtin_bit_cast(int, m), decltype(ctrl)::value,
                                                                              decltype(row_mask)::value, 0xf, false));
        m = (o > m) ? o : m;
    };
    step(std::integral_constant<int, 0x111>(), std::integral_constant<int, 0xf>());     // row_shr:1   lane i <- max(i, i-1)       (lanes without a source keep their own value)
    step(std::integral_constant<int, 0x112>(), std::integral_constant<int, 0xf>());     // row_shr:2
    step(std::integral_constant<int, 0x114>(), std::integral_constant<int, 0xf>());     // row_shr:4
    step(std::integral_constant<int, 0x118>(), std::integral_constant<int, 0xf>());     // row_shr:8   lane 15 of each row of 16 = the row's max
    step(std::integral_constant<int, 0x142>(), std::integral_constant<int, 0xa>());     // row_bcast:15 into rows 1, 3
    step(std::integral_constant<int, 0x143>(), std::integral_constant<int, 0xc>());     // row_bcast:31 into rows 2, 3: lane 63 = the wavefront's max
    if (lane == 63) {
        const unsigned bits = __float_as_uint(m);
        unsigned* u = reinterpret_cast<unsigned*>(slot);
        if (bits > __atomic_load_n(u, __ATOMIC_RELAXED)) atomicMax(u, bits);
    }
}
int relu_inplace(float* y, int64_t rows, int64_t ld, int64_t n_vecs, hipStream_t s);
int dense_reduce(const float* z, int64_t ldz, int64_t outs, int64_t splits, const float* lastcol, const float* xlast, float* y, int64_t ldy, int64_t n_vecs,
                 int relu, hipStream_t s);
int affine_to_linear(const float* x, int64_t n, int64_t d, float* out, int64_t ldo, hipStream_t s);
int u8_to_linear(const uint8_t* img, int64_t n, int64_t c, int64_t h, int64_t w, int layout, float* out, int64_t ldo, int64_t n_cols, hipStream_t s);
int linear_to_u8(const float* x, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* gain, const float* bias, uint8_t* img, hipStream_t s);
int frames_to_linear(const void* img, int depth, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* scale, const float* offset, float* out, int64_t ldo,
                     int64_t n_cols, hipStream_t s);
int linear_to_u16(const float* x, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* gain, const float* bias, uint16_t* img, hipStream_t s);
int column_range(const float* x, int64_t rows, int64_t ld, int64_t n_vecs, float* lo, float* hi, hipStream_t s);
int linear_to_affine(const float* y, int64_t ldy, int64_t n, int64_t d, float* out, float* maxdev, hipStream_t s);
int planes_to_columns(const float* in, int64_t plane_stride, int64_t ld, int64_t planes, int64_t rows, int64_t n_vecs, float* out, int64_t ld_out, hipStream_t s);
int columns_to_planes(const float* in, int64_t ld_in, int64_t planes, int64_t rows, int64_t n_vecs, float* out, int64_t plane_stride, int64_t ld, hipStream_t s);
// Processing order for rows of a sparse pattern (host): breadth-first balls of `patch` rows over "shares a column", seeded along
// a global breadth-first sweep.  Columns referenced by more than `max_degree` of the rows (a bias column) do not link rows.
std::vector<int32_t> locality_order(const std::vector<int32_t>& row_ids, const int32_t* indptr, const int32_t* indices, int64_t n_cols, int patch,
                                    int max_degree);
// Column patterns of a CSR (host): rows with an identical stored column sequence share one id, numbered in order of first appearance.  pat[r] = the id of row r,
// pat_rep[id] = the first row that carries it.  Empty rows share one id when `empty_rows` (the whole-net packer), else they get none (pat[r] = -1: the CSR packer
// leaves them loose).
void row_patterns(int64_t rows, const int32_t* indptr, const int32_t* indices, bool empty_rows, std::vector<int32_t>& pat, std::vector<int32_t>& pat_rep);
int chain_create(int64_t n_ops, kn_operator* const* ops, const uint32_t* flags, ChainDev** out, int64_t* rows_out, int64_t* cols_out, int64_t* nnz_out);
int chain_forward(const ChainDev* c, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, hipStream_t s);
void chain_free(ChainDev* c);
int convtaps_build_bf16(ConvTapsDev& A, const std::vector<float>& taps);
int convtaps_build_fill(ConvTapsDev& A, hipStream_t s);
int convtaps_build_pt(kn_operator* h);      // kn_api.hip (it reads the host description of the handle)
bool convtaps_fill_ok(const ConvTapsDev& A);
void csr_free(CsrDev& c);
void convtaps_free(ConvTapsDev& c);

template <typename T>
inline int upload(T** dptr, const T* h, size_t n) {
    *dptr = nullptr;
    const size_t n_copy = n;   // an empty host array has nothing to read, even when its pointer is non-null
    if (n == 0) n = 1;         // keep device pointers non-null
    hipError_t e = hipMalloc((void**)dptr, n * sizeof(T));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? KN_ERR_NOMEM : KN_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    if (n_copy == 0) {
        e = hipMemset(*dptr, 0, n * sizeof(T));
        if (e != hipSuccess) return fail(KN_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    } else if (h) {
        e = hipMemcpy(*dptr, h, n_copy * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(KN_ERR_HIP, std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
    }
    return KN_OK;
}
}  // namespace kn
