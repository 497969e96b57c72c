// kn_csr_narrow.hip -- order-preserving CSR product for 1 .. 8 batch columns (KN_FLAG_NARROW_ROWS): lanes are OUTPUT ROWS.
//
// The kernels of kn_csr.hip give a lane batch columns, so one image fills one lane in 64.  Here the lane is the output row and its NV (1 | 2 | 4 | 8)
// running sums are the batch columns; widths between the forms run the next NV, the surplus sums re-read the last real column and store nothing
// (convtaps_narrow_kernel's convention, kn_conv.hip).  The arithmetic is csr_group_kernel's / csr_rows_kernel's statement for statement: per output
// element a strictly serial walk over the stored columns, p = a * x; acc = acc + p, separately rounded, then ReLU -- bit-equal to those kernels and to
// scipy's csr_matvecs.  The walk over the columns is never split across lanes or wavefronts.  One launch, two roles:
//   * grouped rows (blocks below grid_grp): a wavefront owns 64 member rows of one pattern group.  grp_vals is [column j][member row]: the
//     values of a step are ONE coalesced segment (256 bytes at 64 rows), requested RING = 48 steps ahead of the add that consumes them (a ring of 48
//     vector registers: a keyed Linear puts about one wavefront on a SIMD, so the cover has to come from inside the wavefront).  The column index and
//     the NV activations of a step are wave-uniform and arrive through the scalar data cache in batches of SB steps, one batch ahead of the
//     arithmetic (scalar loads return out of order: the wait that opens a batch drains the requests made one batch earlier, never its own).
//     Rows beyond the member count ride on the rpad padding (zeros) and store nothing.
//   * loose rows (the remaining blocks): lane = row, each lane walks its own indptr range, four entries per trip; a wavefront loops to its longest
//     row under the execution mask.  Rows may be empty (they store 0) and may repeat a column.
// No LDS, no barriers, no atomics, no workspace.  Element offsets into X are 32-bit BYTE offsets (checked by narrow_rows_call, kn_internal.h), rows of Y
// are formed in 64 bits.
#include "kn_internal.h"
#include <type_traits>

#pragma clang fp contract(off)

namespace kn {

struct NarrowRowsArgs {
    int64_t n_items;                 // 64-row chunks of the pattern groups: (group, first member)
    const int32_t* nr_grp;
    const int32_t* nr_r0;
    const int32_t* grp_colptr;
    const int32_t* grp_cols;         // (padded by NARROW_ROWS_COL_PAD entries: the look-ahead of a group's last steps reads past its sequence)
    const int32_t* grp_rowptr;
    const int32_t* grp_rows;
    const int64_t* grp_valptr;
    const float* grp_vals;
    int64_t n_loose;
    const int32_t* loose_rows;
    const int32_t* indptr;
    const int32_t* indices;
    const float* data;
    const float* X;
    float* Y;
    int64_t ldy;
    uint32_t ldx4;                   // ldx in bytes
    int n_vecs;
    int relu;
    uint32_t grid_grp;               // blocks of the grouped role
};

static constexpr int NR_RING = 48;   // value rows in flight per wavefront

template <int NV, bool FULL>
__global__ __launch_bounds__(256) void csr_narrow_kernel(NarrowRowsArgs p) {
    constexpr int SB = NV == 1 ? 16 : (NV == 2 ? 8 : (NV == 4 ? 4 : 2));       // steps per scalar batch: 2 * SB * (NV + 1) scalar registers
    static_assert(NR_RING % SB == 0 && 2 * SB <= NARROW_ROWS_COL_PAD - NR_RING, "look-ahead of the scalar batches");
    const int lane = threadIdx.x & 63;
    int vcol[NV];                                           // column a running sum reads (surplus sums of a width below NV: the last real column)
#pragma unroll
    for (int v = 0; v < NV; v++) vcol[v] = (FULL || v < p.n_vecs) ? v : p.n_vecs - 1;
    const char* const Xb = reinterpret_cast<const char*>(p.X);
    auto xload = [&](float (&d)[NV], const uint32_t off4) {          // the NV activations of the row at byte offset off4 (one wide load when the width fills the form)
        const float* const xp = reinterpret_cast<const float*>(Xb + off4);
#pragma unroll
        for (int v = 0; v < NV; v++) d[v] = FULL ? xp[v] : xp[vcol[v]];
    };

    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = 0.0f;
    int64_t row = -1;                                       // the row this lane stores (none)

    if (blockIdx.x >= p.grid_grp) {
        // ---- loose rows ----------------------------------------------------------------------------------------------------------------------
        const int64_t ri = (int64_t)(blockIdx.x - p.grid_grp) * 256 + threadIdx.x;
        if (ri < p.n_loose) {
            row = p.loose_rows[ri];
            int k = p.indptr[row];
            const int end = p.indptr[row + 1];
            for (; k + 4 <= end; k += 4) {
                uint32_t xo[4];
                float a[4], x[4][NV];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    xo[u] = (uint32_t)p.indices[k + u] * p.ldx4;
                    a[u] = p.data[k + u];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) xload(x[u], xo[u]);
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        const float pr = a[u] * x[u][v];
                        acc[v] = acc[v] + pr;
                    }
            }
            for (; k < end; k++) {
                const float a = p.data[k];
                float x[NV];
                xload(x, (uint32_t)p.indices[k] * p.ldx4);
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float pr = a * x[v];
                    acc[v] = acc[v] + pr;
                }
            }
        }
    } else {
        // ---- grouped rows --------------------------------------------------------------------------------------------------------------------
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int64_t w = (int64_t)blockIdx.x * 4 + wave;
        const int64_t e = w;
        if (e >= p.n_items) return;                         // (wave-uniform; no barriers in this kernel)
        const int g = __builtin_amdgcn_readfirstlane(p.nr_grp[e]);
        const int r0 = __builtin_amdgcn_readfirstlane(p.nr_r0[e]);
        const int cbeg = __builtin_amdgcn_readfirstlane(p.grp_colptr[g]);
        const int ncol = __builtin_amdgcn_readfirstlane(p.grp_colptr[g + 1]) - cbeg;
        const int rbeg = __builtin_amdgcn_readfirstlane(p.grp_rowptr[g]);
        const int nmem = __builtin_amdgcn_readfirstlane(p.grp_rowptr[g + 1]) - rbeg;
        const int rpad = (nmem + 15) / 16 * 16;
        if (r0 >= nmem || ncol <= 0) return;
        const int m = r0 + lane;
        const int lrow = m < rpad ? m : rpad - 1;           // lanes beyond the padded member count re-read its last row (and store nothing)
        const float* const vals = p.grp_vals + p.grp_valptr[g];
        const int32_t* const cols = p.grp_cols + cbeg;

        float ring[NR_RING];                                // ring[u]: the lane's value of step q + u, then of step q + NR_RING + u
#pragma unroll
        for (int u = 0; u < NR_RING; u++) ring[u] = 0.0f;
        const float* vp = vals + lrow;                      // the lane's value of the next step to request
#pragma unroll
        for (int u = 0; u < NR_RING; u++) {
            if (u < ncol) ring[u] = *vp;
            vp += rpad;
        }

        float xc[SB][NV];                                   // activations of the scalar batch the arithmetic is at
        int cn[SB];                                         // column indices of the batch after it
        {
            int c0[SB];
#pragma unroll
            for (int i = 0; i < SB; i++) c0[i] = cols[i];
#pragma unroll
            for (int i = 0; i < SB; i++) xload(xc[i], (uint32_t)c0[i] * p.ldx4);
#pragma unroll
            for (int i = 0; i < SB; i++) cn[i] = cols[SB + i];
        }

        // one round = NR_RING steps from step q on, in scalar batches of SB steps.  TAIL: the rounds whose look-ahead may pass the end of the sequence
        // (value rows beyond it are not requested, steps beyond it not added; the scalar look-ahead reads the padding of grp_cols and row 0 .. of X)
        auto round = [&](const int q, auto tail) {
            constexpr bool TAIL = decltype(tail)::value;
#pragma unroll
            for (int b = 0; b < NR_RING / SB; b++) {
                const int qb = q + b * SB;
                if (TAIL && qb >= ncol) break;
                float xn[SB][NV];
                int cf[SB];
#pragma unroll
                for (int i = 0; i < SB; i++) xload(xn[i], (uint32_t)cn[i] * p.ldx4);
#pragma unroll
                for (int i = 0; i < SB; i++) cf[i] = cols[qb + 2 * SB + i];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < SB; i++) {
                    const int u = b * SB + i;
                    if (TAIL && qb + i >= ncol) break;
                    const float a = ring[u];
#pragma unroll
                    for (int v = 0; v < NV; v++) {
                        const float pr = a * xc[i][v];
                        acc[v] = acc[v] + pr;
                    }
                    if (!TAIL || qb + i + NR_RING < ncol) ring[u] = *vp;
                    vp += rpad;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < SB; i++) {
                    cn[i] = cf[i];
#pragma unroll
                    for (int v = 0; v < NV; v++) xc[i][v] = xn[i][v];
                }
            }
        };
        int q = 0;
        for (; q + 2 * NR_RING <= ncol; q += NR_RING) round(q, std::false_type{});
        for (; q < ncol; q += NR_RING) round(q, std::true_type{});
        if (m < nmem) row = p.grp_rows[rbeg + m];
    }
    if (row < 0) return;
    float* const yr = p.Y + row * p.ldy;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        float t = acc[v];
        if (p.relu) t = (t < 0.0f) ? 0.0f : t;              // torch relu: NaN stays NaN
        if (FULL || v < p.n_vecs) yr[v] = t;
    }
}

typedef void (*NarrowRowsKernel)(NarrowRowsArgs);
static NarrowRowsKernel narrow_rows_kernel(int nv, bool full) {
    switch (nv) {                                           // (a width of 1 or 2 columns always fills its form)
        case 1: return csr_narrow_kernel<1, true>;
        case 2: return csr_narrow_kernel<2, true>;
        case 4: return full ? csr_narrow_kernel<4, true> : csr_narrow_kernel<4, false>;
        default: return full ? csr_narrow_kernel<8, true> : csr_narrow_kernel<8, false>;
    }
}

// KN_FLAG_NARROW_ROWS on at most NARROW_MAX_VECS columns (narrow_rows_call): `groups` (CsrDev::nr: every pattern group, big ones included) and the `n_loose` rows of
// `loose_rows` in ONE launch, 64 member rows per wavefront.  A keyed Linear puts at most one wavefront on a SIMD whatever the height (VGG-16 fc6: 65 wavefronts at 64 rows, 257 at
// 16, on 1 024 SIMDs), and the bytes its value rings keep in flight are rows x 48 steps x 4 bytes at every height: the form with whole 256-byte value segments.
int csr_narrow_rows_spmm(const CsrDev& A, const WorkList& groups, const int32_t* loose_rows, int64_t n_loose, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu,
                         hipStream_t s) {
    const NarrowWidth w = narrow_width(n_vecs);
    const int64_t grid_grp = (groups.n + 3) / 4, grid_loose = (n_loose + 255) / 256;
    if (grid_grp + grid_loose == 0) return KN_OK;
    KN_REQUIRE(grid_grp + grid_loose < ((int64_t)1 << 31), KN_ERR_UNSUPPORTED, "grid too large for the row-lane kernel");
    NarrowRowsArgs a;
    a.n_items = groups.n;
    a.nr_grp = groups.grp;
    a.nr_r0 = groups.r0;
    a.grp_colptr = A.grp_colptr;
    a.grp_cols = A.grp_cols;
    a.grp_rowptr = A.grp_rowptr;
    a.grp_rows = A.grp_rows;
    a.grp_valptr = A.grp_valptr;
    a.grp_vals = A.grp_vals;
    a.n_loose = n_loose;
    a.loose_rows = loose_rows;
    a.indptr = A.indptr;
    a.indices = A.indices;
    a.data = A.data;
    a.X = x;
    a.Y = y;
    a.ldy = ldy;
    a.ldx4 = (uint32_t)(4 * ldx);
    a.n_vecs = (int)n_vecs;
    a.relu = relu;
    a.grid_grp = (uint32_t)grid_grp;
    KN_LAUNCH("csr_narrow_kernel<nv=" + std::to_string(w.nv) + (w.full ? "" : ",masked to " + std::to_string(n_vecs)) + ",rows=64> (lane = output row: " +
                  std::to_string(groups.n) + " group chunks, " + std::to_string(n_loose) + " loose rows)",
              narrow_rows_kernel(w.nv, w.full), dim3((unsigned)(grid_grp + grid_loose)), dim3(256), 0, s, a);
    KN_HIP(hipGetLastError());
    return KN_OK;
}

}  // namespace kn
