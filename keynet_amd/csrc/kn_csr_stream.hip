// kn_csr_stream.hip -- order-preserving product of a keyed Linear's BIG pattern groups for 1 .. 32 batch columns (KN_FLAG_NARROW_LINEAR): lanes are OUTPUT ROWS,
// values AND activations stream through an LDS ring.
//
// csr_big_group_kernel (kn_csr.hip) gives a lane a batch column and a workgroup 32 rows: its cost is that of 64 columns at every width.  csr_narrow_kernel
// (kn_csr_narrow.hip) gives a lane a row, but a wavefront keeps only its own 48 x 256 bytes of values requested and pays a scalar-cache round trip per step.  Here a
// WORKGROUP owns 64 member rows of one big group times ALL n_vecs <= 32 columns of the call, so a step's values -- grp_vals is [column j][member row]: one coalesced
// 256-byte segment -- leave HBM once per call:
//   * the ring: NSLOT slots, each one SLAB of 16 steps: [16 x 64 values][16 x CW activations][64 column indices], CW = W * NV.  The W wavefronts fill it with
//     global_load_lds, PF = NSLOT - 3 slabs ahead of the walk: four 16-byte-per-lane pieces of values (1 KB each), CW / 4 (at least one) 4-byte-per-lane pieces of
//     activations (a lane gathers X[cols[step], column], 64 / CW steps per piece; columns beyond n_vecs repeat the last real one), and one piece of column indices --
//     those of the slab PF slabs FURTHER on, which the activation pieces of that slab read back from LDS when their turn comes: no load in the loop returns into a
//     register, so nothing but the counted wait ever waits for memory.  Piece i of a slab is issued by wavefront i % W; every wavefront issues LPW = ceil(pieces / W)
//     loads per slab (the surplus ones repeat a piece), so one count holds for all.  A slab is published by a COUNTED wait (every wavefront: its own pieces of that
//     slab have landed, the PF - 1 younger slabs stay in flight) and a raw barrier; the slot a fill overwrites was last read three barriers earlier.  Fills beyond
//     the end of the sequence re-read its last step (the count of loads in flight stays the same on every trip) and are drained before the workgroup ends.
//   * walkers: wavefront w owns the NV consecutive columns w * NV ..; lane = member row.  Per step one ds_read_b32 per lane for the value and one BROADCAST read
//     of the wavefront's NV activations (4 * NV bytes, the same address in every lane), both requested one batch of SB steps ahead of the adds that consume them.
//     W * NV >= n_vecs; widths between the forms run the next form, the surplus sums repeat the last real column and store nothing (csr_narrow_kernel's convention).
//     Lanes beyond the member count read what the segment holds there (the padding of rpad, or -- in a last chunk -- values of the next step: inside grp_vals, which
//     ends with 64 floats of padding) and store nothing.
// Arithmetic: csr_big_group_kernel's / csr_narrow_kernel's statement for statement: per output element a strictly serial walk over the stored columns,
// p = a * x; acc = acc + p, separately rounded, then ReLU.  The walk is never split across lanes or wavefronts.  Static LDS only (at most 64 000 bytes), no workspace,
// no atomics.  Every address into X, grp_vals and Y is formed in 64 bits: no condition on ldx.
#include "kn_internal.h"
#include <type_traits>

#pragma clang fp contract(off)

namespace kn {

struct StreamArgs {
    int64_t n_items;                 // 64-row chunks of the big pattern groups: (group, first member)
    const int32_t* sg_grp;
    const int32_t* sg_r0;
    const int32_t* grp_colptr;
    const int32_t* grp_cols;
    const int32_t* grp_rowptr;
    const int32_t* grp_rows;
    const int64_t* grp_valptr;
    const float* grp_vals;
    const float* X;
    float* Y;
    int64_t ldy;
    int64_t ldx4;                    // ldx in bytes
    int n_vecs;
    int relu;
};

// The ring of a form (the slot count is stream_ring_slots, kn_internal.h: kn_spmm_plan prints it)
template <int W, int NV>
struct StreamRing {
    static constexpr int CW = W * NV;                           // activations per step: the columns of the form
    static constexpr int SLAB = STREAM_SLAB_STEPS;
    static constexpr int V_FLOATS = SLAB * 64;
    static constexpr int X_FLOATS = SLAB * CW < 64 ? 64 : SLAB * CW;           // (a piece writes 64 floats)
    static constexpr int SLOT_FLOATS = V_FLOATS + X_FLOATS + 64;
    static constexpr int NSLOT = stream_ring_slots(CW);
    static constexpr int PF = NSLOT - STREAM_SPARE_SLOTS;       // slabs in flight
    static constexpr int G = CW >= 4 ? 64 / CW : SLAB;          // steps per activation piece
    static constexpr int XP = SLAB / G;                         // activation pieces per slab
    static constexpr int P = 4 + XP + 1;                        // pieces per slab: values, activations, column indices
    static constexpr int LPW = (P + W - 1) / W;                 // loads per wavefront and slab
    static_assert(SLOT_FLOATS * 4 == stream_slot_bytes(CW) && NSLOT * SLOT_FLOATS * 4 <= 64 * 1024 && PF >= 2, "static LDS");
    static_assert(W * LPW < 2 * P && SLOT_FLOATS % 4 == 0, "a surplus load repeats a piece");
};

typedef const __attribute__((address_space(1))) void* GlobalSrc;
typedef __attribute__((address_space(3))) void* LdsDst;

template <int W, int NV>
__global__ __launch_bounds__(64 * W) void csr_stream_group_kernel(StreamArgs p) {
    typedef StreamRing<W, NV> R;
    constexpr int SB = NV <= 2 ? 8 : (NV == 4 ? 4 : 2);                        // steps per batch of LDS reads
    constexpr int NB = R::SLAB / SB;                            // batches per slab
    static_assert(R::SLAB % SB == 0 && NB >= 2, "the last batch of a slab reads ahead into the next one");
    __shared__ __attribute__((aligned(16))) float ring[R::NSLOT * R::SLOT_FLOATS];
    const int lane = threadIdx.x & 63;
    const int wave = W == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t e = blockIdx.x;
    if (e >= p.n_items) return;                                 // (uniform over the workgroup, as every return below)
    const int g = __builtin_amdgcn_readfirstlane(p.sg_grp[e]);
    const int r0 = __builtin_amdgcn_readfirstlane(p.sg_r0[e]);
    const int cbeg = __builtin_amdgcn_readfirstlane(p.grp_colptr[g]);
    const int ncol = __builtin_amdgcn_readfirstlane(p.grp_colptr[g + 1]) - cbeg;
    const int rbeg = __builtin_amdgcn_readfirstlane(p.grp_rowptr[g]);
    const int nmem = __builtin_amdgcn_readfirstlane(p.grp_rowptr[g + 1]) - rbeg;
    const int rpad = (nmem + 15) / 16 * 16;
    if (r0 >= nmem || ncol <= 0) return;
    const int32_t* const cols = p.grp_cols + cbeg;
    const int last = ncol - 1;

    // ---- the fills -----------------------------------------------------------------------------------------------------------------------------
    // values: piece i < 4 is steps 4 i .. 4 i + 3 of the slab, a lane's 16 bytes are rows 4 (lane % 16) .. + 3 of step 4 i + lane / 16
    const float* const vsrc = p.grp_vals + p.grp_valptr[g] + r0 + (lane & 15) * 4;      // rpad % 16 == 0, r0 % 64 == 0: 16-byte aligned
    // activations: piece k is steps k G .. k G + G - 1, a lane's float is column lane % CW (columns beyond the batch: its last) of step k G + lane / CW
    const int xcol = (lane & (R::CW - 1)) < p.n_vecs ? (lane & (R::CW - 1)) : p.n_vecs - 1;
    const char* const xsrc = reinterpret_cast<const char*>(p.X + xcol);
    const int xstep = (lane / R::CW) < R::G ? (lane / R::CW) : R::G - 1;               // (CW < 4: the lanes beyond 16 steps repeat the last one into the slack of the block)
    auto xstep_of = [&](int i) {                                // the step (inside its slab) whose column index this lane needs for piece i, were it an activation piece
        int k = i - 4;
        k = k < 0 ? 0 : (k < R::XP ? k : R::XP - 1);
        return k * R::G + xstep;
    };
    auto piece_of = [&](int l) {                                // the l-th load of this wavefront in a slab
        const int i = wave + W * l;
        return i < R::P ? i : i - R::P;
    };
    int fslab = 0, fslot = 0, cslot = 0;                        // the next slab to request, its slot, and the slot that holds its column indices
    // `colof(l)`: the column index of step xstep_of(piece_of(l)) of slab fslab
    auto fill = [&](auto colof) {
        float* const slot = ring + fslot * R::SLOT_FLOATS;
#pragma unroll
        for (int l = 0; l < R::LPW; l++) {
            const int i = piece_of(l);
            if (i < 4) {
                int j = fslab * R::SLAB + i * 4 + (lane >> 4);
                j = j < last ? j : last;
                __builtin_amdgcn_global_load_lds((GlobalSrc)(vsrc + (int64_t)j * rpad), (LdsDst)(slot + i * 256), 16, 0, 0);      // (the LDS address is wave-uniform: the hardware adds lane x 16 bytes)
            } else if (i < 4 + R::XP) {
                const int64_t col = colof(l);
                __builtin_amdgcn_global_load_lds((GlobalSrc)(xsrc + col * p.ldx4), (LdsDst)(slot + R::V_FLOATS + (i - 4) * 64), 4, 0, 0);
            } else {
                int j = (fslab + R::PF) * R::SLAB + lane;       // the column indices of the slab PF slabs on (64 of them: the first 16 are read)
                j = j < last ? j : last;
                __builtin_amdgcn_global_load_lds((GlobalSrc)(cols + j), (LdsDst)(slot + R::V_FLOATS + R::X_FLOATS), 4, 0, 0);
            }
        }
        fslab++;
        fslot = fslot + 1 == R::NSLOT ? 0 : fslot + 1;
    };
    // the first PF slabs: their column indices straight from memory, all requested before the first fill
    {
        int c0[R::PF][R::LPW];
#pragma unroll
        for (int u = 0; u < R::PF; u++)
#pragma unroll
            for (int l = 0; l < R::LPW; l++) {
                const int j = u * R::SLAB + xstep_of(piece_of(l));
                c0[u][l] = cols[j < last ? j : last];
            }
#pragma unroll
        for (int u = 0; u < R::PF; u++)
#pragma unroll
            for (int l = 0; l < R::LPW; l++) asm volatile("" : "+v"(c0[u][l]));        // all of them landed here: none is requested between two fills (a wait there would drain the fills before it)
#pragma unroll
        for (int u = 0; u < R::PF; u++) fill([&](int l) { return c0[u][l]; });
    }
    // slabs up to the published one may be read; PF - 1 younger slabs stay in flight across the barrier, the fill behind it restores PF: its activation pieces
    // read their column indices from the slot of the slab PF slabs back, which the wait and the barrier have just covered
    auto publish = [&]() {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((R::PF - 1) * R::LPW) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int* const staged = reinterpret_cast<const int*>(ring + cslot * R::SLOT_FLOATS + R::V_FLOATS + R::X_FLOATS);
        fill([&](int l) { return staged[xstep_of(piece_of(l))]; });
        cslot = cslot + 1 == R::NSLOT ? 0 : cslot + 1;
    };
    publish();                                                  // slab 0

    // ---- the walk ------------------------------------------------------------------------------------------------------------------------------
    const int c0 = wave * NV;                                   // the wavefront's first column
    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = 0.0f;
    auto xread = [&](float (&d)[NV], const float* xp) {         // NV consecutive activations, the same address in every lane (a broadcast); plain float reads: a
#pragma unroll                                                  // vector-typed read of this array makes the compiler drain the fills in flight (vmcnt(0)) ahead of it
        for (int v = 0; v < NV; v++) d[v] = xp[v];
    };
    const float* rd = ring + lane;                              // the lane's value of step 0 of the slab the walk is in
    const float* rx = ring + R::V_FLOATS + c0;                  // the wavefront's activations of that step
    int rslot = 0;
    float xc[SB][NV], vc[SB];                                   // activations and values of the batch the arithmetic is at
#pragma unroll
    for (int i = 0; i < SB; i++) {
        vc[i] = rd[i * 64];
        xread(xc[i], rx + i * R::CW);
    }

    // one round = one slab from step q on, in batches of SB steps.  TAIL: the last slab (steps beyond the sequence are not added; the slab after it holds copies
    // of the last step)
    auto round = [&](const int q, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        const float* rdn = rd;
        const float* rxn = rx;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int qb = q + b * SB;
            if (TAIL && qb >= ncol) break;
            if (b == NB - 1) {                                  // the values of the next batch are in the next slab
                publish();
                rslot = rslot + 1 == R::NSLOT ? 0 : rslot + 1;
                rdn = ring + rslot * R::SLOT_FLOATS + lane;
                rxn = ring + rslot * R::SLOT_FLOATS + R::V_FLOATS + c0;
            }
            float xn[SB][NV], vn[SB];
#pragma unroll
            for (int i = 0; i < SB; i++) {
                const int s = (b + 1) * SB + i;
                vn[i] = b == NB - 1 ? rdn[i * 64] : rd[s * 64];
                xread(xn[i], b == NB - 1 ? rxn + i * R::CW : rx + s * R::CW);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < SB; i++) {
                if (TAIL && qb + i >= ncol) break;
                const float a = vc[i];
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float pr = a * xc[i][v];
                    acc[v] = acc[v] + pr;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < SB; i++) {
                vc[i] = vn[i];
#pragma unroll
                for (int v = 0; v < NV; v++) xc[i][v] = xn[i][v];
            }
        }
        rd = rdn;
        rx = rxn;
    };
    int q = 0;
    for (; q + R::SLAB < ncol; q += R::SLAB) round(q, std::false_type{});
    round(q, std::true_type{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // no fill may land in this LDS after the workgroup has ended

    const int m = r0 + lane;
    if (m >= nmem) return;
    const int64_t row = p.grp_rows[rbeg + m];
    float* const yr = p.Y + row * p.ldy;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        float t = acc[v];
        if (p.relu) t = (t < 0.0f) ? 0.0f : t;                  // torch relu: NaN stays NaN
        if (c0 + v < p.n_vecs) yr[c0 + v] = t;
    }
}

typedef void (*StreamKernel)(StreamArgs);
static StreamKernel stream_kernel(const StreamForm& f) {
    switch (f.w * 16 + f.nv) {
        case 1 * 16 + 1: return csr_stream_group_kernel<1, 1>;
        case 2 * 16 + 1: return csr_stream_group_kernel<2, 1>;
        case 4 * 16 + 1: return csr_stream_group_kernel<4, 1>;
        case 8 * 16 + 1: return csr_stream_group_kernel<8, 1>;
        case 8 * 16 + 2: return csr_stream_group_kernel<8, 2>;
        default: return csr_stream_group_kernel<8, 4>;          // (NV = 8, for 33 .. 64 columns, measured slower than the kernel it would replace: narrow_linear_loses)
    }
}

// KN_FLAG_NARROW_LINEAR on at most STREAM_MAX_VECS columns (narrow_linear_call): the big pattern groups in 64-row chunks (CsrDev::sg), one workgroup per chunk.
int csr_stream_group_spmm(const CsrDev& A, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, int relu, hipStream_t s) {
    const StreamForm f = stream_form(n_vecs);
    if (A.sg.n == 0) return KN_OK;
    KN_REQUIRE(A.sg.n < ((int64_t)1 << 31) && n_vecs <= STREAM_MAX_VECS, KN_ERR_UNSUPPORTED, "grid too large or batch too wide for the value-stream kernel");
    StreamArgs a;
    a.n_items = A.sg.n;
    a.sg_grp = A.sg.grp;
    a.sg_r0 = A.sg.r0;
    a.grp_colptr = A.grp_colptr;
    a.grp_cols = A.grp_cols;
    a.grp_rowptr = A.grp_rowptr;
    a.grp_rows = A.grp_rows;
    a.grp_valptr = A.grp_valptr;
    a.grp_vals = A.grp_vals;
    a.X = x;
    a.Y = y;
    a.ldy = ldy;
    a.ldx4 = 4 * ldx;
    a.n_vecs = (int)n_vecs;
    a.relu = relu;
    const int slots = stream_ring_slots(f.w * f.nv);
    KN_LAUNCH("csr_stream_group_kernel<W=" + std::to_string(f.w) + ",NV=" + std::to_string(f.nv) + (f.full ? "" : ",masked to " + std::to_string(n_vecs)) + "> (values and activations through an LDS ring: " +
                  std::to_string(A.sg.n) + " chunks of 64 rows, ring of " + std::to_string(slots) + " slabs x " + std::to_string(STREAM_SLAB_STEPS) + " steps, " +
                  std::to_string((slots - STREAM_SPARE_SLOTS) * STREAM_SLAB_STEPS * 256 / 1024) + " KB of values in flight)",
              stream_kernel(f), dim3((unsigned)A.sg.n), dim3(64 * f.w), 0, s, a);
    KN_HIP(hipGetLastError());
    return KN_OK;
}

}  // namespace kn
