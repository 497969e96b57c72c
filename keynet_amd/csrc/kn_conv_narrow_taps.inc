// ---- order-preserving path for 1 .. 8 batch columns with the taps RESIDENT (KN_FLAG_NARROW_TAPS next to KN_FLAG_NARROW): lanes are OUTPUT CHANNELS ----------
// Included by kn_conv.hip (namespace kn, behind ConvArgs).  convtaps_narrow_kernel's arithmetic, statement for statement -- input channel outer, the pixel's slots by
// ascending input pixel inner, t = (coef == 1 ? a : coef * a), separate multiply and add, then the bias entry where it is stored, then ReLU -- so the result is that
// kernel's bit for bit.  What differs is what a step FETCHES.  That kernel loads three slot records, forms two addresses and loads a 256-byte value row for every
// (input channel, slot) step, although all of it but the activation is the same for every input channel of a pixel.  Here
//   * a wavefront owns P output pixels (consecutive in pix_order) x 64 output channels (lane = channel) x NV (1 | 2 | 4 | 8) running sums per pixel;
//   * per pixel, loaded ONCE in front of the channel loop and kept in scalar registers: the slots' activation offsets inside a channel's plane (slot_in * ldx, in
//     bytes, 32 bits: narrow_choice checks 4 * HiWi * ldx), their tap indices (4 bits each, packed) and, where the operator has them, their coefficients;
//   * per input channel, loaded ONCE into 16 vector registers: the value rows tapsT[t][ci][cb * 64 + lane] of every tap (NT = 9 | 16 loads; taps the operator does not
//     have re-read its last one -- no run-time tap count in the loads).  They are requested one channel ahead of their use (two register sets in turn), and the P
//     pixels share them: P = 2 halves the value-row traffic per step.
//   * a step is then ONE scalar activation load (NV contiguous floats where the batch fills the form), one indexed register read (scalar index mode: At[tap]) and NV
//     multiply / add pairs.  A channel's activation loads are issued in batches of G steps x P pixels in front of that batch's adds (all 9 steps of the channel where
//     they fit the scalar registers: P * NV <= 2).
// A pixel with fewer slots than the form holds (TAPS_MAX_SLOTS; window borders, strided layers) takes wave-uniform branches around the steps it does not have -- never a
// product 0 * x, so a non-finite activation reaches the outputs that hold it and no other; a wavefront whose pixels all have the full count runs the straight-line
// body.  Slots beyond a pixel's list re-read its first slot (loaded, not used).  A last group with fewer than P pixels stores nothing for the missing ones (they walk
// as pixels without slots).  Widths between the forms run the next NV (!FULL): the surplus sums are formed from the floats behind the batch's columns -- or, where
// that segment would leave the caller's block, from the last real column again -- and are not stored.
// Work items are (channel block, pixel group) with the GROUP fastest, dealt to the XCDs in contiguous chunks, as convtaps_narrow_kernel's.
// No LDS, no barriers, no atomics, no scratch, nothing spilled into vector lanes (tests/test_narrow_taps_host.py).
static constexpr int TAPS_MAX_SLOTS = NARROW_TAPS_MAX_SLOTS;      // slots per output pixel the forms hold (a 3 x 3 window; kn_internal.h: the eligibility rule)
static constexpr int TAPS_MAX_TAPS = NARROW_TAPS_MAX_TAPS;        // taps held in registers per lane and input channel
// A step's activations through the scalar data cache with the offset in a scalar register (s_load_dword[x2|x4|x8] sdst, sbase, soffset): written as inline assembly,
// because the compiler forms a 64-bit address per step instead (and, strength-reducing those, keeps a 64-bit pointer per slot: every form then spilled scalar
// registers).  The compiler does not count these loads, so taps_wait stands between them and their first use: it waits for ALL outstanding scalar loads and takes the
// destinations as read-write operands, which orders every use behind it.  What that cannot rule out is a register COPY of a destination between load and wait (a copy of
// a segment that has not landed): tests/test_narrow_taps_host.py scans every instantiation for any instruction that names a destination in between.
template <int NV> struct TapsVec { typedef int type __attribute__((ext_vector_type(NV))); };
template <> struct TapsVec<1> { typedef int type; };
template <int NV>
__device__ __forceinline__ void taps_load_seg(typename TapsVec<NV>::type& x, const float* base, const uint32_t off) {
    if constexpr (NV == 1) asm volatile("s_load_dword %0, %1, %2" : "=&s"(x) : "s"(base), "s"(off));
    else if constexpr (NV == 2) asm volatile("s_load_dwordx2 %0, %1, %2" : "=&s"(x) : "s"(base), "s"(off));
    else if constexpr (NV == 4) asm volatile("s_load_dwordx4 %0, %1, %2" : "=&s"(x) : "s"(base), "s"(off));
    else asm volatile("s_load_dwordx8 %0, %1, %2" : "=&s"(x) : "s"(base), "s"(off));
}
__device__ __forceinline__ void taps_load_col(int& x, const float* base, const uint32_t off) { asm volatile("s_load_dword %0, %1, %2" : "=&s"(x) : "s"(base), "s"(off)); }
template <int N, typename T>
__device__ __forceinline__ void taps_wait(T* x) {       // x[0 .. N) have landed
    static_assert(N >= 1 && N <= 9, "operands of one wait");
    if constexpr (N == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(x[0]));
    else if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(x[0]), "+s"(x[1]));
    else if constexpr (N == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(x[0]), "+s"(x[1]), "+s"(x[2]));
    else if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(x[0]), "+s"(x[1]), "+s"(x[2]), "+s"(x[3]));
    else if constexpr (N == 9)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(x[0]), "+s"(x[1]), "+s"(x[2]), "+s"(x[3]), "+s"(x[4]), "+s"(x[5]), "+s"(x[6]), "+s"(x[7]), "+s"(x[8]));
    else {
        taps_wait<4>(x);
        taps_wait<N - 4>(x + 4);
    }
}
#pragma clang fp contract(off)
template <int NT, int P, int NV, bool FULL, bool COEF>
__global__ __launch_bounds__(256) void convtaps_narrow_taps_kernel(ConvArgs p, int n_cb, int n_grp, int64_t n_wg) {
    typedef float taps_t __attribute__((ext_vector_type(TAPS_MAX_TAPS)));
    constexpr int MS = TAPS_MAX_SLOTS;
    // steps whose activations (G * P * NV scalar registers) are in flight together: what the scalar register file holds next to the slot lists -- 20 registers, 12 with
    // coefficients (9 more resident registers) or a masked width (a second walk that fetches column by column), 8 with both.  Every larger batch compiled with scalar
    // registers spilled into vector lanes.
    constexpr int BUDGET = COEF ? (FULL ? 12 : 8) : (FULL ? 20 : 12);
    constexpr int G = BUDGET / (P * NV) >= MS ? MS : (BUDGET / (P * NV) >= 1 ? BUDGET / (P * NV) : 1);
    static_assert(NT <= TAPS_MAX_TAPS && MS <= 16, "tap vector and packed tap indices");
    const int64_t chunk = (n_wg + 7) >> 3;
    const int64_t wg = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (wg >= n_wg || (blockIdx.x >> 3) >= chunk) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint32_t wi = (uint32_t)wg * 4u + (uint32_t)wave;      // (channel block, pixel group in processing order), group fastest; below 2^31: checked by the launcher
    if (wi >= (uint32_t)n_grp * (uint32_t)n_cb) return;           // (wave-uniform; no barriers in this kernel)
    const int cb = (int)(wi / (uint32_t)n_grp);
    const int g0 = (int)(wi - (uint32_t)cb * (uint32_t)n_grp) * P;      // first pixel of the group (position in pix_order)
    const int co = cb * 64 + lane;
    const uint32_t ldxb = (uint32_t)p.ldx * 4u;

    // the pixels' slot lists: resident for the whole channel loop
    int o[P], n[P];
    uint32_t xb[P][MS];
    uint32_t tp[P][2];                                      // tap indices, 4 bits each: slots 0 .. 7, 8 .. 15
    float cf[P][MS];
    bool all_full = true;
#pragma unroll
    for (int j = 0; j < P; j++) {
        const bool have = j == 0 || g0 + j < p.n_pix;           // (a group's first pixel always exists)
        o[j] = __builtin_amdgcn_readfirstlane(p.pix_order[have ? g0 + j : g0]);
        const int s_beg = __builtin_amdgcn_readfirstlane(p.pix_ptr[o[j]]);
        n[j] = have ? __builtin_amdgcn_readfirstlane(p.pix_ptr[o[j] + 1]) - s_beg : 0;
        if (!have) o[j] = -1;
        all_full = all_full && n[j] == MS;
        tp[j][0] = tp[j][1] = 0;
#pragma unroll
        for (int k = 0; k < MS; k++) {
            const int e = k < n[j] ? s_beg + k : (n[j] > 0 ? s_beg : 0);      // beyond the list: its first slot (a pixel without slots: the operator's first)
            xb[j][k] = (uint32_t)p.slot_in[e] * ldxb;
            tp[j][k >> 3] |= ((uint32_t)p.slot_tap[e] & 15u) << (4 * (k & 7));
            cf[j][k] = COEF ? p.slot_coef[e] : 1.0f;
        }
    }
    uint32_t lastb = 4u * (uint32_t)(p.n_vecs - 1);         // byte offset of the last real column: what the surplus sums of a width below NV read (column by column)

    float acc[P][NV];
#pragma unroll
    for (int j = 0; j < P; j++)
#pragma unroll
        for (int v = 0; v < NV; v++) acc[j][v] = 0.0f;

    // this lane's value rows: element offsets of the taps inside the channel block's share of tapsT (32 bits: checked by the launcher)
    uint32_t to[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) to[t] = (uint32_t)(t < p.ntaps ? t : p.ntaps - 1) * ((uint32_t)p.cin_pad * (uint32_t)p.cout_pad) + (uint32_t)lane;
    const float* const tap0 = p.tapsT + cb * 64;            // wave-uniform
    auto rows = [&](taps_t& A, const int ci) {              // the value rows of input channel ci
        const float* const tc = tap0 + (uint32_t)ci * (uint32_t)p.cout_pad;
#pragma unroll
        for (int t = 0; t < NT; t++) A[t] = tc[to[t]];
    };
    auto channel = [&](const taps_t& A, const float* const xc, auto full, auto seg) {      // one input channel's steps of the P pixels; xc: the channel's plane of X
        constexpr bool ALL = decltype(full)::value, SEG = decltype(seg)::value;
#pragma unroll
        for (int j = 0; j < P; j++)                         // (opaque: the indices stay packed -- hoisted out of the channel loop they are a scalar register per slot)
            asm volatile("" : "+s"(tp[j][0]), "+s"(tp[j][1]));
        if constexpr (!ALL) {                               // (likewise the slot counts: hoisted, every step's test is a lane mask in two scalar registers)
#pragma unroll
            for (int j = 0; j < P; j++) asm volatile("" : "+s"(n[j]));
        }
        if constexpr (!SEG) asm volatile("" : "+s"(lastb));      // (... and the column offsets)
#pragma unroll
        for (int k0 = 0; k0 < MS; k0 += G) {
            constexpr int GN_MAX = G;
            const int gn = MS - k0 < G ? MS - k0 : G;       // (a compile-time value once unrolled)
            typename TapsVec<NV>::type xv[P][GN_MAX];
            int xs[P][GN_MAX][NV];
#pragma unroll
            for (int k = 0; k < gn; k++)
#pragma unroll
                for (int j = 0; j < P; j++) {
                    if constexpr (SEG) {
                        taps_load_seg<NV>(xv[j][k], xc, xb[j][k0 + k]);
                    } else {
#pragma unroll
                        for (int v = 0; v < NV; v++) taps_load_col(xs[j][k][v], xc, xb[j][k0 + k] + (4u * v < lastb ? 4u * v : lastb));
                    }
                }
#pragma unroll
            for (int j = 0; j < P; j++) {
                if constexpr (SEG) {
                    if (k0 + G <= MS) taps_wait<G>(xv[j]);
                    else taps_wait<(MS % G) ? (MS % G) : G>(xv[j]);
                } else {
#pragma unroll
                    for (int k = 0; k < gn; k++)
#pragma unroll
                        for (int v = 0; v < NV; v++) taps_wait<1>(&xs[j][k][v]);
                }
            }
#pragma unroll
            for (int k = 0; k < gn; k++)
#pragma unroll
                for (int j = 0; j < P; j++) {
                    if (ALL || k0 + k < n[j]) {
                        if constexpr (!ALL) asm volatile("");      // (a branch, not a select per step: the selects' lane masks are two scalar registers per step)
                        const float a = A[(int)((tp[j][(k0 + k) >> 3] >> (4 * ((k0 + k) & 7))) & 15u)];       // scalar index mode, no memory access
                        const float t = COEF ? (cf[j][k0 + k] == 1.0f ? a : cf[j][k0 + k] * a) : a;      // the term as the reference stores it
#pragma unroll
                        for (int v = 0; v < NV; v++) {
                            int xi;                             // (the element as a value first: a bit cast of the vector element itself reads element 0)
                            if constexpr (!SEG) xi = xs[j][k][v];
                            else if constexpr (NV == 1) xi = xv[j][k];
                            else xi = xv[j][k][v];
                            const float xa = __builtin_bit_cast(float, xi);
                            const float pr = t * xa;
                            acc[j][v] = acc[j][v] + pr;
                        }
                    }
                }
            // (several batches per channel: the next batch's loads stay behind this batch's adds -- moved up by the scheduler, every batch of the straight-line walk got
            // scalar registers of its own)
            if constexpr (G < MS) __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto walk = [&](auto full, auto seg) {                  // two sets of value rows in turn: a channel's rows are requested while the channel before it is summed
        taps_t A0, A1;
        const float* xc = p.X;
        const int64_t plane = (int64_t)p.HiWi * p.ldx;
        const int last = p.Cin - 1;
        rows(A0, 0);
        for (int ci = 0; ci < p.Cin; ci += 2) {
            rows(A1, ci + 1 < last ? ci + 1 : last);
            channel(A0, xc, full, seg);
            xc += plane;
            if (ci + 1 >= p.Cin) break;
            rows(A0, ci + 2 < last ? ci + 2 : last);
            channel(A1, xc, full, seg);
            xc += plane;
        }
    };
    // A step's activations are ONE segment of NV floats.  Where the batch does not fill the form (!FULL) the segment must still lie inside the caller's block: tested once
    // per wavefront on the last channel's highest input pixel, as convtaps_narrow32_kernel does (with a homogeneous row behind the activations every wavefront passes).
    // The wavefronts that fail fetch column by column.
    bool segs = true;
    if constexpr (!FULL) {
        uint32_t xb_max = 0;
#pragma unroll
        for (int j = 0; j < P; j++)
#pragma unroll
            for (int k = 0; k < MS; k++) xb_max = xb[j][k] > xb_max ? xb[j][k] : xb_max;
        const int64_t far = (int64_t)(p.Cin - 1) * p.HiWi * p.ldx + (int64_t)(xb_max >> 2) + NV;
        segs = far <= (p.last_in_row - (p.lastcol ? 0 : 1)) * p.ldx + p.n_vecs;
    }
    if (segs) {
        if (all_full) walk(std::true_type{}, std::true_type{});
        else walk(std::false_type{}, std::true_type{});
    } else {
        if constexpr (!FULL) walk(std::false_type{}, std::false_type{});
    }

    // The epilogue reads its arguments from the kernel argument segment AGAIN (ConvArgs is the first parameter: offset 0), through a pointer the compiler cannot see
    // through: kept live across the walk they were a dozen scalar registers, spilled into vector lanes in front of the loop in the widest forms.
    typedef const ConvArgs __attribute__((address_space(4))) * kargs_t;
    kargs_t e = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(e));
    if (co >= e->Cout) return;
    const float* const lastcol = e->lastcol;
    const int n_vecs = e->n_vecs;
#pragma unroll
    for (int j = 0; j < P; j++) {
        if (o[j] < 0) continue;
        const int64_t row = (int64_t)co * e->HoWo + o[j];
        if (lastcol) {
            const float lc = lastcol[row];
            if (lc != 0.0f) {                               // the bias entry exists in the reference's row only when it is stored
                const float* const xl = e->X + e->last_in_row * e->ldx;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float bp = lc * xl[(FULL || v < n_vecs) ? v : n_vecs - 1];
                    acc[j][v] = acc[j][v] + bp;
                }
            }
        }
        float* const yr = e->Y + row * e->ldy;
        const int relu = e->relu;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            float t = acc[j][v];
            if (relu) t = (t < 0.0f) ? 0.0f : t;
            if (FULL || v < n_vecs) yr[v] = t;
        }
    }
}
