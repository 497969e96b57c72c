// ---- order-preserving path for 1 .. 8 batch columns with the taps RESIDENT and PACKED over output-channel PAIRS (KN_MODIFIER_NARROW_TAPS_PAIRS next to
// KN_FLAG_NARROW_TAPS, regime NARROW): a lane holds TWO output channels ----------
// Included by kn_conv.hip behind kn_conv_narrow_taps.inc (its scalar-load helpers and the forms' slot and tap counts).  convtaps_narrow_taps_kernel's arithmetic,
// statement for statement -- input channel outer, the pixel's slots by ascending input pixel inner, t = (coef == 1 ? a : coef * a), product and sum as two roundings,
// then the bias entry where it is stored, then ReLU -- so the result is that kernel's bit for bit.  What differs is how many channels share a step:
//   * the work item is (128-channel block, output pixel), pixel fastest, dealt to the XCDs in contiguous chunks, one pixel per wavefront.  Lane l of block cb2 holds
//     channels co0 = cb2 * 128 + l and co1 = co0 + 64 as the low and the high half of a packed register pair: a tap's value rows are two coalesced 256-byte loads
//     per input channel (tapsT[t][ci][co] is contiguous in co).  A trailing block with 64 padded channels only (cout_pad % 128 == 64) walks with co1 re-reading co0's
//     rows and stores nothing for it -- always in bounds, never 0 * x.
//   * per pixel, loaded ONCE and kept in scalar registers, as convtaps_narrow_taps_kernel keeps them: the <= 9 slots' byte offsets inside a channel's plane, their
//     packed 4-bit tap indices and, where the operator has them, their coefficients.  Per input channel: the NT = 9 | 16 value-row PAIRS in 32 vector registers (a
//     vector of 16 register pairs), requested one channel ahead, two sets in turn.
//   * a step is ONE scalar activation load (NV contiguous floats, the offset in a scalar register), ONE indexed read of the tap's register pair (scalar index mode)
//     and NV v_pk_mul_f32 + NV v_pk_add_f32: (a0, a1) * (x, x), the activation broadcast to both halves by op_sel / op_sel_hi from its half of an aligned scalar
//     pair.  Every element is its own IEEE multiply and its own IEEE add.  The scalar half of the step and the index-mode sequence are paid once for 128 channels.
//   * a channel's activation loads are issued in batches of G steps in front of that batch's arithmetic, one lgkmcnt(0) wait per batch.  They live in NAMED scalar
//     registers, s64 .. s95, dword R of a batch in s(64 + R): the packed multiply names the aligned pair that holds its dword, so load, wait and multiply agree on the
//     registers by construction (left to the register allocator a pair is a copy; tests/test_narrow_taps_pairs_host.py scans for any use before the wait).
// A pixel with fewer slots than the form holds takes wave-uniform branches around the steps it does not have -- never a product 0 * x.  Widths between the forms run
// the next NV (!FULL): the surplus sums are formed from the floats behind the batch's columns -- or, where that segment would leave the caller's block (tested once
// per wavefront, as convtaps_narrow_taps_kernel does), column by column from the last real column again -- and are not stored.
// No LDS, no barriers, no atomics, no scratch, nothing spilled into vector lanes; 32-bit offsets, checked by narrow_choice.
// dword R of a batch: X(R, its register, the aligned pair that holds it, which half)
#define KN_TP_D1(X)                                                                                                                                               \
    X(0, 64, 64, 65, 0) X(1, 65, 64, 65, 1) X(2, 66, 66, 67, 0) X(3, 67, 66, 67, 1) X(4, 68, 68, 69, 0) X(5, 69, 68, 69, 1) X(6, 70, 70, 71, 0) X(7, 71, 70, 71, 1)  \
    X(8, 72, 72, 73, 0) X(9, 73, 72, 73, 1) X(10, 74, 74, 75, 0) X(11, 75, 74, 75, 1) X(12, 76, 76, 77, 0) X(13, 77, 76, 77, 1) X(14, 78, 78, 79, 0)                \
    X(15, 79, 78, 79, 1) X(16, 80, 80, 81, 0) X(17, 81, 80, 81, 1) X(18, 82, 82, 83, 0) X(19, 83, 82, 83, 1) X(20, 84, 84, 85, 0) X(21, 85, 84, 85, 1)              \
    X(22, 86, 86, 87, 0) X(23, 87, 86, 87, 1) X(24, 88, 88, 89, 0) X(25, 89, 88, 89, 1) X(26, 90, 90, 91, 0) X(27, 91, 90, 91, 1) X(28, 92, 92, 93, 0)              \
    X(29, 93, 92, 93, 1) X(30, 94, 94, 95, 0) X(31, 95, 94, 95, 1)
#define KN_TP_D2(X)                                                                                                                                               \
    X(0, 64, 65) X(2, 66, 67) X(4, 68, 69) X(6, 70, 71) X(8, 72, 73) X(10, 74, 75) X(12, 76, 77) X(14, 78, 79) X(16, 80, 81) X(18, 82, 83) X(20, 84, 85)            \
    X(22, 86, 87) X(24, 88, 89) X(26, 90, 91) X(28, 92, 93) X(30, 94, 95)
#define KN_TP_D4(X)                                                                                                                                               \
    X(0, 64, 65, 66, 67) X(4, 68, 69, 70, 71) X(8, 72, 73, 74, 75) X(12, 76, 77, 78, 79) X(16, 80, 81, 82, 83) X(20, 84, 85, 86, 87) X(24, 88, 89, 90, 91)          \
    X(28, 92, 93, 94, 95)
#define KN_TP_D8(X) X(0, 64, 65, 66, 67, 68, 69, 70, 71) X(8, 72, 73, 74, 75, 76, 77, 78, 79) X(16, 80, 81, 82, 83, 84, 85, 86, 87) X(24, 88, 89, 90, 91, 92, 93, 94, 95)
// one column: dword R
template <int R>
__device__ __forceinline__ void pairs_load_col(int& x, const float* base, const uint32_t off) {
#define KN_TP_X(i, r, lo, hi, h) \
    if constexpr (R == i) asm volatile("s_load_dword s" #r ", %1, %2" : "=&{s" #r "}"(x) : "s"(base), "s"(off)); else
    KN_TP_D1(KN_TP_X) static_assert(R < 0, "dword of a batch");
#undef KN_TP_X
}
// a step's segment of NV floats: dwords R .. R + NV - 1
template <int NV, int R>
__device__ __forceinline__ void pairs_load_seg(int* x, const float* base, const uint32_t off) {
    if constexpr (NV == 1) pairs_load_col<R>(x[0], base, off);
    else if constexpr (NV == 2) {
#define KN_TP_X(i, a, b) \
    if constexpr (R == i) asm volatile("s_load_dwordx2 s[" #a ":" #b "], %2, %3" : "=&{s" #a "}"(x[0]), "=&{s" #b "}"(x[1]) : "s"(base), "s"(off)); else
        KN_TP_D2(KN_TP_X) static_assert(R < 0, "segment of a batch");
#undef KN_TP_X
    } else if constexpr (NV == 4) {
#define KN_TP_X(i, a, b, c, d)                                                                                                                             \
    if constexpr (R == i)                                                                                                                                  \
        asm volatile("s_load_dwordx4 s[" #a ":" #d "], %4, %5" : "=&{s" #a "}"(x[0]), "=&{s" #b "}"(x[1]), "=&{s" #c "}"(x[2]), "=&{s" #d "}"(x[3]) : "s"(base), "s"(off)); \
    else
        KN_TP_D4(KN_TP_X) static_assert(R < 0, "segment of a batch");
#undef KN_TP_X
    } else {
#define KN_TP_X(i, a, b, c, d, e, f, g, h)                                                                                                                 \
    if constexpr (R == i)                                                                                                                                  \
        asm volatile("s_load_dwordx8 s[" #a ":" #h "], %8, %9"                                                                                           \
                     : "=&{s" #a "}"(x[0]), "=&{s" #b "}"(x[1]), "=&{s" #c "}"(x[2]), "=&{s" #d "}"(x[3]), "=&{s" #e "}"(x[4]), "=&{s" #f "}"(x[5]), "=&{s" #g "}"(x[6]), \
                       "=&{s" #h "}"(x[7])                                                                                                                \
                     : "s"(base), "s"(off));                                                                                                              \
    else
        KN_TP_D8(KN_TP_X) static_assert(R < 0, "segment of a batch");
#undef KN_TP_X
    }
}
// every outstanding scalar load has landed: dword 0 carries the wait, the batch's other dwords are operands of empty statements behind it (volatile: in order)
template <int R>
__device__ __forceinline__ void pairs_landed(int& x) {
#define KN_TP_X(i, r, lo, hi, h)                                                       \
    if constexpr (R == i) {                                                            \
        if constexpr (R == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+{s" #r "}"(x)); \
        else asm volatile("" : "+{s" #r "}"(x));                                       \
    } else
    KN_TP_D1(KN_TP_X) static_assert(R < 0, "dword of a batch");
#undef KN_TP_X
}
// pr = (t.lo, t.hi) * (x, x), x dword R of the batch: one packed multiply, two IEEE multiplies
template <int R, typename P>
__device__ __forceinline__ void pairs_mul(P& pr, const int x, const P tt) {
#define KN_TP_X(i, r, lo, hi, h)                                                                                                                           \
    if constexpr (R == i)                                                                                                                                  \
        asm volatile("v_pk_mul_f32 %0, s[" #lo ":" #hi "], %2 op_sel:[" #h ",0] op_sel_hi:[" #h ",1]" : "=v"(pr) : "{s" #r "}"(x), "v"(tt));            \
    else
    KN_TP_D1(KN_TP_X) static_assert(R < 0, "dword of a batch");
#undef KN_TP_X
}
template <typename P>
__device__ __forceinline__ void pairs_add(P& sum, const P pr) { asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(sum) : "v"(pr)); }      // two IEEE adds
// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): the register names are compile-time values
template <int... I, typename F>
__device__ __forceinline__ void pairs_each(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void pairs_for(F&& f) { pairs_each(std::make_integer_sequence<int, N>{}, f); }
#pragma clang fp contract(off)
template <int NT, int NV, bool FULL, bool COEF>
__global__ __launch_bounds__(256) void convtaps_narrow_taps_pairs_kernel(ConvArgs p, int n_cb2, int n_pix, int64_t n_wg) {
    typedef float pair_t __attribute__((ext_vector_type(2)));
    typedef float taps_t __attribute__((ext_vector_type(TAPS_MAX_TAPS)));
    struct taps2_t { taps_t lo, hi; };                      // tap t of co0 and of co1: one index selects both
    static_assert(NV == 1 || NV == 2 || NV == 4 || NV == 8, "widths");
    static_assert(NT <= TAPS_MAX_TAPS && TAPS_MAX_SLOTS <= 16, "tap vector and packed tap indices");
    constexpr int MS = TAPS_MAX_SLOTS;
    // steps whose activations (G * NV named scalar registers, at most s64 .. s95) are in flight together
    constexpr int BUDGET = COEF ? (FULL ? 16 : 8) : (FULL ? 24 : 16);
    constexpr int G = BUDGET / NV >= MS ? MS : (BUDGET / NV >= 1 ? BUDGET / NV : 1);
    static_assert(G * NV <= 32, "the named registers");
    const int64_t chunk = (n_wg + 7) >> 3;
    const int64_t wg = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (wg >= n_wg || (blockIdx.x >> 3) >= chunk) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint32_t wi = (uint32_t)wg * 4u + (uint32_t)wave;      // (128-channel block, pixel in processing order), pixel fastest; below 2^31: checked by the launcher
    if (wi >= (uint32_t)n_pix * (uint32_t)n_cb2) return;          // (wave-uniform; no barriers in this kernel)
    const int cb2 = __builtin_amdgcn_readfirstlane((int)(wi / (uint32_t)n_pix));
    const int o = __builtin_amdgcn_readfirstlane(p.pix_order[wi - (uint32_t)cb2 * (uint32_t)n_pix]);
    const int co0 = cb2 * 128 + lane;
    const uint32_t hi_off = cb2 * 128 + 128 <= p.cout_pad ? 64u : 0u;      // a trailing half block: co1 re-reads co0's rows
    const uint32_t ldxb = (uint32_t)p.ldx * 4u;

    // the pixel's slot list: resident for the whole channel loop
    const int s_beg = __builtin_amdgcn_readfirstlane(p.pix_ptr[o]);
    int n = __builtin_amdgcn_readfirstlane(p.pix_ptr[o + 1]) - s_beg;
    uint32_t xb[MS];
    uint32_t tp[2] = {0, 0};                                // tap indices, 4 bits each: slots 0 .. 7, 8 .. 15
    float cf[MS];
#pragma unroll
    for (int k = 0; k < MS; k++) {
        const int e = k < n ? s_beg + k : (n > 0 ? s_beg : 0);      // beyond the list: its first slot (a pixel without slots: the operator's first)
        xb[k] = (uint32_t)p.slot_in[e] * ldxb;
        tp[k >> 3] |= ((uint32_t)p.slot_tap[e] & 15u) << (4 * (k & 7));
        cf[k] = COEF ? p.slot_coef[e] : 1.0f;
    }
    const bool all_full = n == MS;
    uint32_t lastb = 4u * (uint32_t)(p.n_vecs - 1);         // byte offset of the last real column: what the surplus sums of a width below NV read (column by column)

    pair_t acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = pair_t{0.0f, 0.0f};

    // this lane's value rows: tapsT[t][ci][cb2 * 128 + lane (+ 64)] (element offsets of 32 bits: checked by the launcher); taps the operator does not have re-read its
    // last one (a tap's offset is formed per channel, as convtaps_narrow_taps32_kernel forms it: kept per lane the sixteen offsets are sixteen more vector registers)
    uint32_t tap_stride = (uint32_t)p.cin_pad * (uint32_t)p.cout_pad, tap_last = (uint32_t)p.ntaps - 1u;
    const float* const tap0 = p.tapsT + cb2 * 128;          // wave-uniform
    const uint32_t lane1 = (uint32_t)lane + hi_off;
    auto rows = [&](taps2_t& A, const int ci) {             // the value-row pairs of input channel ci
        const float* const tc = tap0 + (uint32_t)ci * (uint32_t)p.cout_pad;
        asm volatile("" : "+s"(tap_stride), "+s"(tap_last));      // (opaque: the offsets below are this call's)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const uint32_t base = ((uint32_t)t < tap_last ? (uint32_t)t : tap_last) * tap_stride;
            A.lo[t] = tc[base + (uint32_t)lane];
            A.hi[t] = tc[base + lane1];
        }
    };
    auto channel = [&](const taps2_t& A, const float* const xc, auto full, auto seg) {      // one input channel's steps; xc: the channel's plane of X
        constexpr bool ALL = decltype(full)::value, SEG = decltype(seg)::value;
        asm volatile("" : "+s"(tp[0]), "+s"(tp[1]));       // (opaque: the indices stay packed -- hoisted out of the channel loop they are a scalar register per slot)
        if constexpr (!ALL) asm volatile("" : "+s"(n));    // (likewise the slot count: hoisted, every step's test is a lane mask in two scalar registers)
        if constexpr (!SEG) asm volatile("" : "+s"(lastb));      // (... and the column offsets)
#pragma unroll
        for (int k0 = 0; k0 < MS; k0 += G) {
            const int gn = MS - k0 < G ? MS - k0 : G;       // (a compile-time value once unrolled)
            int x[G * NV];
            auto batch = [&](auto gnc) {
                constexpr int GN = decltype(gnc)::value;
                pairs_for<GN * NV>([&](auto ic) {            // the batch's loads: a segment per step, or a load per column
                    constexpr int k = decltype(ic)::value / NV, v = decltype(ic)::value % NV;
                    if constexpr (SEG) {
                        if constexpr (v == 0) pairs_load_seg<NV, k * NV>(&x[k * NV], xc, xb[k0 + k]);
                    } else
                        pairs_load_col<k * NV + v>(x[k * NV + v], xc, xb[k0 + k] + (4u * v < lastb ? 4u * v : lastb));
                });
                pairs_for<GN * NV>([&](auto ic) { pairs_landed<decltype(ic)::value>(x[decltype(ic)::value]); });
                pairs_for<GN>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    if (ALL || k0 + k < n) {
                        if constexpr (!ALL) asm volatile("");      // (a branch, not a select per step: the selects' lane masks are two scalar registers per step)
                        int idx = (int)((tp[(k0 + k) >> 3] >> (4 * ((k0 + k) & 7))) & 15u);
                        asm volatile("" : "+s"(idx));       // (pinned in front of its step)
                        const pair_t a = pair_t{A.lo[idx], A.hi[idx]};      // scalar index mode, no memory access
                        pair_t tt = a;                      // the term as the reference stores it, per channel
                        if constexpr (COEF) {
                            tt.x = cf[k0 + k] == 1.0f ? a.x : cf[k0 + k] * a.x;
                            tt.y = cf[k0 + k] == 1.0f ? a.y : cf[k0 + k] * a.y;
                        }
                        pairs_for<NV>([&](auto vc) {
                            constexpr int v = decltype(vc)::value;
                            pair_t pr;
                            pairs_mul<k * NV + v>(pr, x[k * NV + v], tt);
                            pairs_add(acc[v], pr);
                        });
                    }
                });
            };
            if (gn == G) batch(std::integral_constant<int, G>{});
            else batch(std::integral_constant<int, (MS % G) ? (MS % G) : G>{});
            // (several batches per channel: the next batch's loads stay behind this batch's adds)
            if constexpr (G < MS) __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto walk = [&](auto full, auto seg) {                  // two sets of value rows in turn: a channel's rows are requested while the channel before it is summed
        taps2_t A0, A1;
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
    // per wavefront on the last channel's highest input pixel, as convtaps_narrow_taps_kernel does.  The wavefronts that fail fetch column by column.
    bool segs = true;
    if constexpr (!FULL) {
        uint32_t xb_max = 0;
#pragma unroll
        for (int k = 0; k < MS; k++) xb_max = xb[k] > xb_max ? xb[k] : xb_max;
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
    // through, as convtaps_narrow_taps_kernel's does: kept live across the walk they are a dozen scalar registers.
    typedef const ConvArgs __attribute__((address_space(4))) * kargs_t;
    kargs_t e = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(e));
    const float* const lastcol = e->lastcol;
    const int n_vecs = e->n_vecs;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int co = co0 + 64 * h;
        if (co >= e->Cout) continue;                        // (the absent half of a trailing block lies beyond cout_pad)
        const int64_t row = (int64_t)co * e->HoWo + o;
        if (lastcol) {
            const float lc = lastcol[row];
            if (lc != 0.0f) {                               // the bias entry exists in the reference's row only when it is stored
                const float* const xl = e->X + e->last_in_row * e->ldx;
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float bp = lc * xl[(FULL || v < n_vecs) ? v : n_vecs - 1];
                    acc[v][h] = acc[v][h] + bp;
                }
            }
        }
        float* const yr = e->Y + row * e->ldy;
        const int relu = e->relu;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            float t = acc[v][h];
            if (relu) t = (t < 0.0f) ? 0.0f : t;
            if (FULL || v < n_vecs) yr[v] = t;
        }
    }
}
#undef KN_TP_D1
#undef KN_TP_D2
#undef KN_TP_D4
#undef KN_TP_D8
