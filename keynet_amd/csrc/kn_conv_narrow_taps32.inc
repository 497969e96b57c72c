// ---- order-preserving path for 9 .. 32 batch columns with the taps RESIDENT and PACKED f32 arithmetic (KN_MODIFIER_NARROW_TAPS32 next to KN_FLAG_NARROW_TAPS, regime
// NARROW32): lanes are OUTPUT CHANNELS, columns come in blocks ----------
// Included by kn_conv.hip behind kn_conv_narrow_taps.inc (its TapsVec and the forms' slot and tap counts).  convtaps_narrow_kernel's arithmetic, statement for statement --
// input channel outer, the pixel's slots by ascending input pixel inner, t = (coef == 1 ? a : coef * a), product and sum as two roundings, then the bias entry where it is
// stored, then ReLU -- so the result is convtaps_narrow32_kernel's bit for bit.  What differs is what a step fetches and how it multiplies:
//   * the work item is convtaps_narrow32_kernel's: (column block, 64-channel block, output pixel), pixel fastest, dealt to the XCDs in contiguous chunks, one pixel per
//     wavefront, NV (8 | 16 | 32) running sums per lane: the columns c0 = block * NV .. of the pixel.  Which width runs is narrow_choice's NARROW32 rule, unchanged.
//   * per pixel, loaded ONCE and kept in scalar registers, as convtaps_narrow_taps_kernel keeps them: the <= 9 slots' byte offsets inside a channel's plane, their packed
//     4-bit tap indices and, where the operator has them, their coefficients.  Per input channel: the NT = 9 | 16 value rows tapsT[t][ci][cb * 64 + lane] in vector
//     registers, requested one channel ahead, two sets in turn.
//   * a step's NV activations are wave-uniform and arrive through the scalar data cache as ONE segment of W = min(NV, 16) dwords (NV = 32: two), the offset in a scalar
//     register.  Columns (v, v + 1) are then an aligned scalar register PAIR of the segment, which is the operand v_pk_mul_f32 takes next to the term t (one indexed
//     register read into the low half of a vector register pair, which op_sel_hi hands to both columns): NV / 2 packed multiplies and NV / 2 packed adds per step, each element rounded on its own, product then sum.
//   * scalar loads return out of order, so only lgkmcnt(0) separates a load from its use.  TWO segments in turn: behind the wait for segment q the load of segment q + 1
//     (the next step; NV = 32: the step's other half; a channel's last: the next channel's first) is issued IN FRONT OF segment q's multiplies and adds.  32 scalar
//     registers of activations in every form.
// A pixel with fewer slots than the form holds takes wave-uniform branches around the arithmetic of the steps it does not have (their segments are loaded from the pixel's
// first slot and not used) -- never a product 0 * x.  Blocks the batch does not fill (!FULL: widths 9 .. 15, 17 .. 31 and the last block of the others): the segment must
// lie inside the caller's block, tested once per wavefront on the last channel's highest input pixel; the wavefronts that fail fetch column pair by column pair, every column a load of its
// own (the surplus columns from the last real column again).  Surplus sums are never stored.
// No LDS, no barriers, no atomics, no scratch, nothing spilled into vector lanes (tests/test_narrow_taps32_host.py); 32-bit offsets, checked by narrow_choice.
// The two segments live in NAMED scalar registers, s[64:79] and s[80:95] (W = 8: the first eight of each).  Left to the register allocator the sets changed registers
// between the channels of a pair -- copies of a segment that had not landed -- and a column pair was a copy of its own.  With the names in the constraints a load, its
// wait and its multiplies agree on the registers by construction, and the column pair (2 i, 2 i + 1) of a segment is the sub-register pair written in the instruction.
template <int W, int SET>
__device__ __forceinline__ void taps32_load_seg(typename TapsVec<W>::type& x, const float* base, const uint32_t off) {
    static_assert((W == 8 || W == 16) && (SET == 0 || SET == 1), "segment widths, two sets");
    if constexpr (W == 8 && SET == 0) asm volatile("s_load_dwordx8 %0, %1, %2" : "=&{s[64:71]}"(x) : "s"(base), "s"(off));
    else if constexpr (W == 8) asm volatile("s_load_dwordx8 %0, %1, %2" : "=&{s[80:87]}"(x) : "s"(base), "s"(off));
    else if constexpr (SET == 0) asm volatile("s_load_dwordx16 %0, %1, %2" : "=&{s[64:79]}"(x) : "s"(base), "s"(off));
    else asm volatile("s_load_dwordx16 %0, %1, %2" : "=&{s[80:95]}"(x) : "s"(base), "s"(off));
}
template <int W, int SET>
__device__ __forceinline__ void taps32_landed(typename TapsVec<W>::type& x) {      // every outstanding scalar load has landed; the uses of x stay behind
    if constexpr (W == 8 && SET == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+{s[64:71]}"(x));
    else if constexpr (W == 8) asm volatile("s_waitcnt lgkmcnt(0)" : "+{s[80:87]}"(x));
    else if constexpr (SET == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+{s[64:79]}"(x));
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+{s[80:95]}"(x));
}
// pr[i] = (x[2 i], x[2 i + 1]) * (t, t), t the low half of tt: one packed multiply per column pair, two IEEE multiplies each
#define KN_T32_MUL(d, lo, hi, t) "v_pk_mul_f32 %" #d ", s[" #lo ":" #hi "], %" #t " op_sel_hi:[1,0]\n\t"
template <int W, int SET, typename P>
__device__ __forceinline__ void taps32_mul(P (&pr)[W / 2], const typename TapsVec<W>::type& x, const P tt) {
    if constexpr (W == 8 && SET == 0)
        asm volatile(KN_T32_MUL(0, 64, 65, 5) KN_T32_MUL(1, 66, 67, 5) KN_T32_MUL(2, 68, 69, 5) KN_T32_MUL(3, 70, 71, 5)
                     : "=&v"(pr[0]), "=&v"(pr[1]), "=&v"(pr[2]), "=&v"(pr[3]) : "{s[64:71]}"(x), "v"(tt));
    else if constexpr (W == 8)
        asm volatile(KN_T32_MUL(0, 80, 81, 5) KN_T32_MUL(1, 82, 83, 5) KN_T32_MUL(2, 84, 85, 5) KN_T32_MUL(3, 86, 87, 5)
                     : "=&v"(pr[0]), "=&v"(pr[1]), "=&v"(pr[2]), "=&v"(pr[3]) : "{s[80:87]}"(x), "v"(tt));
    else if constexpr (SET == 0)
        asm volatile(KN_T32_MUL(0, 64, 65, 9) KN_T32_MUL(1, 66, 67, 9) KN_T32_MUL(2, 68, 69, 9) KN_T32_MUL(3, 70, 71, 9)
                     KN_T32_MUL(4, 72, 73, 9) KN_T32_MUL(5, 74, 75, 9) KN_T32_MUL(6, 76, 77, 9) KN_T32_MUL(7, 78, 79, 9)
                     : "=&v"(pr[0]), "=&v"(pr[1]), "=&v"(pr[2]), "=&v"(pr[3]), "=&v"(pr[4]), "=&v"(pr[5]), "=&v"(pr[6]), "=&v"(pr[7]) : "{s[64:79]}"(x), "v"(tt));
    else
        asm volatile(KN_T32_MUL(0, 80, 81, 9) KN_T32_MUL(1, 82, 83, 9) KN_T32_MUL(2, 84, 85, 9) KN_T32_MUL(3, 86, 87, 9)
                     KN_T32_MUL(4, 88, 89, 9) KN_T32_MUL(5, 90, 91, 9) KN_T32_MUL(6, 92, 93, 9) KN_T32_MUL(7, 94, 95, 9)
                     : "=&v"(pr[0]), "=&v"(pr[1]), "=&v"(pr[2]), "=&v"(pr[3]), "=&v"(pr[4]), "=&v"(pr[5]), "=&v"(pr[6]), "=&v"(pr[7]) : "{s[80:95]}"(x), "v"(tt));
}
#undef KN_T32_MUL
#pragma clang fp contract(off)
template <int NT, int NV, bool FULL, bool COEF>
__global__ __launch_bounds__(256) void convtaps_narrow_taps32_kernel(ConvArgs p, int n_cb, int n_colb, int64_t n_wg) {
    typedef float taps_t __attribute__((ext_vector_type(TAPS_MAX_TAPS)));
    typedef float pair_t __attribute__((ext_vector_type(2)));
    static_assert(NV == 8 || NV == 16 || NV == 32, "column block widths");
    static_assert(NT <= TAPS_MAX_TAPS && TAPS_MAX_SLOTS <= 16, "tap vector and packed tap indices");
    constexpr int MS = TAPS_MAX_SLOTS;
    constexpr int W = NV < 16 ? NV : 16;                    // dwords of a segment
    constexpr int H = NV / W;                               // segments of a step
    constexpr int NQ = MS * H;                              // segments of a channel
    typedef typename TapsVec<W>::type seg_t;
    const int64_t chunk = (n_wg + 7) >> 3;
    const int64_t wg = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (wg >= n_wg || (blockIdx.x >> 3) >= chunk) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint32_t wi = (uint32_t)wg * 4u + (uint32_t)wave;      // (column block, channel block, pixel in processing order), pixel fastest; below 2^31: checked by the launcher
    const uint32_t per_colb = (uint32_t)p.n_pix * (uint32_t)n_cb;
    if (wi >= per_colb * (uint32_t)n_colb) return;                // (wave-uniform; no barriers in this kernel)
    const int colb = __builtin_amdgcn_readfirstlane((int)(wi / per_colb));      // (the quotients come out of vector instructions; the block's base pointer is a scalar operand)
    const uint32_t wr = wi - (uint32_t)colb * per_colb;
    const int cb = __builtin_amdgcn_readfirstlane((int)(wr / (uint32_t)p.n_pix));
    const int o = __builtin_amdgcn_readfirstlane(p.pix_order[wr - (uint32_t)cb * (uint32_t)p.n_pix]);
    const int co = cb * 64 + lane;
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

    pair_t acc[NV / 2];
#pragma unroll
    for (int v = 0; v < NV / 2; v++) acc[v] = pair_t{0.0f, 0.0f};

    // this lane's value rows: tapsT[t][ci][cb * 64 + lane] (element offsets of 32 bits: checked by the launcher); taps the operator does not have re-read its last one
    // (a tap's offset is formed per channel, one scalar addition and one vector addition in front of its load -- against 9 NV / 2 packed pairs a channel: kept per lane the
    // sixteen offsets were sixteen more vector registers and the widest forms did not fit 128; kept as scalars, hoisted out of the channel loop, they were spilled)
    uint32_t tap_stride = (uint32_t)p.cin_pad * (uint32_t)p.cout_pad, tap_last = (uint32_t)p.ntaps - 1u;
    const float* const tap0 = p.tapsT + cb * 64;            // wave-uniform
    auto rows = [&](taps_t& A, const int ci) {              // the value rows of input channel ci
        const float* const tc = tap0 + (uint32_t)ci * (uint32_t)p.cout_pad;
        asm volatile("" : "+s"(tap_stride), "+s"(tap_last));      // (opaque: the offsets below are this call's)
#pragma unroll
        for (int t = 0; t < NT; t++) A[t] = tc[((uint32_t)t < tap_last ? (uint32_t)t : tap_last) * tap_stride + (uint32_t)lane];
    };
    auto term = [&](const taps_t& A, const int k) {         // step k's term as the reference stores it, in the low half of a register pair
        int idx = (int)((tp[k >> 3] >> (4 * (k & 7))) & 15u);
        asm volatile("" : "+s"(idx));                       // (pinned in front of its step: formed early, the nine terms of a channel are eighteen vector registers)
        const float a = A[idx];                             // scalar index mode, no memory access
        pair_t tt;
        tt.x = COEF ? (cf[k] == 1.0f ? a : cf[k] * a) : a;
        return tt;
    };
    // W columns of a step: the packed multiplies of the segment's register pairs, then the packed adds into sums B .. B + W / 2 - 1 (pinned: volatile)
    auto mac = [&](const seg_t& x, const pair_t tt, auto base, auto set) {
        constexpr int B = decltype(base)::value;
        pair_t pr[W / 2];
        pair_t(&sums)[NV / 2] = acc;                        // (named outside the assembly: an operand alone does not capture it in a generic lambda)
        taps32_mul<W, decltype(set)::value>(pr, x, tt);
#pragma unroll
        for (int i = 0; i < W / 2; i++) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(sums[B + i]) : "v"(pr[i]));
    };
    seg_t x0, x1;                                           // the two segments in turn
    constexpr std::integral_constant<int, 0> S0{};
    constexpr std::integral_constant<int, 1> S1{};
    constexpr std::integral_constant<int, 0> LO{};          // sums 0 .. W / 2 - 1, and those of columns 16 .. (NV = 32)
    constexpr std::integral_constant<int, W / 2> HI{};
    // One input channel, its plane at xc.  On entry its first segment is in flight in set PAR (0: x0); on exit xc is `step` further and the first segment there is in
    // flight, in set (PAR + NQ) & 1.
    auto channel = [&](const taps_t& A, const float*& xc, const int64_t step, auto full, auto par) {
        constexpr bool ALL = decltype(full)::value;
        constexpr int PAR = decltype(par)::value;
        asm volatile("" : "+s"(tp[0]), "+s"(tp[1]));       // (opaque: the indices stay packed -- hoisted out of the channel loop they are a scalar register per slot)
        if constexpr (!ALL) asm volatile("" : "+s"(n));    // (likewise the slot count: hoisted, every step's test is a lane mask in two scalar registers)
#pragma unroll
        for (int k = 0; k < MS; k++) {
            const pair_t tt = term(A, k);
#pragma unroll
            for (int h = 0; h < H; h++) {
                const int q = k * H + h;                    // (a compile-time value once unrolled)
                const bool even = ((PAR + q) & 1) == 0;
                if (q + 1 == NQ) xc += step;
                const float* const nb = xc;                 // the next segment: the next channel's first, this step's other half (NV = 32: columns 16 ..), the next step's
                const uint32_t no = q + 1 == NQ ? xb[0] : (h + 1 < H ? xb[k] + 4u * W : xb[k + 1 < MS ? k + 1 : 0]);
                if (even) {                                 // (one load is in flight at a time: the set that is used next)
                    taps32_landed<W, 0>(x0);
                    taps32_load_seg<W, 1>(x1, nb, no);
                } else {
                    taps32_landed<W, 1>(x1);
                    taps32_load_seg<W, 0>(x0, nb, no);
                }
                if (ALL || k < n) {
                    if constexpr (!ALL) asm volatile("");      // (a branch, not a select per step)
                    if (even) {
                        if (h == 0) mac(x0, tt, LO, S0);
                        else mac(x0, tt, HI, S0);
                    } else {
                        if (h == 0) mac(x1, tt, LO, S1);
                        else mac(x1, tt, HI, S1);
                    }
                }
            }
        }
    };
    const float* const xcol = p.X + colb * NV;              // this column block's activations
    auto walk = [&](auto full) {                            // two sets of value rows in turn: a channel's rows are requested while the channel before it is summed
        taps_t A0, A1;
        const float* xc = xcol;
        const int64_t plane = (int64_t)p.HiWi * p.ldx;
        const int last = p.Cin - 1;
        rows(A0, 0);
        taps32_load_seg<W, 0>(x0, xc, xb[0]);
        for (int ci = 0; ci + 1 < p.Cin; ci += 2) {         // channel pairs: 2 NQ segments, so every pair finds its first one in x0
            rows(A1, ci + 1);
            channel(A0, xc, plane, full, std::integral_constant<int, 0>{});
            rows(A0, ci + 2 < last ? ci + 2 : last);
            channel(A1, xc, ci + 2 <= last ? plane : 0, full, std::integral_constant<int, NQ & 1>{});      // (behind the last channel: its first segment again -- loaded, not used)
        }
        taps32_landed<W, 0>(x0);                            // (nothing in flight across the branch below: a segment carried over it was copied while in flight)
        if (p.Cin & 1) {                                    // an odd channel count: the last one on its own, its first segment requested again
            taps32_load_seg<W, 0>(x0, xc, xb[0]);
            channel(A0, xc, 0, full, std::integral_constant<int, 0>{});
            if constexpr (NQ & 1) taps32_landed<W, 1>(x1);
            else taps32_landed<W, 0>(x0);
        }
    };
    // !FULL, a wavefront whose farthest segment would leave the caller's block (without a homogeneous row behind the activations: the pixels whose window holds the last
    // input pixel, in the last column block): one column PAIR at a time, every column a load of its own, the surplus ones of the last real column again
    auto walk_cols = [&](uint32_t lastb) {
        taps_t A;
        const float* xc = xcol;
        const int64_t plane = (int64_t)p.HiWi * p.ldx;
        pair_t(&sums)[NV / 2] = acc;
        for (int ci = 0; ci < p.Cin; ci++) {
            rows(A, ci);
            asm volatile("" : "+s"(tp[0]), "+s"(tp[1]));
            asm volatile("" : "+s"(n), "+s"(lastb));   // (... and the column offsets: hoisted they are a scalar register per column and slot)
#pragma unroll
            for (int k = 0; k < MS; k++) {
                if (k < n) {
                    asm volatile("");
                    const pair_t tt = term(A, k);
#pragma unroll
                    for (int i = 0; i < NV / 2; i++) {
                        int xa, xz;
                        pair_t pr;
                        asm volatile("s_load_dword %0, %1, %2" : "=&{s64}"(xa) : "s"(xc), "s"(xb[k] + (8u * i < lastb ? 8u * i : lastb)));
                        asm volatile("s_load_dword %0, %1, %2" : "=&{s65}"(xz) : "s"(xc), "s"(xb[k] + (8u * i + 4u < lastb ? 8u * i + 4u : lastb)));
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+{s64}"(xa), "+{s65}"(xz));
                        asm volatile("v_pk_mul_f32 %0, s[64:65], %3 op_sel_hi:[1,0]" : "=v"(pr) : "{s64}"(xa), "{s65}"(xz), "v"(tt));
                        asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(sums[i]) : "v"(pr));
                    }
                }
            }
            xc += plane;
        }
    };
    bool segs = true;
    if constexpr (!FULL) {
        uint32_t xb_max = 0;
#pragma unroll
        for (int k = 0; k < MS; k++) xb_max = xb[k] > xb_max ? xb[k] : xb_max;
        const int64_t far = (int64_t)(p.Cin - 1) * p.HiWi * p.ldx + (int64_t)(xb_max >> 2) + colb * NV + NV;
        segs = far <= (p.last_in_row - (p.lastcol ? 0 : 1)) * p.ldx + p.n_vecs;
    }
    if (segs) {
        if (all_full) walk(std::true_type{});
        else walk(std::false_type{});
    } else {
        if constexpr (!FULL) {
            const int nh0 = p.n_vecs - colb * NV < NV ? p.n_vecs - colb * NV : NV;
            walk_cols(4u * (uint32_t)(nh0 - 1));
        }
    }

    // The epilogue reads its arguments from the kernel argument segment AGAIN (ConvArgs is the first parameter: offset 0), through a pointer the compiler cannot see
    // through, as convtaps_narrow_taps_kernel's does: kept live across the walk they are a dozen scalar registers.
    typedef const ConvArgs __attribute__((address_space(4))) * kargs_t;
    kargs_t e = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(e));
    if (co >= e->Cout) return;
    const float* const lastcol = e->lastcol;
    const int c0 = colb * NV;                               // first column of this block, and how many of its NV columns the batch holds
    const int nh = FULL ? NV : (e->n_vecs - c0 < NV ? e->n_vecs - c0 : NV);
    const int64_t row = (int64_t)co * e->HoWo + o;
    if (lastcol) {
        const float lc = lastcol[row];
        if (lc != 0.0f) {                                   // the bias entry exists in the reference's row only when it is stored
            const float* const xl = e->X + e->last_in_row * e->ldx + c0;
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const float bp = lc * xl[(FULL || v < nh) ? v : nh - 1];
                acc[v >> 1][v & 1] = acc[v >> 1][v & 1] + bp;
            }
        }
    }
    float* const yr = e->Y + row * e->ldy + c0;
    const int relu = e->relu;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        float t = acc[v >> 1][v & 1];
        if (relu) t = (t < 0.0f) ? 0.0f : t;
        if (FULL || v < nh) yr[v] = t;
    }
}
