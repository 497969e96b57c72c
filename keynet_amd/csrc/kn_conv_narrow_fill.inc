// ---- order-preserving path for 1 .. 32 batch columns on FILLED-IN operators (KN_FLAG_NARROW_FILL next to KN_FLAG_NARROW [| KN_FLAG_NARROW32]): lanes are OUTPUT CHANNELS ----------
// Included by kn_conv.hip (namespace kn, behind convtaps_narrow_taps_kernel, whose scalar-load helpers it uses).  convtaps_narrow_kernel<DUPS>'s arithmetic, statement for
// statement -- input channel outer, the pixel's slots by ascending input pixel inner, the term of a slot coef * tap, the terms of one (output, input) pixel pair summed in
// entry order into ONE stored value, on the pair's last slot pr = value * x[v]; acc[v] = acc[v] + pr, then the bias entry where it is stored, then ReLU -- so the result
// is that kernel's bit for bit.  What differs is what a slot FETCHES: that kernel loads three slot records and a 256-byte value row per (input channel, slot) and forms two
// addresses.  Here the two halves of convtaps_exact_fill_kernel<TREG> and convtaps_narrow_taps_kernel meet:
//   * a wavefront owns one output pixel x 64 output channels (lane = channel) x NV (1 | 2 | 4 | 8) running sums (the images of its column block);
//   * the pixel's slots are its FillRec list {input pixel, tap index, coefficient, first | last slot of its stored column} (convtaps_fill_records_kernel), the same for
//     every input channel: streamed in batches of B records (4; 2 at NV = 4 | 8, where the activations need the scalar registers) by ONE scalar load per batch, one batch ahead;
//   * per input channel, loaded ONCE into 16 vector registers: the value rows tapsT[t][ci][cb * 64 + lane] of every tap (taps the operator does not have re-read its last
//     one), requested one channel ahead of their use (two register sets in turn).  A slot picks its tap by the scalar index mode: no value-row load per slot;
//   * the activations of a stored column -- NV contiguous floats, wave-uniform -- are ONE scalar load, issued for the record whose `first` flag is set, a batch ahead of
//     the batch that uses them;
//   * a slot is then one indexed register read, one multiply, one add; a stored column's last slot adds NV multiply / add pairs.
// The coefficient is always multiplied (1.0f * a is a, bit for bit: one form for operators with coefficients and without).
// A stored value starts from +0.0 (`ar` is 0 behind every column's last slot and at the head of every input channel) where convtaps_narrow_kernel starts from the first
// term: the same value but for the sign of a zero, which no running sum that starts at +0.0 can show (convtaps_exact_fill_kernel's argument).
// PADDING.  The lists are padded to a multiple of 8 records {0, 0, 0.0f, 0}.  A padding record is neither first nor last: it issues NO activation load and commits NOTHING
// to the running sums, so a non-finite activation reaches no output through it.  What it does is add 0.0f * tap0 to `ar`, which nobody reads: the padding stands behind the
// pixel's last column, and `ar` is set to 0 again at the head of the next input channel (so even a non-finite value row cannot leak into the next channel's first column).
// A pixel with an empty list walks nothing: its bias product, or 0.
// Widths between the forms run the next NV (!FULL): where the segment of NV floats would leave the caller's block (tested once per wavefront, on the last channel's highest
// input pixel of this pixel) the columns are fetched one by one, the surplus ones reading the last real column again; surplus sums are not stored.
// 9 .. 32 columns (KN_FLAG_NARROW32): NV = 8 with the column block as the slowest part of the work item; every block forms the stored values again.
// Work items are (column block, channel block, pixel) with the PIXEL fastest, dealt to the XCDs in contiguous chunks; the pixels go by pix_deal (slot-weighted, heavy first):
// the lists of a filled-in operator differ by 4x between border and interior pixels, and a chunk of pix_order ends on its heaviest ones.
// No scalar load is in flight across a loop's back edge (every half body ends on its wait).  No LDS, no barriers, no atomics, no scratch, nothing spilled into vector lanes
// (tests/test_narrow_fill_host.py).
template <int B> struct FillBatch { typedef int type __attribute__((ext_vector_type(4 * B))); };
template <int B>
__device__ __forceinline__ void fill_load_recs(typename FillBatch<B>::type& R, const uint64_t base, const uint32_t off) {
    if constexpr (B == 4) asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(R) : "s"(base), "s"(off));
    else if constexpr (B == 1) asm volatile("s_load_dwordx4 %0, %1, %2" : "=&s"(R) : "s"(base), "s"(off));
    else asm volatile("s_load_dwordx8 %0, %1, %2" : "=&s"(R) : "s"(base), "s"(off));
}
// (the destination is a read-write operand: the load stands inside a wave-uniform branch, and a register the branch leaves alone keeps its -- unused -- content)
template <int NV>
__device__ __forceinline__ void fill_load_seg(typename TapsVec<NV>::type& x, const uint64_t base, const uint32_t off) {
    if constexpr (NV == 1) asm volatile("s_load_dword %0, %1, %2" : "+s"(x) : "s"(base), "s"(off));
    else if constexpr (NV == 2) asm volatile("s_load_dwordx2 %0, %1, %2" : "+s"(x) : "s"(base), "s"(off));
    else if constexpr (NV == 4) asm volatile("s_load_dwordx4 %0, %1, %2" : "+s"(x) : "s"(base), "s"(off));
    else asm volatile("s_load_dwordx8 %0, %1, %2" : "+s"(x) : "s"(base), "s"(off));
}
__device__ __forceinline__ void fill_load_col(int& x, const uint64_t base, const uint32_t off) { asm volatile("s_load_dword %0, %1, %2" : "+s"(x) : "s"(base), "s"(off)); }

#pragma clang fp contract(off)
template <int NV, bool FULL>
__global__ __launch_bounds__(256) void convtaps_narrow_fill_kernel(ConvArgs p, const int32_t* __restrict__ fill_ptr, const FillRec* __restrict__ rec, int n_cb, int n_colb, int64_t n_wg) {
    typedef float taps_t __attribute__((ext_vector_type(16)));
    typedef typename TapsVec<NV>::type xseg_t;
    constexpr int B = NV >= 4 ? 2 : 4;                      // records per batch (NV = 4 with 4 spilled scalar registers into vector lanes)
    const int64_t chunk = (n_wg + 7) >> 3;
    const int64_t wg = (int64_t)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    if (wg >= n_wg || (blockIdx.x >> 3) >= chunk) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint32_t wi = (uint32_t)wg * 4u + (uint32_t)wave;      // (column block, channel block, pixel in processing order), pixel fastest; below 2^31: checked by the launcher
    const uint32_t per = (uint32_t)p.n_pix * (uint32_t)n_cb;
    if (wi >= per * (uint32_t)n_colb) return;                     // (wave-uniform; no barriers in this kernel)
    const int colb = __builtin_amdgcn_readfirstlane((int)(wi / per));      // (the quotients come out of the vector unit: uniform, and in scalar registers from here on)
    const uint32_t wr = wi - (uint32_t)colb * per;
    const int cb = __builtin_amdgcn_readfirstlane((int)(wr / (uint32_t)p.n_pix));
    const int o = __builtin_amdgcn_readfirstlane(p.pix_order[wr - (uint32_t)cb * (uint32_t)p.n_pix]);
    const int r_beg = __builtin_amdgcn_readfirstlane(fill_ptr[o]);
    const int n_pad = __builtin_amdgcn_readfirstlane(fill_ptr[o + 1]) - r_beg;      // multiple of 8
    const int co = cb * 64 + lane;
    const int col0 = colb * NV;                             // first column of this block
    const int nvh = FULL ? NV : (p.n_vecs - col0 < NV ? p.n_vecs - col0 : NV);      // columns of this block that exist

    float acc[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) acc[v] = 0.0f;

    if (n_pad > 0) {
        const uint32_t ldxb = (uint32_t)p.ldx * 4u;         // (4 * (HiWi * ldx + 32) < 2^32: checked by narrow_choice)
        const uint32_t lastb = 4u * (uint32_t)(nvh - 1);    // byte offset of the block's last real column: what the surplus sums of a width below NV read (column by column)
        // this lane's value rows: element offsets of the taps inside the channel block's share of tapsT (32 bits: checked by the launcher)
        uint32_t to[16];
#pragma unroll
        for (int t = 0; t < 16; t++) to[t] = (uint32_t)(t < p.ntaps ? t : p.ntaps - 1) * ((uint32_t)p.cin_pad * (uint32_t)p.cout_pad) + (uint32_t)lane;
        const float* const tap0 = p.tapsT + cb * 64;        // wave-uniform
        auto rows = [&](taps_t& A, const int ci) {          // the value rows of input channel ci
            const float* const tc = tap0 + (uint32_t)ci * (uint32_t)p.cout_pad;
#pragma unroll
            for (int t = 0; t < 16; t++) A[t] = tc[to[t]];
        };
        const uint32_t list_bytes = 16u * (uint32_t)n_pad;
        const uint64_t plane = 4ull * (uint64_t)((int64_t)p.HiWi * p.ldx);      // bytes between the planes of two input channels
        // the fetch cursors (wave-uniform): the batch whose records are loaded next (byte offset inside the list; behind the last batch: the first again), and the batch whose
        // activations are requested next (batches left in its input channel, that channel's plane of X; behind the last channel: the last channel again, loaded and not used)
        auto uni = [](const uint64_t v) {                   // (a pointer the scalar loads take as their base: in scalar registers by construction)
            return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        };
        const uint64_t rbase = uni(reinterpret_cast<uint64_t>(rec + r_beg));
        uint32_t rq = 0;
        int xci_left = p.Cin - 1;
        uint64_t xq = uni(reinterpret_cast<uint64_t>(p.X + col0));
        float ar = 0.0f;                                    // the stored value being formed
        xseg_t xcur = xseg_t{};                             // ... and the activations of its column

        auto walk = [&](auto seg) {
            constexpr bool SEG = decltype(seg)::value;
            constexpr int BW = SEG ? B : 8 / NV;               // records per batch of this walk (column by column: 8 registers per batch, or the widest form spills)
            typedef typename FillBatch<BW>::type recs_t;
            const int nb = n_pad / BW;                      // batches per input channel (even)
            int xq_left = nb;
            recs_t R0, R1;
            xseg_t X0[BW], X1[BW];                            // SEG: the activation segments of a batch's stored columns
            int C0[BW][NV], C1[BW][NV];                       // !SEG: the same, column by column
#pragma unroll
            for (int k = 0; k < BW; k++) {
                X0[k] = xseg_t{};
                X1[k] = xseg_t{};
#pragma unroll
                for (int v = 0; v < NV; v++) C0[k][v] = C1[k][v] = 0;
            }
            auto load_recs = [&](recs_t& R) {
                fill_load_recs<BW>(R, rbase, rq);
                rq = (rq + 16u * BW == list_bytes) ? 0u : rq + 16u * BW;
            };
            auto request = [&](const recs_t& R, xseg_t (&X)[BW], int (&C)[BW][NV]) {      // the activations of the stored columns that begin in batch R (landed)
#pragma unroll
                for (int k = 0; k < BW; k++) {
                    if (R[4 * k + 3] & 1) {
                        const uint32_t off = (uint32_t)R[4 * k] * ldxb;
                        if constexpr (SEG) {
                            fill_load_seg<NV>(X[k], xq, off);
                        } else {
#pragma unroll
                            for (int v = 0; v < NV; v++) fill_load_col(C[k][v], xq, off + (4u * v < lastb ? 4u * v : lastb));
                        }
                    }
                }
                if (--xq_left == 0) {
                    xq_left = nb;
                    if (xci_left > 0) {
                        xci_left--;
                        xq += plane;
                    }
                }
            };
            auto landed = [&](recs_t& R, xseg_t (&X)[BW], int (&C)[BW][NV]) {       // every scalar load issued so far: the records R and the activations X / C
                if constexpr (SEG) {
                    if constexpr (BW == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(R), "+s"(X[0]), "+s"(X[1]), "+s"(X[2]), "+s"(X[3]));
                    else if constexpr (BW == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(R), "+s"(X[0]));
                    else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(R), "+s"(X[0]), "+s"(X[1]));
                } else {
                    int* const c = &C[0][0];
                    static_assert(SEG || BW * NV == 8, "the column-by-column walk waits on 8 registers per batch");
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(R), "+s"(c[0]), "+s"(c[1]), "+s"(c[2]), "+s"(c[3]), "+s"(c[4]), "+s"(c[5]), "+s"(c[6]), "+s"(c[7]));
                }
            };
            auto slots = [&](const taps_t& A, const recs_t& R, const xseg_t (&X)[BW], const int (&C)[BW][NV]) {      // the BW slots of a landed batch
#pragma unroll
                for (int k = 0; k < BW; k++) {
                    const int tp = R[4 * k + 1], cbits = R[4 * k + 2], fl = R[4 * k + 3];
                    const float a = A[tp];                  // scalar index mode, no memory access
                    const float t = __builtin_bit_cast(float, cbits) * a;       // the term as the reference stores it (coef == 1: the tap itself)
                    ar = ar + t;
                    if (fl & 1) {
                        if constexpr (SEG) {
                            xcur = X[k];
                        } else if constexpr (NV > 1) {      // (the widths 1 and 2 always fill their form)
#pragma unroll
                            for (int v = 0; v < NV; v++) xcur[v] = C[k][v];
                        }
                    }
                    if (fl & 2) {
                        asm volatile("");                   // (a branch, not selects on every slot)
#pragma unroll
                        for (int v = 0; v < NV; v++) {
                            int xi;                         // (the element as a value first: a bit cast of the vector element itself reads element 0)
                            if constexpr (NV == 1) xi = xcur;
                            else xi = xcur[v];
                            const float pr = ar * __builtin_bit_cast(float, xi);
                            acc[v] = acc[v] + pr;
                        }
                        ar = 0.0f;
                    }
                }
            };
            auto channel = [&](const taps_t& A) {          // one input channel's slots.  In: R0 = its first batch and X0 / C0 landed, R1 = the batch behind it landed.  Out: the same one channel on
                ar = 0.0f;
                for (int b = 0; b < nb; b += 2) {
                    request(R1, X1, C1);
                    slots(A, R0, X0, C0);
                    load_recs(R0);
                    landed(R0, X1, C1);
                    request(R0, X0, C0);
                    slots(A, R1, X1, C1);
                    load_recs(R1);
                    landed(R1, X0, C0);
                }
            };
            // prologue: the first batch's records and activations, the second batch's records
            load_recs(R0);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(R0));
            load_recs(R1);
            request(R0, X0, C0);
            landed(R1, X0, C0);
            // two sets of value rows in turn: a channel's rows are requested while the channel before it is summed
            taps_t A0, A1;
            const int last = p.Cin - 1;
            rows(A0, 0);
            for (int ci = 0; ci < p.Cin; ci += 2) {
                rows(A1, ci + 1 < last ? ci + 1 : last);
                channel(A0);
                if (ci + 1 >= p.Cin) break;
                rows(A0, ci + 2 < last ? ci + 2 : last);
                channel(A1);
            }
        };
        // A stored column's activations are ONE segment of NV floats.  Where the batch does not fill the form (!FULL) the segment must still lie inside the caller's block:
        // tested once per wavefront on the last channel's highest input pixel of this pixel (its last real record: the lists ascend), as convtaps_narrow_taps_kernel does.
        bool segs = true;
        if constexpr (!FULL) {
            const int n_real = __builtin_amdgcn_readfirstlane(p.pix_ptr[o + 1]) - __builtin_amdgcn_readfirstlane(p.pix_ptr[o]);
            const int in_max = __builtin_amdgcn_readfirstlane(rec[r_beg + n_real - 1].in);
            const int64_t far = ((int64_t)(p.Cin - 1) * p.HiWi + in_max) * p.ldx + col0 + NV;
            segs = far <= (p.last_in_row - (p.lastcol ? 0 : 1)) * p.ldx + p.n_vecs;
        }
        if (segs) walk(std::true_type{});
        else if constexpr (!FULL) walk(std::false_type{});
    }

    // The epilogue reads its arguments from the kernel argument segment AGAIN (ConvArgs is the first parameter: offset 0), through a pointer the compiler cannot see
    // through, as convtaps_narrow_taps_kernel's does: kept live across the walk they are a dozen scalar registers.
    typedef const ConvArgs __attribute__((address_space(4))) * kargs_t;
    kargs_t e = (kargs_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(e));
    if (co >= e->Cout) return;
    const int64_t row = (int64_t)co * e->HoWo + o;
    const float* const lastcol = e->lastcol;
    if (lastcol) {
        const float lc = lastcol[row];
        if (lc != 0.0f) {                                   // the bias entry exists in the reference's row only when it is stored
            const float* const xl = e->X + e->last_in_row * e->ldx + col0;
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const float bp = lc * xl[(FULL || v < nvh) ? v : nvh - 1];
                acc[v] = acc[v] + bp;
            }
        }
    }
    float* const yr = e->Y + row * e->ldy + col0;
    const int relu = e->relu;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        float t = acc[v];
        if (relu) t = (t < 0.0f) ? 0.0f : t;
        if (FULL || v < nvh) yr[v] = t;
    }
}
