// The body of convtaps_exact_pipe_kernel and convtaps_exact_pipe64_kernel (kn_conv.hip includes it inside both: two entry points over one text, so neither kernel's
// code depends on how a shared function would be inlined).  In scope: the template parameters RBX, COEF, XD, VEC and the kernel parameters p, n_cob, n_rb.
    constexpr int NP = VEC / 2;                                           // column pairs per lane
    typedef float xvec_t __attribute__((ext_vector_type(VEC == 1 ? 2 : VEC)));
    typedef typename std::conditional<VEC == 1, float, xvec_t>::type xrow_t;     // what a lane loads of an activation row
    const int64_t n_ct = (p.n_vecs + 64 * VEC - 1) / (64 * VEC);
    const int64_t n_items = n_ct * n_rb;
    const int64_t chunk = (n_items + 7) >> 3;
    const int64_t xl = blockIdx.x & 7;
    const int64_t item = xl * chunk + (blockIdx.x >> 3);
    if (item >= ((xl + 1) * chunk < n_items ? (xl + 1) * chunk : n_items)) return;
    const int64_t ct = item / n_rb;
    const int64_t rb = item - ct * n_rb;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t w = rb * 4 + wave;
    if (w >= (int64_t)p.n_pix * n_cob) return;
    // wave-uniform by construction; pinned to SGPRs here so that the whole step-advance logic below stays on the scalar ALU (a value
    // that comes out of a vector-memory load counts as divergent for the compiler, and would drag the loop counters into VGPRs)
    // w -> (channel-bundle group, pixel, bundle inside the group), bundle fastest: the bundles of a pixel that run side by side share its gathered
    // activation rows in L2.  G = p.tail_main bundles per group (0 = all n_cob: one group).  With G = n_cob / 8 every XCD's contiguous share of the
    // items is ONE group over all pixels, so its slice of the taps (1/8 of 9.4 MB on the 512-channel layers) stays L2-resident for the scalar loads.
    const int G = p.tail_main > 0 ? p.tail_main : n_cob;
    const int64_t per_group = (int64_t)p.n_pix * G;
    const int cg = (int)(w / per_group);
    const int64_t rem = w - (int64_t)cg * per_group;
    const int o = __builtin_amdgcn_readfirstlane(p.pix_order[rem / G]);
    const int co0 = __builtin_amdgcn_readfirstlane((cg * G + (int)(rem % G)) * RBX);
    const int s_beg = __builtin_amdgcn_readfirstlane(p.pix_ptr[o]);
    const int n_slots = __builtin_amdgcn_readfirstlane(p.pix_ptr[o + 1]) - s_beg;
    const int64_t c = ct * (64 * VEC) + (int64_t)lane * VEC;
    const bool active = c < p.n_vecs;
    const uint32_t lane_off_bytes = 4u * (uint32_t)(active ? c : 0);      // byte offset: (uniform base) + zext(VGPR) selects the saddr load form

    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int NA = VEC == 1 ? RBX / 2 : RBX, NPA = VEC == 1 ? 1 : NP;
    f32x2 acc[NA][NPA];                                                   // [output channel][columns 0-1 | 2-3]; VEC = 1: [channel pair r / 2][0], halves = channels r, r + 1
#pragma unroll
    for (int r = 0; r < NA; r++)
#pragma unroll
        for (int h = 0; h < NPA; h++) acc[r][h] = f32x2{0.f, 0.f};

    if (n_slots > 0) {
        // lane s: element offsets of slot s (32-bit: the launcher checks the ranges)
        int my_xoff = 0, my_aoff = 0;
        float my_coef = 1.0f;                                     // COEF: lane s = coefficient of slot s
        if (lane < n_slots) {
            my_xoff = p.slot_in[s_beg + lane] * (int)p.ldx;
            my_aoff = p.slot_tap[s_beg + lane] * (p.cin_pad * p.cout_pad);
            if constexpr (COEF) my_coef = p.slot_coef[s_beg + lane];
        }
        const int ch_x = __builtin_amdgcn_readfirstlane(p.HiWi * (int)p.ldx);      // one input channel of X
        const float* a_base = p.tapsT + co0;
        const int n_q = n_slots * p.Cin;
        // two wave-uniform cursors over the steps (slot inner, channel outer): the activation rows may run further ahead than the tap values
        int s = 0, ci_x = 0, q_next = 0;                         // cursor of the activation-row requests
        int s_a = 0, ci_a = 0, q_a = 0;                          // cursor of the tap-value requests
        // Operand fetch of one step, written as inline asm so that both addresses stay scalar: the activation row is a saddr-form vector
        // load (wave-uniform 64-bit base in SGPRs + the lane's constant byte offset: no per-step vector address arithmetic), the step's
        // RBX tap values one s_load into an SGPR tuple that the packed multiplies read directly.  The compiler's waitcnt bookkeeping does
        // not see these loads; the waits are written out below.  Each fetch advances its cursor, branch-free (selects on wave-uniform
        // values, all on the scalar ALU); past the end the last step's operands are fetched again, so the waits stay counted ones.
        typedef float taps_t __attribute__((ext_vector_type(RBX)));
        auto fetch_x = [&](xrow_t& xr) {
            const int xo = __builtin_amdgcn_readlane(my_xoff, s) + ci_x;
            const uint64_t xaddr = reinterpret_cast<uint64_t>(p.X + xo);
            if constexpr (VEC == 4) asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(xr) : "v"(lane_off_bytes), "s"(xaddr));
            else if constexpr (VEC == 2) asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(xr) : "v"(lane_off_bytes), "s"(xaddr));
            else asm volatile("global_load_dword %0, %1, %2" : "=&v"(xr) : "v"(lane_off_bytes), "s"(xaddr));
            q_next++;
            const bool more = q_next < n_q;
            const bool wrap = (s + 1 == n_slots);
            s = more ? (wrap ? 0 : s + 1) : s;
            ci_x = __builtin_amdgcn_readfirstlane(ci_x + ((more && wrap) ? ch_x : 0));
        };
        auto fetch_a = [&](taps_t& ar, float& cf) {
            const int ao = __builtin_amdgcn_readlane(my_aoff, s_a) + ci_a;
            const uint64_t aaddr = reinterpret_cast<uint64_t>(a_base + ao);
            if constexpr (RBX == 16) asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(ar) : "s"(aaddr));
            else asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=&s"(ar) : "s"(aaddr));
            if constexpr (COEF) cf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_coef), s_a));
            q_a++;
            const bool more = q_a < n_q;
            const bool wrap = (s_a + 1 == n_slots);
            s_a = more ? (wrap ? 0 : s_a + 1) : s_a;
            ci_a = ci_a + ((more && wrap) ? p.cout_pad : 0);
        };
        auto advance = [&]() {};                                 // (the fetches advance their own cursors)
        // the "+" operands make the multiplies that follow depend on the wait
        auto taps_landed = [&](taps_t& ar) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ar)); };
        auto row_landed = [&](xrow_t& xr, auto younger) {                 // vector loads return in order
            asm volatile("s_waitcnt vmcnt(%1)" : "+v"(xr) : "n"(decltype(younger)::value));
        };
        // acc[r] += x * av[r] (separate IEEE multiply and add).  The packed multiply reads an aligned SGPR pair and broadcasts its low
        // or high half with op_sel, so one pair serves two output channels.  The instruction order is pinned (volatile asm): the four
        // multiplies of channel pair k are followed by the four adds of pair k-1, so no add waits on the multiply right in front of it
        // (left to itself the scheduler serialises "mul, add, mul, add" through one temporary in the second half of the loop body).
        // mul4: the four products of ONE channel pair (VEC = 4: two column pairs x two channels) or of TWO channel pairs (VEC = 2: one column pair x
        // four channels); add4 adds them to their running sums.  `r` is the first of the 2 (VEC = 4) or 4 (VEC = 2) channels a call covers.
        auto mul4 = [&](const f32x2& xlo, const f32x2& xhi, const f32x2& a2, const f32x2& b2, f32x2 (&pr)[4]) {
            if constexpr (VEC == 4) {
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[0]) : "v"(xlo), "s"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[1]) : "v"(xhi), "s"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[2]) : "v"(xlo), "s"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[3]) : "v"(xhi), "s"(a2));
            } else {
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[0]) : "v"(xlo), "s"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[1]) : "v"(xlo), "s"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[2]) : "v"(xlo), "s"(b2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[3]) : "v"(xlo), "s"(b2));
            }
        };
        auto add4 = [&](int r, const f32x2 (&pr)[4]) {
            if constexpr (VEC == 4) {
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r][0]) : "v"(pr[0]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r][NP - 1]) : "v"(pr[1]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r + 1][0]) : "v"(pr[2]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r + 1][NP - 1]) : "v"(pr[3]));
            } else {
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r][0]) : "v"(pr[0]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r + 1][0]) : "v"(pr[1]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r + 2][0]) : "v"(pr[2]));
                asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(acc[r + 3][0]) : "v"(pr[3]));
            }
        };
        // COEF (float keys whose entries carry a coefficient): the stored non-zero of the reference is fl(coef * tap) -- one more packed
        // multiply per channel pair, tap pair (SGPR) x the step's coefficient (broadcast from a VGPR pair's low half), and the products
        // are then formed from that VGPR pair.
        auto mul4v = [&](const f32x2& xlo, const f32x2& xhi, const f32x2& a2, const f32x2& b2, f32x2 (&pr)[4]) {
            if constexpr (VEC == 4) {
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[0]) : "v"(xlo), "v"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[1]) : "v"(xhi), "v"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[2]) : "v"(xlo), "v"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[3]) : "v"(xhi), "v"(a2));
            } else {
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[0]) : "v"(xlo), "v"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[1]) : "v"(xlo), "v"(a2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(pr[2]) : "v"(xlo), "v"(b2));
                asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(pr[3]) : "v"(xlo), "v"(b2));
            }
        };
        // VEC = 1: one packed multiply and one packed add per CHANNEL PAIR.  mulp: pr = {x * a[r], x * a[r + 1]} -- the activation's low half to both halves (op_sel_hi 0 on
        // that source), the tap pair straight, from SGPRs or (COEF) from the VGPR pair fl(coef * tap); addp adds it to the pair's running sums.  Pinned order as above: the
        // multiplies of a group of four pairs are followed by the adds of the group before it.
        auto mulp = [&](const f32x2& x2, const f32x2& a2, f32x2& pr) { asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(pr) : "v"(x2), "s"(a2)); };
        auto mulpv = [&](const f32x2& x2, const f32x2& a2, f32x2& pr) { asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(pr) : "v"(x2), "v"(a2)); };
        auto addp = [&](f32x2& sum, const f32x2& pr) { asm volatile("v_pk_add_f32 %0, %1, %0" : "+v"(sum) : "v"(pr)); };
        auto mac1 = [&](const float xs, const taps_t& av, const float cf) {
            f32x2 x2;                                                    // (high half left unset: op_sel_hi never reads it)
            x2[0] = xs;
            f32x2 pr[RBX / 2];
            const f32x2 cf2 = {cf, cf};
#pragma unroll
            for (int g = 0; g < RBX / 2; g += 4) {
                if constexpr (COEF) {
                    f32x2 sa[4];                                         // the group's stored values fl(coef * tap)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(sa[k]) : "s"(f32x2{av[2 * (g + k)], av[2 * (g + k) + 1]}), "v"(cf2));
#pragma unroll
                    for (int k = 0; k < 4; k++) mulpv(x2, sa[k], pr[g + k]);
                } else {
#pragma unroll
                    for (int k = g; k < g + 4; k++) mulp(x2, f32x2{av[2 * k], av[2 * k + 1]}, pr[k]);
                }
                if (g > 0) {
#pragma unroll
                    for (int k = g - 4; k < g; k++) addp(acc[k][0], pr[k]);
                }
            }
#pragma unroll
            for (int k = RBX / 2 - 4; k < RBX / 2; k++) addp(acc[k][0], pr[k]);
        };
        auto mac = [&](const xrow_t& xv, const taps_t& av, const float cf) {
            if constexpr (VEC == 1) {
                mac1(xv, av, cf);
            } else {
            const f32x2 xlo = {xv[0], xv[1]}, xhi = {xv[VEC - 2], xv[VEC - 1]};
            f32x2 pa[4], pb[4];
            constexpr int CH = (VEC == 4) ? 2 : 4;                       // channels per mul4 / add4
            if constexpr (COEF) {
                const f32x2 cf2 = {cf, cf};
                f32x2 sa, sb, sc, sd;
#pragma unroll
                for (int r = 0; r < RBX; r += 2 * CH) {
                    asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(sa) : "s"(f32x2{av[r], av[r + 1]}), "v"(cf2));
                    asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(sb) : "s"(f32x2{av[r + 2], av[r + 3]}), "v"(cf2));
                    if constexpr (VEC == 2) {
                        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(sc) : "s"(f32x2{av[r + 4], av[r + 5]}), "v"(cf2));
                        asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(sd) : "s"(f32x2{av[r + 6], av[r + 7]}), "v"(cf2));
                    }
                    if (r > 0) add4(r - CH, pb);
                    if constexpr (VEC == 4) {
                        mul4v(xlo, xhi, sa, sa, pa);
                        mul4v(xlo, xhi, sb, sb, pb);
                    } else {
                        mul4v(xlo, xhi, sa, sb, pa);
                        mul4v(xlo, xhi, sc, sd, pb);
                    }
                    add4(r, pa);
                }
                add4(RBX - CH, pb);
                return;
            }
#pragma unroll
            for (int r = 0; r < RBX; r += 2 * CH) {
                if constexpr (VEC == 4) mul4(xlo, xhi, f32x2{av[r], av[r + 1]}, f32x2{av[r], av[r + 1]}, pa);
                else mul4(xlo, xhi, f32x2{av[r], av[r + 1]}, f32x2{av[r + 2], av[r + 3]}, pa);
                if (r > 0) add4(r - CH, pb);
                if constexpr (VEC == 4) mul4(xlo, xhi, f32x2{av[r + 2], av[r + 3]}, f32x2{av[r + 2], av[r + 3]}, pb);
                else mul4(xlo, xhi, f32x2{av[r + 4], av[r + 5]}, f32x2{av[r + 6], av[r + 7]}, pb);
                add4(r, pa);
            }
            add4(RBX - CH, pb);
            }
        };
        // Two steps per trip, operands double-buffered.  Step q+1's tap load is issued right after step q's taps have landed (scalar
        // loads return out of order, so lgkmcnt can only be waited to zero) and its activation row right after that; both have step q's
        // 2*RBX packed multiplies / adds to land.  kn_order() keeps the compiler from moving the arithmetic across the fetches.
        if constexpr (XD == 4) {
            // FOUR activation rows in flight (wide batches: a gathered row of a [D, 4096] block misses L2 -- the grouped CSR pipeline's finding),
            // tap values one step ahead as before.  One step: this step's taps have landed -> request the next step's -> wait for this step's
            // row (three younger rows stay in flight) -> arithmetic -> request the row four steps ahead into the register just released.
            xrow_t x0, x1, x2, x3;
            taps_t a0, a1;
            float c0 = 1.0f, c1 = 1.0f;
            fetch_x(x0);
            fetch_x(x1);
            fetch_x(x2);
            fetch_x(x3);
            fetch_a(a0, c0);
            auto step4 = [&](const int q, xrow_t& xq, taps_t& aq, float& cq, taps_t& an, float& cn) {
                taps_landed(aq);
                fetch_a(an, cn);
                row_landed(xq, std::integral_constant<int, 3>());
                kn_order();
                if (q < n_q) mac(xq, aq, cq);
                kn_order();
                fetch_x(xq);
            };
            for (int q = 0; q < n_q; q += 4) {
                step4(q, x0, a0, c0, a1, c1);
                step4(q + 1, x1, a1, c1, a0, c0);
                step4(q + 2, x2, a0, c0, a1, c1);
                step4(q + 3, x3, a1, c1, a0, c0);
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+s"(a0));
        } else if constexpr (VEC == 1) {
            // One column per lane halves the packed instructions of a step, and then the step's SCALAR instructions are what a SIMD waits for: the two cursors above cost
            // about 40 of them per step.  With two rows in flight both operands are fetched one step ahead, in lock step: ONE cursor (slot `sl`, the channel's two base
            // pointers), advanced with a compare and selects, and no fetch past the last step (the loop stops two steps early, the tail fetches only what exists), so
            // nothing is clamped.  Same addresses, same order of the arithmetic.
            uint64_t xch = reinterpret_cast<uint64_t>(p.X);          // X + channel * HiWi * ldx, as a byte address
            uint64_t ach = reinterpret_cast<uint64_t>(a_base);       // taps + co0 + channel * cout_pad
            const uint64_t x_step = 4ull * (uint32_t)ch_x, a_step = 4ull * (uint32_t)p.cout_pad;      // one channel further, in bytes
            int sl = 0;
            auto fetch1 = [&](xrow_t& xr, taps_t& ar, float& cf) {
                const uint64_t xaddr = xch + 4ull * (uint32_t)__builtin_amdgcn_readlane(my_xoff, sl);
                const uint64_t aaddr = ach + 4ull * (uint32_t)__builtin_amdgcn_readlane(my_aoff, sl);
                asm volatile("global_load_dword %0, %1, %2" : "=&v"(xr) : "v"(lane_off_bytes), "s"(xaddr));
                if constexpr (RBX == 16) asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=&s"(ar) : "s"(aaddr));
                else asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=&s"(ar) : "s"(aaddr));
                if constexpr (COEF) cf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_coef), sl));
                const bool wrap = (sl + 1 == n_slots);
                sl = wrap ? 0 : sl + 1;
                xch += wrap ? x_step : 0;
                ach += wrap ? a_step : 0;
            };
            xrow_t x0, x1;
            taps_t a0, a1;
            float c0 = 1.0f, c1 = 1.0f;
            fetch1(x0, a0, c0);
            int q = 0;
            for (; q + 2 < n_q; q += 2) {
                taps_landed(a0);
                fetch1(x1, a1, c1);
                row_landed(x0, std::integral_constant<int, 1>());
                kn_order();
                mac(x0, a0, c0);
                kn_order();
                taps_landed(a1);
                fetch1(x0, a0, c0);
                row_landed(x1, std::integral_constant<int, 1>());
                kn_order();
                mac(x1, a1, c1);
                kn_order();
            }
            // One or two steps are left; x0 / a0 hold the first of them.  Its wait stands right behind the loop, as in the other forms (a wait inside a branch made the
            // compiler copy the row register ahead of it); the last step of an even walk is then fetched and waited for on its own: one step per work item without overlap.
            taps_landed(a0);
            row_landed(x0, std::integral_constant<int, 0>());
            kn_order();
            mac(x0, a0, c0);
            kn_order();
            if (q + 1 < n_q) {
                fetch1(x1, a1, c1);
                taps_landed(a1);
                row_landed(x1, std::integral_constant<int, 0>());
                kn_order();
                mac(x1, a1, c1);
            }
        } else {
        xrow_t x0, x1;
        taps_t a0, a1;
        float c0 = 1.0f, c1 = 1.0f;
        fetch_x(x0);
        fetch_a(a0, c0);
        advance();
        int q = 0;
        for (; q + 1 < n_q; q += 2) {
            taps_landed(a0);
            fetch_x(x1);
            fetch_a(a1, c1);
            advance();
            row_landed(x0, std::integral_constant<int, 1>());
            kn_order();
            mac(x0, a0, c0);
            kn_order();
            taps_landed(a1);
            fetch_x(x0);
            fetch_a(a0, c0);
            advance();
            row_landed(x1, std::integral_constant<int, 1>());
            kn_order();
            mac(x1, a1, c1);
            kn_order();
        }
        taps_landed(a0);
        row_landed(x0, std::integral_constant<int, 0>());
        if (q < n_q) mac(x0, a0, c0);
        }
    }
    if (!active) return;
    const float* xlast = p.lastcol ? (p.X + p.last_in_row * p.ldx + c) : nullptr;
    if constexpr (VEC == 1) {                                            // the same epilogue on one column: acc[r / 2][0][r % 2] is channel r
        const float xl1 = xlast ? *xlast : 0.f;
#pragma unroll
        for (int r = 0; r < RBX; r++) {
            const int m = co0 + r;
            if (m >= p.Cout) continue;
            const int64_t row = (int64_t)m * p.HoWo + o;
            float t = acc[r / 2][0][r % 2];
            if (xlast) {
                const float lc = p.lastcol[row];
                if (lc != 0.0f) {
                    const float bp = xl1 * lc;
                    t = t + bp;
                }
            }
            if (p.relu) t = (t < 0.0f) ? 0.0f : t;
            __builtin_nontemporal_store(t, p.Y + row * p.ldy + c);
        }
    } else {
    xrow_t xl4;
#pragma unroll
    for (int v = 0; v < VEC; v++) xl4[v] = 0.f;
    if (xlast) xl4 = *reinterpret_cast<const xrow_t*>(xlast);
#pragma unroll
    for (int r = 0; r < RBX; r++) {
        const int m = co0 + r;
        if (m >= p.Cout) continue;
        const int64_t row = (int64_t)m * p.HoWo + o;
        xrow_t t;
#pragma unroll
        for (int v = 0; v < VEC; v++) t[v] = acc[r][v / 2][v % 2];
        if (xlast) {
            const float lc = p.lastcol[row];
            if (lc != 0.0f) {
                const xrow_t bp = xl4 * lc;
                t = t + bp;
            }
        }
        if (p.relu) {
#pragma unroll
            for (int v = 0; v < VEC; v++) t[v] = (t[v] < 0.0f) ? 0.0f : t[v];
        }
        __builtin_nontemporal_store(t, reinterpret_cast<xrow_t*>(p.Y + row * p.ldy + c));      // the output is not re-read by this launch (conv1_1: 1.33 -> 1.11 ms)
    }
    }
