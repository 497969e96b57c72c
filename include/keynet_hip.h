/*
 * keynet_hip.h -- C ABI of libkeynet_hip.so: the MI355X (gfx950) engine behind the keyed forward of visym/keynet.
 *
 * Drop-in boundary.  The reference has exactly one plug-in seam for the forward path: the object stored in
 * KeyedLayer.W (keynet/layer.py:81-82), selected by layergen(..., backend=) (keynet/system.py:303-314), whose
 * torchdot() is the hot loop (keynet/layer.py:92).  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no torch / numpy / scipy types cross this boundary.
 *
 * Conventions
 *   - every function returns KN_OK (0) or a KN_ERR_* code; kn_last_error() gives the message (thread-local);
 *     no C++ exception crosses the boundary.
 *   - "host" pointers are ordinary CPU memory and are COPIED during the call (caller keeps ownership);
 *     "dev" pointers are HIP device memory owned by the caller (PyTorch-ROCm allocations in the Python host).
 *   - activations are FEATURE-MAJOR: X is [n_features, n_vecs] f32, element (f, b) at x[f*ldx + b].  This is the
 *     layout the reference hands to scipy (x_affine.t() -> ravel, keynet/layer.py:92 + scipy _matmul_multivector).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All compute calls are asynchronous and
 *     stream-ordered; a handle may be used from several streams/threads concurrently (it is immutable after create).
 */
#ifndef KEYNET_HIP_H
#define KEYNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KN_ABI_VERSION 5

enum kn_status {
    KN_OK = 0,
    KN_ERR_INVALID = 1,    /* bad argument (NULL, negative size, index out of range): the reference's `assert`s */
    KN_ERR_SHAPE = 2,      /* non-conformal shapes: keynet/sparse.py:605 */
    KN_ERR_HIP = 3,        /* a HIP runtime call failed (message has the hipError string) */
    KN_ERR_NOMEM = 4,
    KN_ERR_NODEVICE = 5,   /* no gfx950 device visible */
    KN_ERR_UNSUPPORTED = 6
};

/* kn_spmm flags */
#define KN_FLAG_RELU   1u  /* fuse torch.nn.functional.relu over the whole output incl. the homogeneous row
                              (unkeyed nn.ReLU after a keyed layer: keynet/system.py:92; keyed ReLU: keynet/layer.py:93) */
#define KN_FLAG_EXACT  2u  /* demand the reference's accumulation order and mul-then-add rounding (bit-exact with
                              scipy csr_matvecs).  CSR operators always honour it; conv-tap operators switch from the
                              MFMA kernel to an order-preserving VALU kernel that walks the factored operator in the
                              expansion's column order (no CSR is materialised: works at VGG-16 scale).
                              What "bit-exact" means per operator: a CSR / tiled operator holds the reference's own stored
                              values, so the result IS scipy's.  A conv-taps operator keyed directly in factored form
                              (kn_convtaps_create) whose entries carry float coefficients holds the TERMS coef * tap of
                              every stored value; a pixel pair hit by several taps is one stored value = the f32 sum of
                              its terms in entry order.  The flag then gives the order-preserving product of THOSE
                              stored values -- bit-equal to scipy csr_matvecs on kn_export_csr of this handle.  The
                              reference formed the same values inside scipy's SpGEMM (keynet/layer.py:35) in SpGEMM's
                              order: they agree to ~2e-6 relative, not bit for bit, which is inside the reference's
                              1e-5 criterion for float keys and outside "bit-exact with the reference" */

#define KN_FLAG_BF16X3 4u  /* allow a conv-taps operator to form its f32 products on the bf16 matrix pipe: operands split exactly into three
                              bf16 parts, six of the nine cross products kept (the dropped ones are <= 2^-23 of a product), f32 accumulate.
                              ~1 ulp per term away from the f32-MFMA result; never bit-exact; ignored with KN_FLAG_EXACT and by operators /
                              operands that do not qualify (Cin % 16, Cout > 64, n_vecs % 128).  No reference counterpart: the Python host
                              sets it only for layers whose calibration measured the result inside the float-key tolerance. */

#define KN_FLAG_NARROW 8u  /* low-latency form for 1 .. 8 batch columns: for n_vecs <= 8 a conv-taps operator runs the channel-lane order-preserving kernel
                              (one wavefront = one output pixel x 64 output channels, the batch columns are a lane's running sums).  The result is the
                              one KN_FLAG_EXACT gives, bit for bit, whether or not KN_FLAG_EXACT is set.  It wins over KN_FLAG_BF16X3.  It is ignored for
                              n_vecs > 8 and by operators that have no narrow form (every kind but conv-taps).  No reference counterpart as a flag: the
                              reference's forward IS one image at a time (keynet/system.py:130-133); the other conv-taps kernels give a lane batch
                              columns and want 128 of them. */

#define KN_FLAG_NARROW_MFMA 16u  /* KN_FLAG_NARROW for callers that accept the float-key tolerance: for n_vecs <= 8, without KN_FLAG_EXACT, an ELIGIBLE conv-taps operator runs
                              convtaps_narrow_mfma_kernel -- an implicit GEMM on v_mfma_f32_32x32x2_f32 whose N dimension is output pixels x batch columns (32 / NV pixels x
                              NV = 1 | 2 | 4 | 8 columns per tile), K = tap x input channel split over the four wavefronts of a workgroup and summed in a fixed order:
                              deterministic (the same bits on every call), not the reference's order of additions.  Eligible: no (output pixel, tap) pair holds more than 2
                              slots, no output pixel more than 64, and the per-pair records (16 bytes per pair, built at first use) stay below 2^22 -- identity / permutation / block-diagonal keys; the
                              filled-in operators of dense float keys are not.  In EVERY other case the flag means KN_FLAG_NARROW, bit for bit: with KN_FLAG_EXACT, on an
                              ineligible operator, on any other operator kind, at n_vecs > 8 (ignored).  Same size rule and refusal as KN_FLAG_NARROW.  kn_spmm_plan names
                              the kernel, its tile and NV.  No reference counterpart. */

#define KN_FLAG_NARROW_ROWS 32u  /* low-latency form of the float32 CSR operators for 1 .. 8 batch columns.  An opt-in of its own: KN_FLAG_NARROW and KN_FLAG_NARROW_MFMA
                              stay ignored by CSR handles, and this flag is ignored by conv-taps handles.
                              What runs.  For n_vecs <= 8 a float32 CSR handle (kn_csr_create, kn_tiled_create) runs csr_narrow_kernel on its pattern groups and loose rows.
                              The lane is the OUTPUT ROW and the batch columns are its NV = 1 | 2 | 4 | 8 running sums.  The walk over a row's stored columns is serial, in
                              stored order, with separate multiply and add: bit for bit the result without the flag.  Long loose rows (>= 1 024 entries) and the patched-row
                              guard run as without the flag.  So do the loose rows of an operator whose longest loose row holds more than 64 entries.
                              Where it is IGNORED (same kernels, same plan string, same bits as without it; the call falls back, it does not refuse):
                                - at n_vecs > 8;
                                - by conv-taps, dense, float64 and chain handles, and by kn_spmm_planes;
                                - where the kernel's 32-bit byte offsets into X would not hold (it runs while cols * ldx + 8 < 2^30);
                                - on the shape measured slower than the kernels it has: an operator with a keyed Linear's big pattern group (>= 256 rows over >= 2 048 shared
                                  columns) at more than 2 columns (profiles/r09_narrow_rows.txt).
                              Honoured by kn_spmm, by kn_spmm_screen (max |Y| by the library's reduction pass over Y) and by kn_spmm_plan, which names the kernel, NV and the
                              rows-per-wavefront form.  No reference counterpart. */

#define KN_FLAG_NARROW32 64u  /* a MODIFIER of KN_FLAG_NARROW and KN_FLAG_NARROW_MFMA: with either of them on a conv-taps handle it raises that flag's column range from 8 to 32.
                              For 9 <= n_vecs <= 32 KN_FLAG_NARROW then runs convtaps_narrow32_kernel -- the channel-lane order-preserving kernel with the columns in blocks of
                              NV = 8 | 16 | 32 running sums per lane, bit for bit the result of KN_FLAG_EXACT -- and KN_FLAG_NARROW_MFMA runs convtaps_narrow_mfma_kernel at NV = 16 | 32
                              (two pixels | one pixel per 32-column tile): the association of a column's sum depends on the K split alone, so every column has the bits the flag
                              gives that column in a batch of at most 8.  Every rule of the two flags carries over: KN_FLAG_EXACT, an ineligible operator and the Cin <= 4 shape
                              (beyond 4 columns on a chip-filling layer) turn KN_FLAG_NARROW_MFMA into KN_FLAG_NARROW, and the size rule REFUSES (KN_ERR_UNSUPPORTED, no fall-back)
                              unless (D + 1) * ldx + 32 < 2^31.
                              Where it changes NOTHING (same kernels, same plan string, same bits as without it): without one of the two flags; at n_vecs <= 8; at n_vecs > 32;
                              on CSR, dense, float64 and chain handles.  kn_spmm_plan names the kernel, NV and the number of column blocks.  No reference counterpart. */

#define KN_FLAG_NARROW64 0x80u  /* = 128.  A second MODIFIER of KN_FLAG_NARROW and KN_FLAG_NARROW_MFMA: with either of them on a conv-taps handle it opens the range 33 <= n_vecs <= 64.
                              There the call is the order-preserving product -- bit for bit the result of KN_FLAG_EXACT, and of the same columns inside a wider batch -- on the
                              software-pipelined kernel with ONE column per lane (convtaps_exact_pipe64_kernel: one wavefront = one output pixel x 16 | 8 output channels x one
                              64-column tile, the packed multiplies and adds run over output-channel pairs, half the vector-ALU work per step of a 128-column tile, lanes beyond
                              n_vecs masked).  No condition on the alignment of x and y or on ldx, ldy.  Without KN_FLAG_NARROW64_MFMA (below) KN_FLAG_NARROW_MFMA means
                              KN_FLAG_NARROW here, and KN_FLAG_EXACT / KN_FLAG_BF16X3 next to the flags change nothing.
                              Unlike KN_FLAG_NARROW / KN_FLAG_NARROW32 the range NEVER REFUSES: an operator without the pipeline's shape (filled-in operators: more than 64 slots
                              per output pixel or a pixel pair hit twice) and a block beyond (D + 1) * ldx < 2^31 run what KN_FLAG_EXACT runs at that width -- same plan string,
                              same bits.
                              Where it changes NOTHING (same kernels, same plan string, same bits as without it): without one of the two flags; at n_vecs <= 32 (the call is what its
                              other flags make it, KN_FLAG_NARROW32 included); at n_vecs > 64; on CSR, dense, float64 and chain handles; in kn_spmm_planes.  In particular KN_FLAG_EXACT
                              alone at 64 columns keeps the generic kernel.  kn_spmm_plan names the form ("64-column tiles").  No reference counterpart. */

#define KN_FLAG_NARROW64_MFMA (0x100u)  /* = 256.  The matrix-core form of the range KN_FLAG_NARROW64 opens, for callers that accept the float-key tolerance.  It takes effect ONLY next to
                              KN_FLAG_NARROW_MFMA | KN_FLAG_NARROW64, without KN_FLAG_EXACT, on a conv-taps handle at 33 <= n_vecs <= 64.  There the call is the f32 matrix-core
                              product of a plain kn_spmm (v_mfma_f32_32x32x2_f32, exact f32 products, re-ordered f32 sums) on ONE 64-column tile per (output pixel, channel tile):
                              convtaps_mfma_kernel<MT = 128 | 64, NB = 64>: 128 output channels per tile where that divides the padded channel count and leaves 1 024 workgroups, else 64.  Every column
                              has the bits that a plain kn_spmm gives it inside the same batch zero-padded to 128 aligned columns (same K order per output element), so a tolerance
                              decision made on the wide kernel covers it.  With KN_FLAG_EXACT the call is the order-preserving pipeline of KN_FLAG_NARROW64, bit for bit;
                              KN_FLAG_BF16X3 next to it changes nothing (there is no bf16 form at this width).  The range never refuses: a width, leading dimension or alignment the
                              straight-line loaders do not take (anything but 64 aligned columns) runs the generic loader.
                              Where it changes NOTHING (same kernels, same plan string, same bits as without it): alone, or with only one of the two flags; at n_vecs <= 32 and at
                              n_vecs > 64; on CSR, dense, float64 and chain handles; in kn_spmm_planes.  kn_spmm_plan names the launch
                              ("convtaps_mfma_kernel<MT=..,NB=64,KC=..> loader=..").  No reference counterpart. */

#define KN_FLAG_NARROW_LINEAR (0x200u)  /* = 512.  Low-latency form of a keyed Linear under the bit-exact contract, for 1 .. 64 batch columns.  An opt-in of its own, like KN_FLAG_NARROW_ROWS:
                              the conv flags neither imply nor exclude it.
                              What runs.  For n_vecs <= 32 (see below for 33 .. 64) a float32 CSR handle (kn_csr_create, kn_tiled_create) that holds BIG pattern groups (>= 256 rows over >= 2 048 shared
                              columns: a keyed nn.Linear) runs csr_stream_group_kernel on those groups.  A workgroup owns 64 member rows times all n_vecs columns: the lane is
                              the OUTPUT ROW, W = 1 | 2 | 4 | 8 wavefronts carry NV = 1 | 2 | 4 columns each as running sums (W * NV >= n_vecs), and the values reach them
                              through a ring in LDS that all wavefronts fill ahead of the walk -- the 256-byte value segments, and the activations of each step next to them --, so a value leaves HBM once per call.  The walk over a
                              row's stored columns is serial, in stored order, with separate multiply and add: bit for bit the result without the flag.  Everything else
                              the operator holds -- loose rows, the homogeneous row, long loose rows, small groups, the patched-row guard -- runs exactly what the call's other
                              flags make it; with KN_FLAG_NARROW_ROWS next to it at n_vecs <= 8 those parts take csr_narrow_kernel, and the big groups take
                              csr_stream_group_kernel at every width 1 .. 8 (KN_FLAG_NARROW_ROWS alone keeps its own rule, big-group operators at 1 and 2 columns only).
                              Where it changes NOTHING (same kernels, same plan string, same bits as without it; the call falls back, it does not refuse):
                                - on an operator without a big pattern group;
                                - at n_vecs > 64, and at 33 <= n_vecs <= 64: the form built for that range (8 wavefronts x 8 columns) measured 0.69x of csr_big_group_kernel on
                                  VGG-16's fc6 - fc8, so a handle with big groups keeps the kernel it has there (narrow_linear_loses; profiles/r13_narrow_linear.txt);
                                - on conv-taps, dense, float64 and chain handles, and in kn_spmm_planes.
                              The kernel forms every address into X in 64 bits: it takes any ldx (KN_FLAG_NARROW_ROWS next to it keeps its own rule for the parts it runs).
                              Honoured by kn_spmm, by kn_spmm_screen (max |Y| by the library's reduction pass over Y) and by kn_spmm_plan, which names the kernel, W, NV, the
                              number of 64-row chunks and the ring.  No reference counterpart. */
#define KN_FLAG_NARROW_TAPS (0x400u)  /* = 1024.  A MODIFIER of the channel-lane form of KN_FLAG_NARROW: the same product, bit for bit, with the taps resident in registers.
                              It takes effect ONLY where the call would run convtaps_narrow_kernel: on a conv-taps handle at n_vecs <= 8 with KN_FLAG_NARROW, or with
                              KN_FLAG_NARROW_MFMA where that flag means KN_FLAG_NARROW (with KN_FLAG_EXACT, on an operator without a matrix-core form, on the Cin <= 4 rule).
                              There an ELIGIBLE operator runs convtaps_narrow_taps_kernel: a wavefront owns P = 1 | 2 output pixels x 64 output channels x NV = 1 | 2 | 4 | 8
                              running sums; the pixels' slot lists (activation offsets, packed tap indices, coefficients) stay in scalar registers for the whole walk, an
                              input channel's value rows of all taps are loaded once into 16 vector registers, one channel ahead, and a step is one scalar activation load,
                              one indexed register read and NV multiply / add pairs.  Same order (input channel outer, slots by ascending input pixel inner), same separate
                              roundings, same bias entry, ReLU, homogeneous row and zero guard as KN_FLAG_NARROW: the result equals KN_FLAG_NARROW's and KN_FLAG_EXACT's.
                              Eligible: no summed stored values (filled-in operators are not), at most 9 slots per output pixel, at most 16 taps, with
                              coefficients or without, value rows in whole 64-channel blocks -- every conv layer of the tiled permutation / identity key-nets and the factored
                              untiled convs.  Per call: 4 * Hin * Win * ldx < 2^32 (the kernel's byte offsets inside one channel's plane).  An operator with coefficients runs 5 .. 8
                              columns as two launches, columns 0 .. 3 and the rest (its 8-column forms are not built), the same bits.
                              Where it changes NOTHING (same kernels, same plan string, same bits; it never refuses what KN_FLAG_NARROW does not refuse): alone; on an
                              ineligible operator or call; at n_vecs > 8 (the KN_FLAG_NARROW32 / KN_FLAG_NARROW64 ranges); where KN_FLAG_NARROW_MFMA runs the matrix-core
                              kernel; on CSR, dense, float64 and chain handles; in kn_spmm_planes.  kn_spmm_plan names the kernel, P, NV, the masked width and `coef`.
                              No reference counterpart. */
#define KN_MODIFIER_NARROW_TAPS32 (0x1000u)  /* = 4096.  A MODIFIER of KN_FLAG_NARROW_TAPS: with BOTH bits, the channel-lane form of KN_FLAG_NARROW | KN_FLAG_NARROW32 at
                              9 <= n_vecs <= 32 computes the same product, bit for bit, with the taps resident in registers and packed f32 arithmetic.
                              It takes effect ONLY where the call would run convtaps_narrow32_kernel on an operator ELIGIBLE for KN_FLAG_NARROW_TAPS (the rule above).
                              There the call runs convtaps_narrow_taps32_kernel: a wavefront owns one output pixel x 64 output channels x one block of NV = 8 | 16 | 32
                              columns (the block width and count KN_FLAG_NARROW32 chooses); the pixel's slot list stays in scalar registers, an input channel's value rows
                              of all taps are loaded once into 16 vector registers, one channel ahead, and a step is one or two scalar activation segment loads of 16
                              floats (the next one in flight behind the current arithmetic), one indexed register read and NV / 2 v_pk_mul_f32 + NV / 2 v_pk_add_f32 --
                              each element its own IEEE multiply and its own IEEE add.  Same order, same separate roundings, same bias entry, ReLU, homogeneous row and
                              zero guard as KN_FLAG_NARROW32: the result equals KN_FLAG_NARROW32's and KN_FLAG_EXACT's.
                              Per call: 4 * (Hin * Win * ldx + 32) < 2^32 (the kernel's byte offsets inside one channel's plane); a call that fails it runs
                              convtaps_narrow32_kernel.
                              Where it changes NOTHING (same kernels, same plan string, same bits): without KN_FLAG_NARROW_TAPS; at n_vecs <= 8 (KN_FLAG_NARROW_TAPS
                              alone decides there) and at n_vecs > 32; in every other regime; on an ineligible operator; where KN_FLAG_NARROW_FILL takes the launch; on
                              CSR, dense, float64 and chain handles; in kn_spmm_planes.  KN_FLAG_NARROW_TAPS without this bit stays a no-op at n_vecs > 8.
                              kn_spmm_plan names the kernel, the value rows, NV, the masked width, the column blocks and `coef`.  No reference counterpart. */
#define KN_MODIFIER_NARROW_TAPS_PAIRS (0x2000u)  /* = 8192.  A MODIFIER of KN_FLAG_NARROW_TAPS: with BOTH bits, the tap-resident form of KN_FLAG_NARROW at 1 <= n_vecs <= 8
                              computes the same product, bit for bit, with TWO output channels per lane and packed f32 arithmetic.
                              It takes effect ONLY where the call would run convtaps_narrow_taps_kernel (the rule of KN_FLAG_NARROW_TAPS above) on an operator of more than
                              64 output channels.  There the call runs convtaps_narrow_taps_pairs_kernel: a wavefront owns one output pixel x 128 output channels (lane l:
                              channels 128 b + l and 128 b + 64 + l, the two halves of a register pair) x NV = 1 | 2 | 4 | 8 running sums per channel; the pixel's slot
                              list stays in scalar registers, an input channel's value rows of all taps are loaded once into 16 vector register pairs, one channel ahead,
                              and a step is one scalar activation load, one indexed read of a register pair and NV v_pk_mul_f32 + NV v_pk_add_f32 -- each element its own
                              IEEE multiply and its own IEEE add, the step's scalar half paid once for 128 channels.  A trailing block of 64 padded channels re-reads its
                              first half's value rows and stores nothing for the second.  Same order, same separate roundings, same bias entry, ReLU, homogeneous row
                              and zero guard as KN_FLAG_NARROW: the result equals KN_FLAG_NARROW's and KN_FLAG_EXACT's.  An operator with coefficients runs 5 .. 8 columns
                              as two launches of this kernel, columns 0 .. 3 and the rest, as it does on convtaps_narrow_taps_kernel.
                              A launch has half the wavefronts of convtaps_narrow_taps_kernel's: the (shape, width) pairs whose launch was not faster in a kernel
                              trace (deep layers of few pixels: fewer than 1 024 wavefronts at every width, fewer than 4 096 up to 4 columns) keep that kernel.
                              Where it changes NOTHING (same kernels, same plan string, same bits; it never refuses): without KN_FLAG_NARROW_TAPS; at n_vecs > 8; where
                              KN_FLAG_NARROW_MFMA runs the matrix-core kernel; where KN_FLAG_NARROW_FILL takes the launch; on operators of 64 output channels or fewer;
                              on an ineligible operator or call; on CSR, dense, float64 and chain handles; in kn_spmm_planes.
                              kn_spmm_plan names the kernel, the value rows, NV, the masked width and `coef`.  No reference counterpart. */
#define KN_FLAG_NARROW_FILL (0x800u)  /* = 2048.  A MODIFIER of the channel-lane forms of KN_FLAG_NARROW (1 .. 8 columns) and KN_FLAG_NARROW | KN_FLAG_NARROW32 (9 .. 32): the same
                              product, bit for bit, for FILLED-IN operators (summed stored values, hundreds of slots per output pixel: the reference's doubly-stochastic keys).
                              It takes effect ONLY where the call would run convtaps_narrow_kernel or convtaps_narrow32_kernel: on a conv-taps handle with KN_FLAG_NARROW, or
                              with KN_FLAG_NARROW_MFMA where that flag means KN_FLAG_NARROW.  There an ELIGIBLE operator runs convtaps_narrow_fill_kernel: a wavefront owns one
                              output pixel x 64 output channels x NV = 1 | 2 | 4 | 8 running sums; the pixel's slot records {input pixel, tap index, coefficient, first | last
                              slot of a stored column} are streamed by scalar loads a batch ahead, an input channel's value rows of all taps are loaded once into 16 vector
                              registers, one channel ahead, a slot is one indexed register read, one multiply and one add, and a stored column costs one scalar activation
                              load and NV multiply / add pairs.  9 .. 32 columns run as blocks of 8 columns, each block a wavefront of its own.  Same order (input channel
                              outer, slots by ascending input pixel inner, the terms of a stored value in entry order), same separate roundings, same bias entry, ReLU,
                              homogeneous row and zero guard as KN_FLAG_NARROW: the result equals KN_FLAG_NARROW's and KN_FLAG_EXACT's.
                              Eligible: an operator that has the record lists of the filled-in KN_FLAG_EXACT kernel (summed stored values, or more than 64 slots on an output
                              pixel), at most 16 taps, value rows in whole 64-channel blocks.  Per call: 4 * (Hin * Win * ldx + 32) < 2^32 (the kernel's byte offsets inside one
                              channel's plane); a call that fails it runs the kernel it runs without the bit.
                              The flag CAN ALLOCATE: the first such call builds the operator's record table on the device (16 bytes per slot, the table KN_FLAG_EXACT builds;
                              kn_release_side_tables frees it, the next such call builds it again).
                              Where it changes NOTHING (same kernels, same plan string, same bits; it never refuses what KN_FLAG_NARROW does not refuse): alone; on an
                              ineligible operator or call; at n_vecs > 32 (the KN_FLAG_NARROW64 range); where KN_FLAG_NARROW_MFMA runs the matrix-core kernel; with
                              KN_FLAG_EXACT or the matrix-core flags only; on CSR, dense, float64 and chain handles; in kn_spmm_planes.  No operator is eligible for both
                              KN_FLAG_NARROW_TAPS and KN_FLAG_NARROW_FILL.  kn_spmm_plan names the kernel, NV, the masked width, the column blocks and `coef`.
                              No reference counterpart. */

#define KN_MODIFIER_WINO (0x4000u)  /* = 16384 (the next free bit: 0x1000 and 0x2000 are the two modifiers above).  A MODIFIER of a plain kn_spmm on a conv-taps handle, for callers
                              that accept the float-key tolerance: a keyed 3 x 3 convolution runs in its 1-D Winograd F(2,3) form along the image rows -- two neighbouring outputs of
                              a 3-tap row from 4 products instead of 6, two thirds of the matrix instructions.  Three launches: wino_in_kernel forms V [Cin][HiWi / 2][4] (sums and
                              differences of two activation rows, f32), convtaps_mfma_kernel applies the DERIVED conv-taps operator (2 * HoWo pseudo output pixels, at most 3 slots each,
                              12 tap matrices U formed in double and rounded once, K = 3 * Cin) into M, wino_out_kernel forms y(2c) = M0 + M1 + M2 + bias, y(2c + 1) = M1 - M2 - M3 + bias in
                              that order, applies ReLU and stores (nontemporal; max |Y| of kn_spmm_screen folded in); conv_lastrow_kernel keeps the homogeneous row.  Every
                              product and sum is f32; the association is not the plain call's, so the result agrees with it to the float-key tolerance, never bit for bit,
                              and a column's bits do not depend on the batch width.  Inf - Inf inside the transforms is NaN where the plain product is Inf: a caller that must
                              reproduce non-finite activations keeps them away from the flag (the Python host's screen does).
                              It takes effect ONLY on a conv-taps handle, without KN_FLAG_EXACT and outside the narrow ranges, at n_vecs a multiple of 128 with x, y 16-byte
                              aligned and ldx, ldy multiples of 4, on an ELIGIBLE operator: 9 taps, unit coefficients, no (output pixel, input pixel) pair hit twice, equal
                              image sizes, at most one entry per (pixel, tap), and an entry table that IS a 3 x 3 convolution with zero padding of an image of even width under
                              some pixel permutation on either side (derived from the table itself at the first call that asks, verified against the whole table;
                              kn_wino_status says why an operator is not).  KN_FLAG_BF16X3 next to it changes nothing.
                              The flag CAN ALLOCATE: the first such call (kn_spmm_plan included) derives and packs the operator's form (kn_release_side_tables frees it), and a
                              call takes 2 * (Cin * HiWi + Cout * HoWo) * n_vecs floats from ONE pool per (device, stream) shared by all handles, grown to the largest request
                              (kn_reserve_workspace with the flag's handle sizes it ahead of a HIP-graph capture; an unreserved call under capture fails).
                              Where it changes NOTHING (same kernels, same plan string, same bits): with KN_FLAG_EXACT; in the narrow ranges; at other widths or alignments; on an
                              ineligible operator; on CSR, dense, float64 and chain handles; in kn_spmm_planes.  kn_spmm_plan lists the three launches.  No reference counterpart. */

typedef struct kn_operator* kn_handle_t;   /* opaque keyed operator resident in HBM */

int         kn_abi_version(void);
const char* kn_last_error(void);
/* number of visible HIP devices and the gcnArchName of the current one (buf may be NULL) */
int         kn_device_info(int* n_devices, char* arch_buf, int64_t arch_buf_len);

/* ---- operators ---------------------------------------------------------------------------------------------- */

/* Replaces keynet.sparse.SparseMatrix(A) for a scipy CSR matrix (keynet/sparse.py:419-425).
 * indptr[rows+1], indices[nnz], data[nnz] are HOST arrays; the STORED order of each row is preserved on the device
 * (keyed matrices are SpGEMM outputs: unsorted, non-canonical; sorting them changes results -- SURVEY 8c). */
int kn_csr_create(int64_t rows, int64_t cols, int64_t nnz,
                  const int32_t* indptr, const int32_t* indices, const float* data,
                  kn_handle_t* out);

/* The same container when its scipy matrix is FLOAT64 (SparseMatrix keeps `A.dtype`, keynet/sparse.py:423; the public challenge key-net the
 * reference ships, demo/keynet_challenge_lenet_10AUG20.pkl + demo/challenge.ipynb cell 5, carries float64 conv / pool operators).  torchdot
 * (keynet/sparse.py:488-492) coerces x to float32 and hands both to scipy: numpy up-casts, csr_matvecs runs in float64 (x up-cast element by
 * element, f64 multiply then f64 add in stored order) and the layer returns a float64 block that the next layer's coercion rounds to f32.
 * kn_spmm on such a handle writes that block rounded to f32 ONCE (what the next layer consumes); kn_spmm_f64 writes the float64 block itself
 * (what the reference's torchdot returns).  Bit-exact with scipy either way; KN_FLAG_EXACT is implied, kn_chain_create refuses the handle. */
int kn_csr_create_f64(int64_t rows, int64_t cols, int64_t nnz,
                      const int32_t* indptr, const int32_t* indices, const double* data,
                      kn_handle_t* out);

/* Replaces keynet.sparse.TiledMatrix / DiagonalTiledMatrix (keynet/sparse.py:517-571, 657-687):
 * blocks[nblocks][3] = (row0, col0, k) as iterated by __iter__; tile k = COO entries tile_ptr[k]..tile_ptr[k+1] of
 * (tile_row, tile_col, tile_val) relative to the block origin.  Semantics = tosparse() (keynet/sparse.py:621-641). */
int kn_tiled_create(int64_t rows, int64_t cols,
                    int64_t nblocks, const int64_t* blocks,
                    int64_t ntiles, const int64_t* tile_ptr,
                    const int32_t* tile_row, const int32_t* tile_col, const float* tile_val,
                    kn_handle_t* out);

/* Replaces keynet.sparse.Conv2dTiledMatrix (keynet/sparse.py:690-776): spatial blocks x dense channel matrices.
 *   inshape/outshape = (C,H,W); rows = Cout*Hout*Wout (+1), cols = Cin*Hin*Win (+1)
 *   blocks[nblocks][3]   = (i, j, k) incl. the bias blocks (j == Cin*Hin*Win)             (sparse.py:753,773,776)
 *   tile_keys[nent][3]   = (it, jt, k) in dict order                                      (sparse.py:764)
 *   tile_isbias[nent]    = 1 for the 1x1 bias tiles                                       (sparse.py:767-772)
 *   tile_chan            = f32[n_chan][Cout][Cin] for the non-bias entries, in tile_keys order
 *   tile_bias            = f32[n_bias] for the bias entries, in tile_keys order
 * Expansion rule (sparse.py:802-812): W[i+it+ic*HoWo, j+jt+jc*HiWi] = tile[(it,jt,k)][ic,jc]. */
int kn_conv2dtiled_create(int64_t rows, int64_t cols,
                          const int64_t inshape[3], const int64_t outshape[3],
                          int64_t nblocks, const int64_t* blocks,
                          int64_t nent, const int64_t* tile_keys, const uint8_t* tile_isbias,
                          const float* tile_chan, const float* tile_bias,
                          kn_handle_t* out);

/* The same operator in factored form  W = sum_e coef_e * ( taps[tap_e] (x) E[out_e, in_e] )  + last column + e_last row,
 * i.e. what Conv2dTiledMatrix stores after de-duplicating its channel matrices.  Used by the direct-to-tiled keying
 * (never materialises the 15 G-nnz CSR of keyed VGG-16; keynet/layer.py:24-41 + sparse.py:720-776 collapsed).
 *   taps      f32[ntaps][Cout][Cin]
 *   ent_*     [nent]: output pixel (0..HoWo), input pixel (0..HiWi), tap id, coefficient
 *   lastcol   f32[Cout*HoWo + 1] = W[:, Cin*HiWi] (bias column incl. the homogeneous 1 at the end), or NULL => no
 *             homogeneous row/column at all (bias=False operators, rows == Cout*HoWo). */
int kn_convtaps_create(const int64_t inshape[3], const int64_t outshape[3],
                       int64_t ntaps, const float* taps,
                       int64_t nent, const int32_t* ent_out, const int32_t* ent_in, const int32_t* ent_tap, const float* ent_coef,
                       const float* lastcol,
                       kn_handle_t* out);

/* Declares that the ZERO-valued entries of a kn_convtaps_create operator's expansion are ABSENT from the reference operator it stands for.
 * A tiled reference operator keeps the zeros of its dense channel matrices as explicit entries (keynet/sparse.py:802-812), and 0 * Inf = NaN
 * reaches its output like any other entry; an UNTILED keyed conv layer is a scipy CSR (keynet/layer.py:24-41) from which the keying SpGEMM
 * has dropped every exact zero (a filter weight the reference's value round trip turned into 0.0).  When such a CSR is stored in ascending
 * column order -- identity / channel-replicated permutation keys on both sides -- its product in stored order IS the factored operator's
 * order-preserving product (KN_FLAG_EXACT), entry for entry, and the host may hand over the 0.3 MB of taps instead of the CSR's hundreds of
 * MB; after this call kn_spmm with KN_FLAG_EXACT additionally restores, for batch columns whose activation at such an absent position is not
 * finite, exactly what the reference's row (without that entry) computes.  KN_ERR_UNSUPPORTED on other operator kinds. */
int kn_convtaps_drop_zero_entries(kn_handle_t h);

/* A DENSE operator (keyed nn.Linear: keynet/layer.py:67-70 stores it as a sparse matrix whose every entry is present)
 * for callers that accept the float-key tolerance (1e-5) instead of scipy's exact accumulation order -- i.e. the tiled
 * key-nets, whose conv layers already run on the matrix cores.  W is the full keyed matrix, HOST, row-major
 * [rows][cols] INCLUDING the homogeneous row (e_last) and the bias column; rows-1 outputs, cols-1 inputs.
 * kn_spmm computes it as a split-K f32-MFMA GEMM (K slices = pseudo-pixels of the conv-taps kernel) followed by an
 * ordered reduction over the slices (deterministic: no atomics).  Returns KN_ERR_UNSUPPORTED when cols-1 is not a
 * multiple of 256 (use kn_csr_create then).  KN_FLAG_EXACT is refused on such a handle. */
int kn_dense_create(int64_t rows, int64_t cols, const float* W, kn_handle_t* out);

/* Replaces the nn.Sequential walk of KeyedModel.forward (keynet/system.py:130-133, `self._keynet.forward(x)`) for a key-net whose
 * operators are all CSR handles (kn_csr_create / kn_tiled_create: the permutation key-nets) and whose activations are small enough
 * to stay on chip: kn_spmm on the returned handle applies ops[0] ... ops[n_ops-1] back to back in ONE launch, the activations of
 * four batch columns resident in LDS, ReLU after operator l when flags[l] & KN_FLAG_RELU (flags may be NULL).  Same arithmetic as
 * n_ops kn_spmm calls with KN_FLAG_EXACT (stored order, f32 multiply then add): bit-identical results.  The handle keeps its own
 * copy of the operators (ops may be destroyed afterwards).  X is [ops[0].cols, n_vecs], Y is [ops[n_ops-1].rows, n_vecs].
 * KN_ERR_UNSUPPORTED when an operator is not a CSR handle, n_ops > 12, or (max features in + out of a layer) * 16 B > 160 KiB. */
int kn_chain_create(int64_t n_ops, const kn_handle_t* ops, const uint32_t* flags, kn_handle_t* out);

int kn_destroy(kn_handle_t h);

/* SparseMatrix.nnz / TiledMatrix.nnz / Conv2dTiledMatrix.nnz (keynet/sparse.py:494,649,778): stored parameters. */
int kn_nnz(kn_handle_t h, int64_t* nnz);
/* nnz of the expanded operator the reference applies (tocsr()), = the algorithmic MAC count per input vector */
int kn_nnz_expanded(kn_handle_t h, int64_t* nnz);
int kn_shape(kn_handle_t h, int64_t* rows, int64_t* cols);
/* SparseMatrix.dtype (keynet/sparse.py:423) as a width: 64 for a kn_csr_create_f64 operator, 32 for every other handle */
int kn_dtype_bits(kn_handle_t h, int* bits);

/* tocsr()/tocoo() (keynet/sparse.py:502-507, 643-647, 816-835): expanded operator into HOST buffers sized by
 * kn_nnz_expanded (indptr[rows+1]).  CSR operators come back in stored order; tiled ones canonical (sorted). */
int kn_export_csr(kn_handle_t h, int32_t* indptr, int32_t* indices, float* data);
/* the same for a kn_csr_create_f64 operator (stored order, float64 values); kn_export_csr refuses such a handle and vice versa */
int kn_export_csr_f64(kn_handle_t h, int32_t* indptr, int32_t* indices, double* data);

/* ---- the hot path -------------------------------------------------------------------------------------------- */

/* Replaces SparseMatrix.torchdot / TiledMatrix.torchdot (keynet/sparse.py:488-492, 603-612):
 *   Y[rows, n_vecs] = W . X[cols, n_vecs]      (+ ReLU when KN_FLAG_RELU)
 * x_dev/y_dev: device f32, feature-major, leading dimensions ldx/ldy >= n_vecs (floats).  x and y must not alias.
 *
 * What a caller may pass.  ANY ldx, ldy >= n_vecs whose blocks (cols * ldx and rows * ldy floats) fit in device memory are accepted, blocks of more than 2^31 elements
 * included: every kernel forms row * ldy, and the general kernels col * ldx, in 64 bits.  The fast forms keep narrower offsets into X and are chosen only while these hold
 * (HiWi = Hin * Win, D = Cin * HiWi of a conv-taps operator); beyond a threshold the next slower form runs, with the same result under the same flags:
 *   CSR pattern groups, software-pipelined kernel       cols * ldx < 2^31                                  else the plain grouped kernel
 *   conv-taps, matrix cores (no KN_FLAG_EXACT)          wave-uniform loaders: 4 * (T * HiWi * ldx + NB) < 2^31, NB = 128 | 256 batch columns per tile, T = 1024 / NB;
 *                                                       straight-line loaders: 16 * HiWi * ldx < 2^31 (4 * for Cin < 16); else the generic loader
 *   conv-taps, KN_FLAG_EXACT, pipelined kernel          (D + 1) * ldx < 2^31                               else the plain order-preserving kernel
 *   conv-taps, KN_FLAG_EXACT, filled-in operators       4 * ldx < 2^24, 4 * HiWi * ldx < 2^32, HiWi < 2^24  else the plain order-preserving kernel
 *   conv-taps, KN_FLAG_NARROW64 (33 <= n_vecs <= 64)    (D + 1) * ldx < 2^31                               else the plain order-preserving kernel
 *   conv-taps, KN_FLAG_NARROW64_MFMA (33 .. 64)         the matrix-core rules above at NB = 64 (T = 16), on n_vecs = 64 aligned columns; else the generic loader
 *   CSR, KN_FLAG_NARROW_ROWS (n_vecs <= 8)               cols * ldx + 8 < 2^30                              else the kernels the call takes without the flag
 *   CSR, KN_FLAG_NARROW_LINEAR (n_vecs <= 32)            none: 64-bit addresses, any ldx
 *   conv-taps, KN_FLAG_NARROW_FILL (n_vecs <= 32)       4 * (HiWi * ldx + 32) < 2^32                        else the channel-lane kernel the call takes without the flag
 * The small-K matrix-core kernels of first-layer operators (slots * Cin + bias <= 28 contraction rows) form row * ldx in 64 bits and take any ldx.
 * KN_FLAG_NARROW / KN_FLAG_NARROW_MFMA (n_vecs <= 8 on a conv-taps operator) do NOT fall back: they return KN_ERR_UNSUPPORTED, Y untouched, unless (D + 1) * ldx + 8 < 2^31
 * (with KN_FLAG_NARROW32 at 9 <= n_vecs <= 32: unless (D + 1) * ldx + 32 < 2^31).
 * kn_spmm_plan names the kernel a call takes; tests/test_large_offsets_gpu.py runs each of these on both sides of its threshold. */
int kn_spmm(kn_handle_t h, const float* x_dev, int64_t ldx, int64_t n_vecs,
            float* y_dev, int64_t ldy, uint32_t flags, void* stream);

/* SparseMatrix.torchdot of a FLOAT64 operator (kn_csr_create_f64) with the result dtype the reference returns: Y[rows, n_vecs] float64 =
 * W . (double)X, accumulated in float64 in stored order (+ ReLU when KN_FLAG_RELU: F.relu on the float64 block, keynet/layer.py:93).
 * x_dev float32 as everywhere (keynet/sparse.py:489-491), y_dev device float64 with leading dimension ldy (doubles).  KN_ERR_UNSUPPORTED on
 * any other handle: float32 operators return float32. */
int kn_spmm_f64(kn_handle_t h, const float* x_dev, int64_t ldx, int64_t n_vecs,
                double* y_dev, int64_t ldy, uint32_t flags, void* stream);

/* The same operator applied to n_planes independent activation blocks in ONE launch per kernel: block p is X_p = x_dev + p * x_plane_stride (floats), its result
 * Y_p = y_dev + p * y_plane_stride.  Bit-identical to n_planes kn_spmm calls (same kernels, grid dimension y = plane).  No reference counterpart as a call -- the reference
 * applies the fused operator (keynet/sparse.py:603-612); this is what the split application of a FILLED-IN conv needs (keynet_amd/sparse.py: the spatial matrix of all taps
 * applied to every input channel's plane, 64 .. 512 planes per layer -- one launch instead of one per plane).  float32 CSR handles whose rows are pattern groups / loose rows
 * only; KN_ERR_UNSUPPORTED otherwise (the caller loops over kn_spmm).  Always the stored order (KN_FLAG_EXACT is implied for CSR operators); KN_FLAG_RELU is honoured. */
int kn_spmm_planes(kn_handle_t h, const float* x_dev, int64_t ldx, int64_t x_plane_stride, int64_t n_planes, int64_t n_vecs,
                   float* y_dev, int64_t ldy, int64_t y_plane_stride, uint32_t flags, void* stream);

/* kn_spmm that additionally raises *y_absmax_dev (device f32, caller-initialised, e.g. to 0) to max |Y[r, b]| over the block it wrote,
 * stream-ordered.  No reference counterpart: the reference applies ONE arithmetic on every call (keynet/sparse.py:488-492), so its 1e-5
 * float-key agreement holds per call; a host that runs a layer on the matrix cores because a calibration batch showed the re-ordered sum
 * inside that tolerance must notice when a later batch is larger.  max |Y| of layer l is max |X| of layer l+1, and the matrix-core kernels
 * fold it into their store epilogue (no extra pass over a multi-GB activation block); behind the other kernel families the library runs
 * one reduction pass over Y.  NaN entries are ignored, +-Inf counts.  y_absmax_dev == NULL is kn_spmm. */
int kn_spmm_screen(kn_handle_t h, const float* x_dev, int64_t ldx, int64_t n_vecs,
                   float* y_dev, int64_t ldy, uint32_t flags, float* y_absmax_dev, void* stream);

/* max |X[r, b]| of an activation block (the input of the first layer: nothing produced it on the device), raised into *absmax_dev like
 * kn_spmm_screen does. */
int kn_absmax(const float* x_dev, int64_t rows, int64_t ld, int64_t n_vecs, float* absmax_dev, void* stream);

/* Drops the side tables a conv-taps operator builds at first use (the slot records of the filled-in order-preserving kernel: 16 bytes per slot, 0.4 - 4 GB per layer of the
 * reference's doubly-stochastic VGG-16; the bf16 planes of KN_FLAG_BF16X3).  They are rebuilt by the next kn_spmm that needs them.  No reference counterpart (memory management
 * of this library): the host calls it for a layer whose calibration settled on a contract that does not use them.  Waits for the device; not for the hot path. */
int kn_release_side_tables(kn_handle_t h);

/* Pre-size the per-stream state kn_spmm would otherwise allocate at first use on `stream` for `n_vecs` batch columns (only a
 * kn_dense_create handle has any: its split-K partial sums), so that the first kn_spmm on that stream can be captured into a HIP graph.
 * A no-op for every other operator kind. */
int kn_reserve_workspace(kn_handle_t h, int64_t n_vecs, void* stream);
/* The same for a call that carries `flags`: with KN_MODIFIER_WINO on a conv-taps handle whose call at n_vecs columns would take the Winograd form (16-byte aligned blocks assumed) it
 * derives the form if that has not happened yet and grows the (device, stream) pool to what the call needs; with any other flag word it is kn_reserve_workspace.  An added
 * entry point: KN_ABI_VERSION stays. */
int kn_reserve_workspace_flags(kn_handle_t h, int64_t n_vecs, uint32_t flags, void* stream);
/* KN_MODIFIER_WINO: is the operator eligible?  Derives the form if no call has asked yet (it allocates, like the first such kn_spmm).  *eligible = 1 | 0; buf (may be NULL)
 * receives "eligible" or the reason it is not, NUL-terminated.  KN_ERR_UNSUPPORTED on other handle kinds.  An added entry point: KN_ABI_VERSION stays. */
int kn_wino_status(kn_handle_t h, int* eligible, char* buf, int64_t buf_len);

/* Introspection: which kernels kn_spmm would launch for this operator, batch width, leading dimensions (16-byte aligned activations
 * assumed) and flags -- the SAME dispatch code runs, every launch site describes itself instead of launching.  No reference
 * counterpart (scipy has one kernel); it exists so that measurements can state which loader / tile shape produced them
 * ("choices evidenced").  Writes a NUL-terminated, ';'-separated list into buf.  Launches nothing and allocates nothing
 * (with KN_FLAG_BF16X3 it reports eligibility from the operator's shape; the bf16 planes are built by the first real kn_spmm). */
int kn_spmm_plan(kn_handle_t h, int64_t n_vecs, int64_t ldx, int64_t ldy, uint32_t flags, char* buf, int64_t buf_len);

/* unkeyed nn.ReLU on a whole activation block (keynet/system.py:92) when it could not be fused */
int kn_relu(float* y_dev, int64_t rows, int64_t ld, int64_t n_vecs, void* stream);

/* keynet.torch.affine_to_linear (keynet/torch.py:65-68) fused with the x.t() of keynet/layer.py:92:
 * x_dev [n, d] row-major images  ->  out_dev [d+1, n] feature-major with the ones row appended. */
int kn_affine_to_linear(const float* x_dev, int64_t n, int64_t d, float* out_dev, int64_t ldo, void* stream);

/* The sensor's ingest of raw frames (keynet/system.py:183-201, 250-255 with keynet/torch.py:65-68): the reference's sensor loads an image as [0, 255] values, homogenises
 * it and hands it to the image key, on the host; this is the load and the homogenisation for n uint8 frames that are already on the device, in one launch.
 *   img_dev   n frames of c * h * w bytes; layout 0: img[b][ch][y][x] (NCHW), layout 1: img[b][y][x][ch] (NHWC: a camera's or PIL's order)
 *   out_dev   the feature-major block, D = c * h * w:  out[((ch * h + y) * w + x) * ldo + b] = (float)img[b][..]   for b < n
 *                                                      out[D * ldo + b] = 1.0f                                  for b < n   (the ones row)
 *             every row, the ones row included, is +0.0f for n <= b < n_cols (zero images: the padding of a batch to whole tiles, written in the same launch);
 *             columns n_cols <= b < ldo are not touched.
 * uint8 -> float32 is exact: the block is bit-equal to kn_affine_to_linear on the frames converted to float32 NCHW, followed by that padding.  1 <= n <= n_cols <= ldo and
 * c, h, w >= 1 (KN_ERR_SHAPE otherwise; nothing is launched); every address is formed in 64 bits.  Tiled through LDS (256 frame positions x 64 images): contiguous bytes
 * along a frame on the way in, contiguous floats along the batch on the way out -- 16-byte stores where ldo and out_dev are multiples of four floats, scalar stores otherwise;
 * the (y, x, ch) -> (ch, y, x) permutation of layout 1 is index arithmetic of the same pass.  An added entry point: KN_ABI_VERSION stays (the rule below). */
int kn_u8_to_linear(const uint8_t* img_dev, int64_t n, int64_t c, int64_t h, int64_t w, int layout, float* out_dev, int64_t ldo, int64_t n_cols, void* stream);

/* The per-image range of a feature-major block, on the device: the minimum and maximum the reference's mat2gray takes of an image on the host (keynet/sparse.py:25-33,
 * behind keynet/system.py:173-181 and 223-228), for every column of a batch at once.
 *   lo_dev[b] = min, hi_dev[b] = max of x[r * ld + b] over r < rows, for b < n_vecs <= ld (KN_ERR_SHAPE otherwise).  The caller passes rows = D: the ones row stays out.
 * NaN elements are skipped; a column with no other element gives lo = +Inf, hi = -Inf (so does rows == 0).  Minimum and maximum are exact and commute, so the result does
 * not depend on the launch geometry; only the sign of a zero is open (-0.0 and +0.0 compare equal).  The call initialises lo / hi itself (elements n_vecs and beyond are not
 * touched), allocates nothing and does not wait for the device: it can be captured into a HIP graph.  Row chunks meet in the outputs through ordinary vector integer atomics
 * on the floats' bits.  Every address is formed in 64 bits.  An added entry point: KN_ABI_VERSION stays (the rule below). */
int kn_column_range(const float* x_dev, int64_t rows, int64_t ld, int64_t n_vecs, float* lo_dev, float* hi_dev, void* stream);

/* The sensor's egress of frames, the inverse of kn_u8_to_linear in one launch: the reference turns a loaded tensor into a viewable 8-bit image on the host -- linear_to_affine
 * (keynet/torch.py:71-77), the gray mapping of mat2gray (keynet/sparse.py:25-33) and the conversion to bytes (keynet/system.py:173-181, 223-228; decrypt at 257-263 stops
 * at the float tensor) -- this is the affine, the rounding and the layout change for n columns of a feature-major block that is already on the device.
 *   x_dev     the feature-major block, D = c * h * w rows of ldx floats; row D (the ones row) is not read, nor are columns n <= b < ldx
 *   img_dev   n frames of D bytes; layout as kn_u8_to_linear's: 0: img[b][ch][y][x] (NCHW), 1: img[b][y][x][ch] (NHWC).  For b < n:
 *                 t = gain[b] * x[((ch * h + y) * w + x) * ldx + b]        one IEEE f32 multiply
 *                 t = t + bias[b]                                          one IEEE f32 add: never fused with the multiply
 *                 img[b][..] = 0 if t is NaN, else min(255, max(0, rint(t)))    round to nearest, ties to even; -Inf -> 0, +Inf -> 255
 *             bytes outside the n * D of the frames are not touched.
 *   gain_dev, bias_dev   n device floats each; gain_dev == NULL means 1.0f, bias_dev == NULL means 0.0f (with both NULL t is x itself)
 * 1 <= n <= ldx and c, h, w >= 1 (KN_ERR_SHAPE otherwise; nothing is launched); NULL x_dev or img_dev is KN_ERR_INVALID; every address is formed in 64 bits.  Tiled through
 * LDS as bytes (256 frame positions x 64 images): contiguous floats along the batch on the way in -- 16-byte loads where ldx and x_dev are multiples of four floats, scalar
 * loads otherwise -- contiguous bytes along a frame on the way out -- a dword per lane where D and img_dev are multiples of four bytes, bytes otherwise; the
 * (ch, y, x) -> (y, x, ch) permutation of layout 1 is index arithmetic of the same pass.  No workspace.  An added entry point: KN_ABI_VERSION stays (the rule below). */
int kn_linear_to_u8(const float* x_dev, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout,
                    const float* gain_dev, const float* bias_dev, uint8_t* img_dev, void* stream);

/* The dequantising ingest of encrypted frames: kn_u8_to_linear for the wire between a sensor and the key-net.  The reference stores an encrypted image as an 8-bit picture
 * (keynet/system.py:173-181) and reads it back on the host through a private image key (keynet/system.py:185-194); here n quantised frames that are already on the
 * device become the feature-major block a keyed layer reads, and the inverse of the gray mapping -- public numbers, one pair per image -- is applied in the same launch.
 *   img_dev   n frames of D = c * h * w elements: bytes for depth 8, uint16_t in host byte order for depth 16; layout codes as kn_u8_to_linear's (0: NCHW, 1: NHWC)
 *   out_dev   the feature-major block.  For b < n and row r = (ch * h + y) * w + x:
 *                 t = (float)img[b][..]                                    exact at both depths
 *                 t = scale[b] * t                                         one IEEE f32 multiply
 *                 t = t + offset[b]                                        one IEEE f32 add: never fused with the multiply
 *                 out[r * ldo + b] = t
 *             out[D * ldo + b] = 1.0f for b < n (the ones row); every row, the ones row included, is +0.0f for n <= b < n_cols: a zero image is a zero image, it is NOT
 *             offset; columns n_cols <= b < ldo are not touched.
 *   scale_dev, offset_dev   n device floats each; scale_dev == NULL means no multiply, offset_dev == NULL means no add.  With both NULL and depth == 8 the block is
 *             bit-equal to kn_u8_to_linear's.
 * Refusals as kn_u8_to_linear's -- 1 <= n <= n_cols <= ldo and c, h, w >= 1 (KN_ERR_SHAPE), layout 0 or 1 and non-NULL img_dev, out_dev (KN_ERR_INVALID) -- and: a depth other
 * than 8 or 16 is KN_ERR_UNSUPPORTED, 16-bit frames at an address that is not a multiple of two KN_ERR_INVALID.  Nothing is launched on a refusal.  Every address is formed in
 * 64 bits.  The call allocates nothing and does not wait for the device: it can be captured into a HIP graph.  Tiled through LDS as the stored integers (256 bytes of a frame
 * x 64 images: 256 positions at 8 bits, 128 at 16): contiguous reads along a frame -- a dword per lane where the frame size in bytes and img_dev are multiples of four, one
 * element per lane otherwise -- and one 16-byte store along the batch per lane where ldo and out_dev are multiples of four floats, scalar stores otherwise.  An added entry
 * point: KN_ABI_VERSION stays (the rule below). */
int kn_frames_to_linear(const void* img_dev, int depth, int64_t n, int64_t c, int64_t h, int64_t w, int layout,
                        const float* scale_dev, const float* offset_dev,
                        float* out_dev, int64_t ldo, int64_t n_cols, void* stream);

/* kn_linear_to_u8 at 16 bits, the egress a float image key needs (half a gray step of an 8-bit encrypted image is 0.2 % of its range on every feature; 16 bits bring that down
 * 257-fold).  Arguments, layouts and refusals are kn_linear_to_u8's, with n frames of D uint16_t in host byte order.  For b < n:
 *                 t = gain[b] * x[((ch * h + y) * w + x) * ldx + b]        one IEEE f32 multiply
 *                 t = t + bias[b]                                          one IEEE f32 add: never fused with the multiply
 *                 img[b][..] = 0 if t is NaN, else min(65535, max(0, rint(t)))  round to nearest, ties to even; -Inf -> 0, +Inf -> 65535
 * gain_dev == NULL means 1.0f, bias_dev == NULL means 0.0f; halfwords outside the n * D of the frames are not touched; an img_dev that is not a multiple of two is
 * KN_ERR_INVALID.  The same LDS tile at 128 frame positions x 64 images; stores along a frame are a dword per lane where 2 * D and img_dev are multiples of four bytes, halfwords
 * otherwise.  No workspace; allocates nothing, does not wait for the device.  An added entry point: KN_ABI_VERSION stays (the rule below). */
int kn_linear_to_u16(const float* x_dev, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout,
                     const float* gain_dev, const float* bias_dev, uint16_t* img_dev, void* stream);

/* keynet.torch.linear_to_affine (keynet/torch.py:71-77): y_dev [d+1, n] feature-major -> out_dev [n, d] row-major;
 * *maxdev_dev (device float, may be NULL) receives max_b |y[d, b] - 1| so the host can raise ValueError when > 1e-3. */
int kn_linear_to_affine(const float* y_dev, int64_t ldy, int64_t n, int64_t d, float* out_dev, float* maxdev_dev, void* stream);

/* Planes <-> columns of a narrow batch.  No reference counterpart: the reference applies the fused operator (keynet/sparse.py:603-612), at one image
 * (keynet/system.py:130-133).  They serve the narrow split route of a FILLED-IN conv (keynet_amd/sparse.py, Conv2dTiledMatrix._torchdot_split_narrow; the opt-in keyword
 * narrow_split=True of the low-latency forward at 1 .. 32 images): with so few images the input-channel planes ARE the batch of the spatial matrix, so the activation block
 * X [Cin x HiWi, n] is laid out as Xt [HiWi, Cin x n], ONE kn_spmm of the spatial CSR runs at n_vecs = Cin x n (64 .. 16 384 columns, the width the CSR kernels are built
 * for, where kn_spmm_planes at n columns uses n lanes in 64), and its result goes back to planes for the channel-mixing conv-taps operator.
 *   kn_planes_to_columns:  in[p][r][b]  at in_dev + p * plane_stride + r * ld + b     ->   out[r][(p, b)] at out_dev + r * ld_out + p * n_vecs + b
 *   kn_columns_to_planes:  in[r][(p, b)] at in_dev + r * ld_in + p * n_vecs + b        ->   out[p][r][b]  at out_dev + p * plane_stride + r * ld + b
 * for p < n_planes, r < rows, b < n_vecs.  Pure data movement (no arithmetic: NaN payloads and -0 pass through); elements outside the written windows are untouched;
 * every address is formed in 64 bits (a plane may begin beyond 2^31 elements).  1 <= n_vecs <= 32 (KN_ERR_UNSUPPORTED beyond: not a narrow batch), any n_planes and rows,
 * any ld >= n_vecs, ld_in / ld_out >= n_planes * n_vecs, plane_stride >= (rows - 1) * ld + n_vecs (KN_ERR_SHAPE otherwise).  Tiled through LDS: 16 bytes per lane on a side
 * whose base and strides are multiples of four floats (the planes side also needs ld == n_vecs or n_vecs % 4 == 0), one float per lane otherwise.
 * ABI: entry points ADDED to the library leave KN_ABI_VERSION where it is -- the number moves when something a caller of the previous version relies on changes (a
 * signature, the meaning of a flag or of an argument); a binding that needs a newer entry point than a stale library has fails to resolve the symbol when it loads it. */
int kn_planes_to_columns(const float* in_dev, int64_t plane_stride, int64_t ld, int64_t n_planes, int64_t rows, int64_t n_vecs, float* out_dev, int64_t ld_out, void* stream);
int kn_columns_to_planes(const float* in_dev, int64_t ld_in, int64_t n_planes, int64_t rows, int64_t n_vecs, float* out_dev, int64_t plane_stride, int64_t ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEYNET_HIP_H */
