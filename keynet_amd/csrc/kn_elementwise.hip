// kn_elementwise.hip -- the memory-bound glue of the keyed forward (gfx950).
//   relu_inplace        nn.ReLU over [rows, n_vecs] incl. the homogeneous row (keynet/system.py:92) when it cannot be fused
//   affine_to_linear    keynet/torch.py:65-68 + the x.t() of keynet/layer.py:92: [n, d] images -> [d+1, n] feature-major
//   linear_to_affine    keynet/torch.py:71-77: [d+1, n] -> [n, d], plus max |last row - 1| for the host-side ValueError
//   u8_to_linear        the sensor's ingest of raw frames (keynet/system.py:183-201 + keynet/torch.py:65-68): n uint8 frames, NCHW or NHWC -> [d+1, n_cols] feature-major, padded
//   linear_to_u8        the sensor's egress (keynet/system.py:173-181, 223-228 + keynet/torch.py:71-77): n columns of a [d+1, ldx] block -> n uint8 frames, NCHW or NHWC, saturate(rint(gain * x + bias))
//   frames_to_linear    the dequantising ingest of ENCRYPTED frames (no reference counterpart: the wire between keynet/system.py:173-181 on the sensor and the key-net): n uint8 or uint16 frames -> [d+1, n_cols], offset + scale * (float)img per image
//   linear_to_u16       linear_to_u8 at 16 bits: saturate(rint(gain * x + bias)) into uint16 frames
//   column_range        the per-image minimum and maximum mat2gray takes (keynet/sparse.py:27), NaN skipped
//   planes_to_columns / columns_to_planes   the two layout changes around the spatial CSR of the narrow split route (no reference counterpart)
// Transposes go through a padded 64x65 LDS tile so both the global read and the global write are coalesced.
#include "kn_internal.h"

namespace kn {

__global__ __launch_bounds__(256) void relu_kernel(float* __restrict__ y, int64_t rows, int64_t ld, int64_t n_vecs) {
    const int64_t total = rows * n_vecs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_vecs;
        const int64_t c = i - r * n_vecs;
        float v = y[r * ld + c];
        y[r * ld + c] = (v < 0.0f) ? 0.0f : v;
    }
}

__global__ __launch_bounds__(256) void relu_kernel_v4(float4* __restrict__ y, int64_t total4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = y[i];
        v.x = (v.x < 0.0f) ? 0.0f : v.x;
        v.y = (v.y < 0.0f) ? 0.0f : v.y;
        v.z = (v.z < 0.0f) ? 0.0f : v.z;
        v.w = (v.w < 0.0f) ? 0.0f : v.w;
        y[i] = v;
    }
}

int relu_inplace(float* y, int64_t rows, int64_t ld, int64_t n_vecs, hipStream_t s) {
    if (rows <= 0 || n_vecs <= 0) return KN_OK;
    if (ld == n_vecs && (rows * n_vecs) % 4 == 0 && ((uintptr_t)y) % 16 == 0) {
        const int64_t total4 = rows * n_vecs / 4;
        const int64_t grid = std::min<int64_t>((total4 + 255) / 256, 2048);
        hipLaunchKernelGGL(relu_kernel_v4, dim3((unsigned)grid), dim3(256), 0, s, reinterpret_cast<float4*>(y), total4);
    } else {
        const int64_t grid = std::min<int64_t>((rows * n_vecs + 255) / 256, 2048);
        hipLaunchKernelGGL(relu_kernel, dim3((unsigned)grid), dim3(256), 0, s, y, rows, ld, n_vecs);
    }
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// in [R, C] row-major (ld_in) -> out [C, R] row-major (ld_out); 64x64 tiles, 256 threads (64 x 4)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int64_t R, int64_t C, int64_t ld_in, float* __restrict__ out,
                                                        int64_t ld_out) {
    __shared__ float tile[64][65];
    const int64_t c0 = (int64_t)blockIdx.x * 64;
    const int64_t r0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63;
    const int ty = threadIdx.x >> 6;
    for (int k = ty; k < 64; k += 4) {
        const int64_t r = r0 + k, c = c0 + tx;
        if (r < R && c < C) tile[k][tx] = in[r * ld_in + c];
    }
    __syncthreads();
    for (int k = ty; k < 64; k += 4) {
        const int64_t c = c0 + k, r = r0 + tx;
        if (r < R && c < C) out[c * ld_out + r] = tile[tx][k];
    }
}

__global__ __launch_bounds__(256) void fill_row_kernel(float* __restrict__ row, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) row[i] = v;
}

// y[o, b] = (sum_s z[o*S + s, b], s ascending) + lastcol[o] * xlast[b]   (+ReLU);  y[outs, b] = lastcol[outs] * xlast[b]
__global__ __launch_bounds__(256) void dense_reduce_kernel(const float* __restrict__ z, int64_t ldz, int64_t outs, int splits, const float* __restrict__ lastcol,
                                                           const float* __restrict__ xlast, float* __restrict__ y, int64_t ldy, int64_t n_vecs, int relu) {
    const int64_t total = (outs + 1) * n_vecs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = i / n_vecs;
        const int64_t b = i - o * n_vecs;
        float acc = 0.0f;
        if (o < outs) {
            const float* zp = z + (o * splits) * ldz + b;
            for (int s = 0; s < splits; s++) acc = acc + zp[(int64_t)s * ldz];
        }
        const float bp = lastcol[o] * xlast[b];
        acc = acc + bp;
        if (relu) acc = (acc < 0.0f) ? 0.0f : acc;
        y[o * ldy + b] = acc;
    }
}

int dense_reduce(const float* z, int64_t ldz, int64_t outs, int64_t splits, const float* lastcol, const float* xlast, float* y, int64_t ldy, int64_t n_vecs,
                 int relu, hipStream_t s) {
    const int64_t total = (outs + 1) * n_vecs;
    const int64_t grid = std::min<int64_t>((total + 255) / 256, 4096);
    KN_LAUNCH("dense_reduce_kernel", dense_reduce_kernel, dim3((unsigned)grid), dim3(256), 0, s, z, ldz, outs, (int)splits, lastcol, xlast, y, ldy, n_vecs, relu);
    KN_HIP(hipGetLastError());
    return KN_OK;
}

int affine_to_linear(const float* x, int64_t n, int64_t d, float* out, int64_t ldo, hipStream_t s) {
    if (n <= 0) return KN_OK;
    if (d > 0) {
        dim3 grid((unsigned)((d + 63) / 64), (unsigned)((n + 63) / 64));
        hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, s, x, n, d, d, out, ldo);
    }
    hipLaunchKernelGGL(fill_row_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, s, out + d * ldo, n, 1.0f);
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// kn_u8_to_linear: n uint8 frames of D = c * h * w bytes each -> the feature-major block [D + 1, n_cols] (ones row appended, columns n .. n_cols - 1 zero images).
// The byte at position p of a frame belongs to row r(p): p itself for NCHW; for NHWC p = (y * w + x) * c + ch and r = ch * (h * w) + (y * w + x).
// One workgroup moves a tile of U8_POS = 256 frame positions x U8_COLS = 64 images through LDS, kept as BYTES (16.6 KB, nine workgroups on a CU):
//   in    a wavefront reads 256 contiguous bytes of one frame per instruction -- one dword per lane where the frames are dword-aligned (D % 4 == 0 and the
//         base), one byte per lane otherwise -- and stores them at tile[image][position].  An image's row is 260 bytes = 65 dwords, so image i starts in bank
//         i (mod 32): the dword stores of a wavefront fall on consecutive banks, conflict-free.
//   out   lane (g = lane / 4, q = lane % 4) owns images 4g .. 4g + 3 at position 4 * (pass, wave) + q: four byte reads from dwords (4g + k) * 65 + position / 4
//         -- in a half-wave (g = 0 .. 7) 8 distinct banks per k, the four q of one g on ONE dword (a broadcast) -- converted (v_cvt_f32_ubyte: exact) and stored as one
//         float4, 16 lanes x 16 bytes = 256 contiguous bytes of an output row per wavefront.  The row permutation of NHWC is this side's index arithmetic: the
//         row changes, the 256-byte run along the batch does not.  V4 = false (ldo or the base not a multiple of four floats): four scalar stores; a quad that
//         crosses n_cols stores scalars up to it either way, so columns n_cols .. ldo - 1 are never touched.
// Position tile 0 of every column tile also writes the ones row.  No arithmetic but the conversion; every address is formed in 64 bits.
constexpr int U8_POS = 256, U8_COLS = 64, U8_STRIDE = U8_POS + 4;

template <bool V4>
__device__ __forceinline__ void u8_store_quad(float* __restrict__ row, int64_t b, int64_t n_cols, float4 v) {
    if (V4 && b + 4 <= n_cols) {
        *reinterpret_cast<float4*>(row + b) = v;
    } else {
        if (b < n_cols) row[b] = v.x;
        if (b + 1 < n_cols) row[b + 1] = v.y;
        if (b + 2 < n_cols) row[b + 2] = v.z;
        if (b + 3 < n_cols) row[b + 3] = v.w;
    }
}

template <bool NHWC, bool L4, bool V4>
__global__ __launch_bounds__(256) void u8_to_linear_kernel(const uint8_t* __restrict__ img, int64_t n, int64_t D, int c, int64_t hw, float* __restrict__ out, int64_t ldo,
                                                           int64_t n_cols) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[U8_COLS * U8_STRIDE];
    const int64_t p0 = (int64_t)blockIdx.x * U8_POS;
    const int64_t b0 = (int64_t)blockIdx.y * U8_COLS;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int cols = (n_cols - b0 < U8_COLS) ? (int)(n_cols - b0) : U8_COLS;        // columns of this tile that exist: >= 1
    // in: images beyond n (the pad columns) are zero bytes
    if (L4) {
        const int64_t p = p0 + 4 * lane;
        for (int i = wave; i < cols; i += 4) {
            uint32_t v = 0;
            if (b0 + i < n && p < D) v = *reinterpret_cast<const uint32_t*>(img + (b0 + i) * D + p);      // D % 4 == 0: a dword is inside the frame or outside it
            *reinterpret_cast<uint32_t*>(tile + i * U8_STRIDE + 4 * lane) = v;
        }
    } else {
        const int64_t p = p0 + (int)threadIdx.x;
        for (int i = 0; i < cols; i++) {
            uint8_t v = 0;
            if (b0 + i < n && p < D) v = img[(b0 + i) * D + p];
            tile[i * U8_STRIDE + (int)threadIdx.x] = v;
        }
    }
    __syncthreads();
    // out
    const int g = lane >> 2, q = lane & 3;
    const int64_t b = b0 + 4 * g;
    if (4 * g < cols) {
        for (int pass = 0; pass < U8_POS / 16; pass++) {
            const int pl = pass * 16 + wave * 4 + q;
            const int64_t p = p0 + pl;
            if (p >= D) break;                              // positions ascend with the pass
            int64_t r = p;
            if (NHWC) {
                const int64_t pix = p / c;
                r = (p - pix * c) * hw + pix;
            }
            const uint8_t* t = tile + (4 * g) * U8_STRIDE + pl;
            float4 v;
            v.x = (float)t[0];
            v.y = (4 * g + 1 < cols) ? (float)t[U8_STRIDE] : 0.0f;
            v.z = (4 * g + 2 < cols) ? (float)t[2 * U8_STRIDE] : 0.0f;
            v.w = (4 * g + 3 < cols) ? (float)t[3 * U8_STRIDE] : 0.0f;
            u8_store_quad<V4>(out + r * ldo, b, n_cols, v);
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < 16 && 4 * (int)threadIdx.x < cols) {       // the ones row: 1.0 under an image, 0.0 under a pad column
        const int64_t bq = b0 + 4 * (int)threadIdx.x;
        float4 v;
        v.x = (bq < n) ? 1.0f : 0.0f;
        v.y = (bq + 1 < n) ? 1.0f : 0.0f;
        v.z = (bq + 2 < n) ? 1.0f : 0.0f;
        v.w = (bq + 3 < n) ? 1.0f : 0.0f;
        u8_store_quad<V4>(out + D * ldo, bq, n_cols, v);
    }
}

int u8_to_linear(const uint8_t* img, int64_t n, int64_t c, int64_t h, int64_t w, int layout, float* out, int64_t ldo, int64_t n_cols, hipStream_t s) {
    const int64_t D = c * h * w;
    const int64_t ptiles = (D + U8_POS - 1) / U8_POS, ctiles = (n_cols + U8_COLS - 1) / U8_COLS;
    if (ptiles > INT32_MAX || ctiles > 65535) return fail(KN_ERR_UNSUPPORTED, "kn_u8_to_linear: more tiles than one launch grid holds");
    const bool nhwc = layout == 1 && c > 1;                // one channel: the two layouts are the same bytes
    const bool l4 = D % 4 == 0 && ((uintptr_t)img) % 4 == 0;
    const bool v4 = ldo % 4 == 0 && ((uintptr_t)out) % 16 == 0;
    const dim3 grid((unsigned)ptiles, (unsigned)ctiles);
#define KN_U8_LAUNCH(NHWC, L4, V4) \
    KN_LAUNCH("u8_to_linear_kernel<" #NHWC "," #L4 "," #V4 ">", (u8_to_linear_kernel<NHWC, L4, V4>), grid, dim3(256), 0, s, img, n, D, (int)c, h * w, out, ldo, n_cols)
    if (nhwc) {
        if (l4 && v4) KN_U8_LAUNCH(true, true, true);
        else if (l4) KN_U8_LAUNCH(true, true, false);
        else if (v4) KN_U8_LAUNCH(true, false, true);
        else KN_U8_LAUNCH(true, false, false);
    } else {
        if (l4 && v4) KN_U8_LAUNCH(false, true, true);
        else if (l4) KN_U8_LAUNCH(false, true, false);
        else if (v4) KN_U8_LAUNCH(false, false, true);
        else KN_U8_LAUNCH(false, false, false);
    }
#undef KN_U8_LAUNCH
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// kn_frames_to_linear: the dequantising ingest -- kn_u8_to_linear for frames of T = uint8_t or uint16_t with a per-image affine on the way out,
// out = offset[b] + scale[b] * (float)img (a separate multiply and add; either pointer NULL: that statement is left out).  The structure is u8_to_linear_kernel's, with
// the tile kept as stored integers: FR_POS<T> = 256 / sizeof(T) frame positions x U8_COLS = 64 images, so an image's row is again 256 + 4 bytes = 65 dwords and the bank
// argument above carries over: image i starts in bank i (mod 32), the dword stores of a wavefront fall on consecutive banks, and on the way out the four q of one g read one
// dword (bytes) or two neighbouring dwords (halfwords) of 8 distinct rows -- 8 or 16 distinct banks per instruction.
//   in    a wavefront reads 256 contiguous bytes of one frame per instruction: a dword per lane (four bytes or two halfwords) where the frame size in bytes and the base
//         are multiples of four, one element per lane otherwise (at 16 bits the 256 threads then cover two images per step).
//   out   lane (g, q) owns images 4g .. 4g + 3; it loads their four scale / offset pairs once, before the pass loop, converts (exact at both depths), multiplies, adds and
//         stores one float4 along the batch.  A pad column (n <= b < n_cols) is +0.0f whatever the offset: a zero image, not a black one.
template <typename T>
constexpr int FR_POS = U8_POS / (int)sizeof(T);

template <typename T, bool NHWC, bool L4, bool V4>
__global__ __launch_bounds__(256) void frames_to_linear_kernel(const T* __restrict__ img, int64_t n, int64_t D, int c, int64_t hw, const float* __restrict__ scale,
                                                               const float* __restrict__ offset, float* __restrict__ out, int64_t ldo, int64_t n_cols) {
    constexpr int POS = FR_POS<T>, EPD = 4 / (int)sizeof(T);                        // positions of a tile, elements per dword
    __shared__ __attribute__((aligned(16))) uint8_t tile[U8_COLS * U8_STRIDE];
    const int64_t p0 = (int64_t)blockIdx.x * POS;
    const int64_t b0 = (int64_t)blockIdx.y * U8_COLS;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int cols = (n_cols - b0 < U8_COLS) ? (int)(n_cols - b0) : U8_COLS;        // columns of this tile that exist: >= 1
    // in: images beyond n (the pad columns) are zero elements
    if (L4) {
        const int64_t p = p0 + EPD * lane;
        for (int i = wave; i < cols; i += 4) {
            uint32_t v = 0;
            if (b0 + i < n && p < D) v = *reinterpret_cast<const uint32_t*>(img + (b0 + i) * D + p);      // D % EPD == 0: a dword is inside the frame or outside it
            *reinterpret_cast<uint32_t*>(tile + i * U8_STRIDE + 4 * lane) = v;
        }
    } else {
        const int pl = (int)threadIdx.x % POS;
        const int64_t p = p0 + pl;
        for (int i = (int)threadIdx.x / POS; i < cols; i += 256 / POS) {
            T v = 0;
            if (b0 + i < n && p < D) v = img[(b0 + i) * D + p];
            *reinterpret_cast<T*>(tile + i * U8_STRIDE + pl * (int)sizeof(T)) = v;
        }
    }
    __syncthreads();
    // out
    const int g = lane >> 2, q = lane & 3;
    const int64_t b = b0 + 4 * g;
    if (4 * g < cols) {
        const bool mul = scale != nullptr, add = offset != nullptr;
        bool live[4];
        float sc[4], of[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            live[k] = b + k < n;
            sc[k] = (mul && live[k]) ? scale[b + k] : 1.0f;
            of[k] = (add && live[k]) ? offset[b + k] : 0.0f;
        }
        for (int pass = 0; pass < POS / 16; pass++) {
            const int pl = pass * 16 + wave * 4 + q;
            const int64_t p = p0 + pl;
            if (p >= D) break;                              // positions ascend with the pass
            int64_t r = p;
            if (NHWC) {
                const int64_t pix = p / c;
                r = (p - pix * c) * hw + pix;
            }
            const uint8_t* t = tile + (4 * g) * U8_STRIDE + pl * (int)sizeof(T);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float x = 0.0f;
                if (live[k]) {
                    x = (float)*reinterpret_cast<const T*>(t + k * U8_STRIDE);
                    if (mul) x = __fmul_rn(sc[k], x);
                    if (add) x = __fadd_rn(x, of[k]);
                }
                v[k] = x;
            }
            u8_store_quad<V4>(out + r * ldo, b, n_cols, make_float4(v[0], v[1], v[2], v[3]));
        }
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < 16 && 4 * (int)threadIdx.x < cols) {       // the ones row: 1.0 under an image, 0.0 under a pad column
        const int64_t bq = b0 + 4 * (int)threadIdx.x;
        float4 v;
        v.x = (bq < n) ? 1.0f : 0.0f;
        v.y = (bq + 1 < n) ? 1.0f : 0.0f;
        v.z = (bq + 2 < n) ? 1.0f : 0.0f;
        v.w = (bq + 3 < n) ? 1.0f : 0.0f;
        u8_store_quad<V4>(out + D * ldo, bq, n_cols, v);
    }
}

template <typename T>
static int frames_to_linear_t(const T* img, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* scale, const float* offset, float* out, int64_t ldo,
                              int64_t n_cols, hipStream_t s) {
    const int64_t D = c * h * w;
    const int64_t ptiles = (D + FR_POS<T> - 1) / FR_POS<T>, ctiles = (n_cols + U8_COLS - 1) / U8_COLS;
    if (ptiles > INT32_MAX || ctiles > 65535) return fail(KN_ERR_UNSUPPORTED, "kn_frames_to_linear: more tiles than one launch grid holds");
    const bool nhwc = layout == 1 && c > 1;                // one channel: the two layouts are the same elements
    const bool l4 = (D * (int64_t)sizeof(T)) % 4 == 0 && ((uintptr_t)img) % 4 == 0;
    const bool v4 = ldo % 4 == 0 && ((uintptr_t)out) % 16 == 0;
    const dim3 grid((unsigned)ptiles, (unsigned)ctiles);
    const char* name = sizeof(T) == 1 ? "frames_to_linear_kernel<u8>" : "frames_to_linear_kernel<u16>";
#define KN_FR_LAUNCH(NHWC, L4, V4) \
    KN_LAUNCH(name, (frames_to_linear_kernel<T, NHWC, L4, V4>), grid, dim3(256), 0, s, img, n, D, (int)c, h * w, scale, offset, out, ldo, n_cols)
    if (nhwc) {
        if (l4 && v4) KN_FR_LAUNCH(true, true, true);
        else if (l4) KN_FR_LAUNCH(true, true, false);
        else if (v4) KN_FR_LAUNCH(true, false, true);
        else KN_FR_LAUNCH(true, false, false);
    } else {
        if (l4 && v4) KN_FR_LAUNCH(false, true, true);
        else if (l4) KN_FR_LAUNCH(false, true, false);
        else if (v4) KN_FR_LAUNCH(false, false, true);
        else KN_FR_LAUNCH(false, false, false);
    }
#undef KN_FR_LAUNCH
    KN_HIP(hipGetLastError());
    return KN_OK;
}

int frames_to_linear(const void* img, int depth, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* scale, const float* offset, float* out, int64_t ldo,
                     int64_t n_cols, hipStream_t s) {
    if (depth == 8) return frames_to_linear_t(static_cast<const uint8_t*>(img), n, c, h, w, layout, scale, offset, out, ldo, n_cols, s);
    return frames_to_linear_t(static_cast<const uint16_t*>(img), n, c, h, w, layout, scale, offset, out, ldo, n_cols, s);
}

// kn_linear_to_u8: kn_u8_to_linear run backwards -- the first n columns of a feature-major block [D (+ the ones row, not read), ldx] -> n uint8 frames of D bytes,
// img = saturate(rint(gain[b] * x + bias[b])).  The same tile: U8_POS = 256 OUTPUT byte positions x U8_COLS = 64 images, parked in LDS as BYTES, tile[image][position],
// an image's row 260 bytes = 65 dwords.
//   in    lane (g = lane / 4, q = lane % 4) owns images 4g .. 4g + 3 at the four positions of quad j = 16 * pass + 4 * wave + q: four loads, one per position, each a
//         float4 along the batch -- 16 lanes x 16 bytes = 256 contiguous bytes of one feature row, four rows per wave instruction (V4 = false, ldx or the base not a
//         multiple of four floats: scalar loads; a quad that crosses n loads scalars up to it either way, so columns n .. ldx - 1 are never read).  Multiply, add
//         (separate roundings: the build is -ffp-contract=off and the two are __fmul_rn / __fadd_rn), rint, saturate.  Storing each byte on its own would put the
//         four q of one g -- four positions of one image that share a dword -- on ONE bank with four addresses, every store instruction 4-way conflicted, sixteen of
//         them per lane and pass; instead the lane packs the four positions of an image into a dword and stores four dwords: dword (4g + k) * 65 + j is in bank
//         4g + k + j (mod 32), and over a half-wave (g = 0 .. 7, q = 0 .. 3, k fixed) 4g + q + const takes every one of the 32 banks once -- conflict-free.
//         Under NHWC the row of output position p = (y * w + x) * c + ch is ch * (h * w) + (y * w + x): one division per quad, then steps of one channel.
//   out   a wavefront writes 256 contiguous bytes of one frame, one dword per lane from consecutive banks (S4: D % 4 == 0 and a dword-aligned base, so a dword is
//         inside the frame or outside it), one byte per lane otherwise (the four lanes of a dword read it as a broadcast).
// Each lane loads the gain and bias of its four images once, before the passes.  No workspace; every address is formed in 64 bits; bytes outside the n * D are not touched.
__device__ __forceinline__ uint32_t u8_saturate(float t) {
    const float r = rintf(t);                               // v_rndne_f32: ties to even
    return (t != t) ? 0u : (uint32_t)(int)fminf(255.0f, fmaxf(0.0f, r));
}

template <bool NHWC, bool V4, bool S4>
__global__ __launch_bounds__(256) void linear_to_u8_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int64_t D, int c, int64_t hw, const float* __restrict__ gain,
                                                           const float* __restrict__ bias, uint8_t* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[U8_COLS * U8_STRIDE];
    const int64_t p0 = (int64_t)blockIdx.x * U8_POS;
    const int64_t b0 = (int64_t)blockIdx.y * U8_COLS;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int cols = (n - b0 < U8_COLS) ? (int)(n - b0) : U8_COLS;                  // images of this tile: >= 1
    // in
    const int g = lane >> 2, q = lane & 3;
    const int64_t b = b0 + 4 * g;
    if (4 * g < cols) {
        float gn[4], bs[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            gn[k] = (gain && b + k < n) ? gain[b + k] : 1.0f;
            bs[k] = (bias && b + k < n) ? bias[b + k] : 0.0f;
        }
        for (int pass = 0; pass < U8_POS / 64; pass++) {
            const int j = pass * 16 + wave * 4 + q;
            const int64_t p = p0 + 4 * j;
            if (p >= D) break;                              // positions ascend with the pass
            int64_t pix = 0;
            int ch = 0;
            if (NHWC) {
                if (D <= (int64_t)INT32_MAX) {
                    const uint32_t px = (uint32_t)p / (uint32_t)c;
                    pix = px;
                    ch = (int)((uint32_t)p - px * (uint32_t)c);
                } else {
                    pix = p / c;
                    ch = (int)(p - pix * c);
                }
            }
            uint32_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p + i < D) {
                    const int64_t r = NHWC ? (int64_t)ch * hw + pix : p + i;
                    const float* row = x + r * ldx;
                    if (V4 && b + 4 <= n) {
                        v = *reinterpret_cast<const float4*>(row + b);
                    } else {
                        v.x = row[b];                                               // b < n: 4g < cols
                        if (b + 1 < n) v.y = row[b + 1];
                        if (b + 2 < n) v.z = row[b + 2];
                        if (b + 3 < n) v.w = row[b + 3];
                    }
                }
                word[0] |= u8_saturate(__fadd_rn(__fmul_rn(gn[0], v.x), bs[0])) << (8 * i);
                word[1] |= u8_saturate(__fadd_rn(__fmul_rn(gn[1], v.y), bs[1])) << (8 * i);
                word[2] |= u8_saturate(__fadd_rn(__fmul_rn(gn[2], v.z), bs[2])) << (8 * i);
                word[3] |= u8_saturate(__fadd_rn(__fmul_rn(gn[3], v.w), bs[3])) << (8 * i);
                if (NHWC && ++ch == c) {
                    ch = 0;
                    pix++;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) *reinterpret_cast<uint32_t*>(tile + (4 * g + k) * U8_STRIDE + 4 * j) = word[k];     // images cols .. 4g + 3: rows of the tile nothing reads
        }
    }
    __syncthreads();
    // out
    if (S4) {
        const int64_t p = p0 + 4 * lane;
        if (p < D)
            for (int i = wave; i < cols; i += 4) *reinterpret_cast<uint32_t*>(img + (b0 + i) * D + p) = *reinterpret_cast<const uint32_t*>(tile + i * U8_STRIDE + 4 * lane);
    } else {
        const int64_t p = p0 + (int)threadIdx.x;
        if (p < D)
            for (int i = 0; i < cols; i++) img[(b0 + i) * D + p] = tile[i * U8_STRIDE + (int)threadIdx.x];
    }
}

int linear_to_u8(const float* x, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* gain, const float* bias, uint8_t* img, hipStream_t s) {
    const int64_t D = c * h * w;
    const int64_t ptiles = (D + U8_POS - 1) / U8_POS, ctiles = (n + U8_COLS - 1) / U8_COLS;
    if (ptiles > INT32_MAX || ctiles > 65535) return fail(KN_ERR_UNSUPPORTED, "kn_linear_to_u8: more tiles than one launch grid holds");
    const bool nhwc = layout == 1 && c > 1;                // one channel: the two layouts are the same bytes
    const bool v4 = ldx % 4 == 0 && ((uintptr_t)x) % 16 == 0;
    const bool s4 = D % 4 == 0 && ((uintptr_t)img) % 4 == 0;
    const dim3 grid((unsigned)ptiles, (unsigned)ctiles);
#define KN_L8_LAUNCH(NHWC, V4, S4) \
    KN_LAUNCH("linear_to_u8_kernel<" #NHWC "," #V4 "," #S4 ">", (linear_to_u8_kernel<NHWC, V4, S4>), grid, dim3(256), 0, s, x, ldx, n, D, (int)c, h * w, gain, bias, img)
    if (nhwc) {
        if (v4 && s4) KN_L8_LAUNCH(true, true, true);
        else if (v4) KN_L8_LAUNCH(true, true, false);
        else if (s4) KN_L8_LAUNCH(true, false, true);
        else KN_L8_LAUNCH(true, false, false);
    } else {
        if (v4 && s4) KN_L8_LAUNCH(false, true, true);
        else if (v4) KN_L8_LAUNCH(false, true, false);
        else if (s4) KN_L8_LAUNCH(false, false, true);
        else KN_L8_LAUNCH(false, false, false);
    }
#undef KN_L8_LAUNCH
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// kn_linear_to_u16: kn_linear_to_u8 at 16 bits, statement for statement, saturating at 65535.  The same LDS tile at U16_POS = 128 output positions x 64 images: an image's
// row is 128 halfwords + 4 bytes = 65 dwords.
//   in    as linear_to_u8_kernel: lane (g, q) owns images 4g .. 4g + 3 at the four positions of quad j = 16 * pass + 4 * wave + q (two passes), one float4 along the batch
//         per position; multiply, add (separate roundings), rint, saturate.  The four positions of an image are packed into TWO dwords, 2j and 2j + 1 of the image's row:
//         dword (4g + k) * 65 + 2j (+ 1) is in bank 4g + k + 2j (+ 1), and over a half-wave 4g + 2q takes the 16 even residues twice -- a 2-way conflict on each of
//         the eight store instructions of a pass, against twenty float4 loads and stores of global memory per lane: the kernel stays at the rate of its HBM traffic.
//   out   a wavefront writes 256 contiguous bytes of one frame: a dword (two halfwords) per lane where 2 * D and the base are multiples of four, one halfword per lane
//         otherwise (the 256 threads then cover two images per step).
// No workspace; every address is formed in 64 bits; halfwords outside the n * D are not touched.
constexpr int U16_POS = U8_POS / 2;

__device__ __forceinline__ uint32_t u16_saturate(float t) {
    const float r = rintf(t);                               // v_rndne_f32: ties to even
    return (t != t) ? 0u : (uint32_t)(int)fminf(65535.0f, fmaxf(0.0f, r));
}

template <bool NHWC, bool V4, bool S4>
__global__ __launch_bounds__(256) void linear_to_u16_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int64_t D, int c, int64_t hw, const float* __restrict__ gain,
                                                            const float* __restrict__ bias, uint16_t* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[U8_COLS * U8_STRIDE];
    const int64_t p0 = (int64_t)blockIdx.x * U16_POS;
    const int64_t b0 = (int64_t)blockIdx.y * U8_COLS;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int cols = (n - b0 < U8_COLS) ? (int)(n - b0) : U8_COLS;                  // images of this tile: >= 1
    // in
    const int g = lane >> 2, q = lane & 3;
    const int64_t b = b0 + 4 * g;
    if (4 * g < cols) {
        float gn[4], bs[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            gn[k] = (gain && b + k < n) ? gain[b + k] : 1.0f;
            bs[k] = (bias && b + k < n) ? bias[b + k] : 0.0f;
        }
        for (int pass = 0; pass < U16_POS / 64; pass++) {
            const int j = pass * 16 + wave * 4 + q;
            const int64_t p = p0 + 4 * j;
            if (p >= D) break;                              // positions ascend with the pass
            int64_t pix = 0;
            int ch = 0;
            if (NHWC) {
                if (D <= (int64_t)INT32_MAX) {
                    const uint32_t px = (uint32_t)p / (uint32_t)c;
                    pix = px;
                    ch = (int)((uint32_t)p - px * (uint32_t)c);
                } else {
                    pix = p / c;
                    ch = (int)(p - pix * c);
                }
            }
            uint32_t word[4][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p + i < D) {
                    const int64_t r = NHWC ? (int64_t)ch * hw + pix : p + i;
                    const float* row = x + r * ldx;
                    if (V4 && b + 4 <= n) {
                        v = *reinterpret_cast<const float4*>(row + b);
                    } else {
                        v.x = row[b];                                               // b < n: 4g < cols
                        if (b + 1 < n) v.y = row[b + 1];
                        if (b + 2 < n) v.z = row[b + 2];
                        if (b + 3 < n) v.w = row[b + 3];
                    }
                }
                word[0][i >> 1] |= u16_saturate(__fadd_rn(__fmul_rn(gn[0], v.x), bs[0])) << (16 * (i & 1));
                word[1][i >> 1] |= u16_saturate(__fadd_rn(__fmul_rn(gn[1], v.y), bs[1])) << (16 * (i & 1));
                word[2][i >> 1] |= u16_saturate(__fadd_rn(__fmul_rn(gn[2], v.z), bs[2])) << (16 * (i & 1));
                word[3][i >> 1] |= u16_saturate(__fadd_rn(__fmul_rn(gn[3], v.w), bs[3])) << (16 * (i & 1));
                if (NHWC && ++ch == c) {
                    ch = 0;
                    pix++;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {                                           // images cols .. 4g + 3: rows of the tile nothing reads
                uint32_t* t = reinterpret_cast<uint32_t*>(tile + (4 * g + k) * U8_STRIDE + 8 * j);
                t[0] = word[k][0];
                t[1] = word[k][1];
            }
        }
    }
    __syncthreads();
    // out
    if (S4) {
        const int64_t p = p0 + 2 * lane;
        if (p < D)
            for (int i = wave; i < cols; i += 4) *reinterpret_cast<uint32_t*>(img + (b0 + i) * D + p) = *reinterpret_cast<const uint32_t*>(tile + i * U8_STRIDE + 4 * lane);
    } else {
        const int pl = (int)threadIdx.x & (U16_POS - 1);
        const int64_t p = p0 + pl;
        if (p < D)
            for (int i = (int)threadIdx.x / U16_POS; i < cols; i += 256 / U16_POS) img[(b0 + i) * D + p] = *reinterpret_cast<const uint16_t*>(tile + i * U8_STRIDE + 2 * pl);
    }
}

int linear_to_u16(const float* x, int64_t ldx, int64_t n, int64_t c, int64_t h, int64_t w, int layout, const float* gain, const float* bias, uint16_t* img, hipStream_t s) {
    const int64_t D = c * h * w;
    const int64_t ptiles = (D + U16_POS - 1) / U16_POS, ctiles = (n + U8_COLS - 1) / U8_COLS;
    if (ptiles > INT32_MAX || ctiles > 65535) return fail(KN_ERR_UNSUPPORTED, "kn_linear_to_u16: more tiles than one launch grid holds");
    const bool nhwc = layout == 1 && c > 1;                // one channel: the two layouts are the same elements
    const bool v4 = ldx % 4 == 0 && ((uintptr_t)x) % 16 == 0;
    const bool s4 = D % 2 == 0 && ((uintptr_t)img) % 4 == 0;
    const dim3 grid((unsigned)ptiles, (unsigned)ctiles);
#define KN_L16_LAUNCH(NHWC, V4, S4) \
    KN_LAUNCH("linear_to_u16_kernel<" #NHWC "," #V4 "," #S4 ">", (linear_to_u16_kernel<NHWC, V4, S4>), grid, dim3(256), 0, s, x, ldx, n, D, (int)c, h * w, gain, bias, img)
    if (nhwc) {
        if (v4 && s4) KN_L16_LAUNCH(true, true, true);
        else if (v4) KN_L16_LAUNCH(true, true, false);
        else if (s4) KN_L16_LAUNCH(true, false, true);
        else KN_L16_LAUNCH(true, false, false);
    } else {
        if (v4 && s4) KN_L16_LAUNCH(false, true, true);
        else if (v4) KN_L16_LAUNCH(false, true, false);
        else if (s4) KN_L16_LAUNCH(false, false, true);
        else KN_L16_LAUNCH(false, false, false);
    }
#undef KN_L16_LAUNCH
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// kn_column_range: lo[b] = min, hi[b] = max over r < rows of x[r * ld + b], NaN skipped (keynet/sparse.py:27 per image: the input of mat2gray).  Lanes sit on columns, so a
// wavefront's load is contiguous along the batch: a column tile is cw = the power of two >= min(n_vecs, 64) columns wide, a lane owns VEC of them -- four, one 16-byte
// load, where ld and the base are multiples of four floats and the tile has four columns; one otherwise, and scalars in the quad that crosses n_vecs -- and thread t the
// rows t / (cw / VEC) (+ multiples of 256 * VEC / cw) of its row chunk: one image still fills its wavefronts, with 256 consecutive rows.  A thread's running pairs go to
// LDS, the first cw threads fold the partials of their column, and the row chunks meet in lo / hi through integer atomics on the float's bits: for a value with the sign bit clear
// signed-integer order is float order, and every negative float is a negative integer below it; for a value with the sign bit set unsigned order is reversed float order,
// and every non-negative float is an unsigned below it.  So min = (sign clear ? signed min : unsigned max), max = (sign clear ? signed max : unsigned min), each correct
// whatever the slot holds, +-Inf and the fill values included.  The slot is read first and the atomic issued only when it would change it (kn_wave_absmax_commit: why).
// Minimum and maximum are exact and commute: the result does not depend on the chunking.  column_range_fill_kernel initialises the outputs in the same stream.
__global__ __launch_bounds__(256) void column_range_fill_kernel(float* __restrict__ lo, float* __restrict__ hi, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        lo[i] = __builtin_huge_valf();
        hi[i] = -__builtin_huge_valf();
    }
}

__device__ __forceinline__ void atomic_min_f32(float* slot, float v) {
    if (!(v < __builtin_bit_cast(float, __atomic_load_n(reinterpret_cast<unsigned*>(slot), __ATOMIC_RELAXED)))) return;
    if ((int)__float_as_uint(v) >= 0) atomicMin(reinterpret_cast<int*>(slot), (int)__float_as_uint(v));
    else atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(v));
}

__device__ __forceinline__ void atomic_max_f32(float* slot, float v) {
    if (!(v > __builtin_bit_cast(float, __atomic_load_n(reinterpret_cast<unsigned*>(slot), __ATOMIC_RELAXED)))) return;
    if ((int)__float_as_uint(v) >= 0) atomicMax(reinterpret_cast<int*>(slot), (int)__float_as_uint(v));
    else atomicMin(reinterpret_cast<unsigned*>(slot), __float_as_uint(v));
}

template <int VEC>
__global__ __launch_bounds__(256) void column_range_kernel(const float* __restrict__ x, int64_t rows, int64_t ld, int64_t n_vecs, int cw, int64_t chunk_rows,
                                                           float* __restrict__ lo, float* __restrict__ hi) {
    __shared__ float red_lo[256 * VEC], red_hi[256 * VEC];
    const int t = (int)threadIdx.x;
    const int lpr = cw / VEC;                               // lanes per row of the tile: a power of two
    const int col = (t & (lpr - 1)) * VEC, rsub = t / lpr, step = 256 / lpr;
    const int64_t b = (int64_t)blockIdx.y * cw + col;
    const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t r1 = (rows - r0 < chunk_rows) ? rows : r0 + chunk_rows;
    float mn[VEC], mx[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
        mn[k] = __builtin_huge_valf();
        mx[k] = -__builtin_huge_valf();
    }
    if (VEC == 4 && b + 4 <= n_vecs) {
        const float* px = x + b;
#pragma unroll 4
        for (int64_t r = r0 + rsub; r < r1; r += step) {
            const float4 q = *reinterpret_cast<const float4*>(px + r * ld);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                mn[k] = (v[k] < mn[k]) ? v[k] : mn[k];      // a NaN compares false: skipped
                mx[k] = (v[k] > mx[k]) ? v[k] : mx[k];
            }
        }
    } else if (b < n_vecs) {                                // VEC == 1, or the quad that crosses n_vecs: scalars up to it
        const float* px = x + b;
#pragma unroll 4
        for (int64_t r = r0 + rsub; r < r1; r += step) {
#pragma unroll
            for (int k = 0; k < VEC; k++) {
                if (b + k < n_vecs) {
                    const float v = px[r * ld + k];
                    mn[k] = (v < mn[k]) ? v : mn[k];
                    mx[k] = (v > mx[k]) ? v : mx[k];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; k++) {
        red_lo[rsub * cw + col + k] = mn[k];                // [step][cw]: 256 * VEC floats
        red_hi[rsub * cw + col + k] = mx[k];
    }
    __syncthreads();
    const int64_t bt = (int64_t)blockIdx.y * cw + t;
    if (t < cw && bt < n_vecs) {
        float a = red_lo[t], z = red_hi[t];
        for (int k = 1; k < step; k++) {
            const float a2 = red_lo[k * cw + t], z2 = red_hi[k * cw + t];
            a = (a2 < a) ? a2 : a;
            z = (z2 > z) ? z2 : z;
        }
        atomic_min_f32(lo + bt, a);
        atomic_max_f32(hi + bt, z);
    }
}

int column_range(const float* x, int64_t rows, int64_t ld, int64_t n_vecs, float* lo, float* hi, hipStream_t s) {
    if (n_vecs <= 0) return KN_OK;
    KN_LAUNCH("column_range_fill_kernel", column_range_fill_kernel, dim3((unsigned)std::min<int64_t>((n_vecs + 255) / 256, 1024)), dim3(256), 0, s, lo, hi, n_vecs);
    if (rows > 0) {
        int cw = 1;
        while (cw < n_vecs && cw < 64) cw <<= 1;
        const int64_t ctiles = (n_vecs + cw - 1) / cw;
        if (ctiles > 65535) return fail(KN_ERR_UNSUPPORTED, "kn_column_range: more column tiles than one launch grid holds");
        const bool v4 = cw >= 4 && ld % 4 == 0 && ((uintptr_t)x) % 16 == 0;         // 16 bytes per lane: tile corners are multiples of four columns
        const int64_t step = 256 / (cw / (v4 ? 4 : 1));
        const int64_t want = std::max<int64_t>(1, 2048 / ctiles);                   // row chunks per column tile: ~2 048 workgroups in all
        int64_t chunk_rows = std::max<int64_t>((rows + want - 1) / want, 16 * step);
        chunk_rows = (chunk_rows + step - 1) / step * step;
        const int64_t chunks = (rows + chunk_rows - 1) / chunk_rows;               // <= want
        const dim3 grid((unsigned)chunks, (unsigned)ctiles);
        if (v4) KN_LAUNCH("column_range_kernel<4>", column_range_kernel<4>, grid, dim3(256), 0, s, x, rows, ld, n_vecs, cw, chunk_rows, lo, hi);
        else KN_LAUNCH("column_range_kernel<1>", column_range_kernel<1>, grid, dim3(256), 0, s, x, rows, ld, n_vecs, cw, chunk_rows, lo, hi);
    }
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// max over b of |y[d, b] - 1| ; single workgroup (n is a batch size)
__global__ __launch_bounds__(256) void lastrow_dev_kernel(const float* __restrict__ row, int64_t n, float* __restrict__ maxdev) {
    __shared__ float red[256];
    float m = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        float dv = fabsf(row[i] - 1.0f);
        m = (dv > m || dv != dv) ? dv : m;   // NaN wins so the host check fires
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
        if ((int)threadIdx.x < sft) {
            float o = red[threadIdx.x + sft];
            float a = red[threadIdx.x];
            red[threadIdx.x] = (o > a || o != o) ? o : a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *maxdev = red[0];
}

// max |y| over [rows, n_vecs] (leading dimension ld) raised into *absmax (kn_absmax; kn_spmm_screen after kernels that do not fold it into
// their stores).  NaN entries are ignored (max of the finite and infinite ones); grid-stride, 16 bytes per lane when the block is dense.
__global__ __launch_bounds__(256) void absmax_kernel_v4(const float4* __restrict__ y, int64_t total4, float* __restrict__ absmax) {
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = y[i];
        m = fmaxf(fmaxf(m, fabsf(v.x)), fabsf(v.y));
        m = fmaxf(fmaxf(m, fabsf(v.z)), fabsf(v.w));
    }
    kn_wave_absmax_commit(m, absmax, threadIdx.x & 63);
}

// a column window of a wider block (ld > n_vecs: the half-batch windows of the overlapped forward), 16 bytes per lane: `tpr` threads walk one
// row's n_vecs / 4 quads, 256 / tpr rows per workgroup step -- one 32-bit division per thread, none per element
__global__ __launch_bounds__(256) void absmax_kernel_win4(const float* __restrict__ y, int64_t rows, int64_t ld, int n4, int tpr, float* __restrict__ absmax) {
    const int rpb = 256 / tpr;
    const int tr = (int)threadIdx.x / tpr, tc = (int)threadIdx.x - tr * tpr;
    float m = 0.0f;
    if (tr < rpb) {
        for (int64_t r = (int64_t)blockIdx.x * rpb + tr; r < rows; r += (int64_t)gridDim.x * rpb) {
            const float4* row = reinterpret_cast<const float4*>(y + r * ld);
            for (int c = tc; c < n4; c += tpr) {
                const float4 v = row[c];
                m = fmaxf(fmaxf(m, fabsf(v.x)), fabsf(v.y));
                m = fmaxf(fmaxf(m, fabsf(v.z)), fabsf(v.w));
            }
        }
    }
    kn_wave_absmax_commit(m, absmax, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ y, int64_t rows, int64_t ld, int64_t n_vecs, float* __restrict__ absmax) {
    float m = 0.0f;
    const int64_t total = rows * n_vecs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_vecs;
        m = fmaxf(m, fabsf(y[r * ld + (i - r * n_vecs)]));
    }
    kn_wave_absmax_commit(m, absmax, threadIdx.x & 63);
}

int absmax_pass(const float* y, int64_t rows, int64_t ld, int64_t n_vecs, float* absmax, hipStream_t s) {
    if (rows <= 0 || n_vecs <= 0 || absmax == nullptr) return KN_OK;
    const bool a16 = ((uintptr_t)y) % 16 == 0;
    if (ld == n_vecs && (rows * n_vecs) % 4 == 0 && a16) {
        const int64_t total4 = rows * n_vecs / 4;
        KN_LAUNCH("absmax_kernel_v4", absmax_kernel_v4, dim3((unsigned)std::min<int64_t>((total4 + 255) / 256, 4096)), dim3(256), 0, s, reinterpret_cast<const float4*>(y), total4, absmax);
    } else if (n_vecs % 4 == 0 && ld % 4 == 0 && a16) {
        const int n4 = (int)(n_vecs / 4);
        int tpr = 1;
        while (tpr < n4 && tpr < 256) tpr <<= 1;                  // threads per row: a power of two >= the row's quads (<= 256)
        const int rpb = 256 / tpr;
        KN_LAUNCH("absmax_kernel_win4", absmax_kernel_win4, dim3((unsigned)std::min<int64_t>((rows + rpb - 1) / rpb, 8192)), dim3(256), 0, s, y, rows, ld, n4, tpr, absmax);
    } else {
        KN_LAUNCH("absmax_kernel", absmax_kernel, dim3((unsigned)std::min<int64_t>((rows * n_vecs + 255) / 256, 4096)), dim3(256), 0, s, y, rows, ld, n_vecs, absmax);
    }
    KN_HIP(hipGetLastError());
    return KN_OK;
}

// Planes <-> columns of a narrow batch (kn_planes_to_columns / kn_columns_to_planes; the narrow split route of keynet_amd/sparse.py).
//   planes side   Pl[p][r][b] at pl + p * ps + r * ldp + b      (p < planes, r < rows, b < nv <= 32)
//   columns side  Co[r][(p, b)] at co + r * ldc + p * nv + b
// A transpose of the planes x rows matrix of nv-float elements: one workgroup moves a tile of T planes x T rows through LDS, so that it walks the planes side along
// r (contiguous where ldp == nv) and the columns side along (p, b) (always contiguous).  T = 64 | 32 | 16 for nv <= 2 | 8 | 32: segments of 64 .. 512 floats on either
// side.  In LDS plane pl of the tile starts at pl * sp with sp = T * nv + pad = nv (mod 64): the columns side, whose consecutive lanes step to the next plane every nv
// elements, then reads bank (element index mod 64) -- without the pad every plane would start in the same bank (nv = 1: all 64 lanes in one).  A lane moves 16 bytes
// of global memory per access where its side is aligned (`vec`: the host's rule below) and one float otherwise; LDS is accessed float by float (a 16-byte lane's four
// accesses meet those of three other lanes in a bank: LDS at a quarter of its rate is still ahead of HBM).  No arithmetic: bits pass through.
constexpr int PERMUTE_LDS_FLOATS = 10240;      // >= T * sp for every nv (T = 32, nv = 8: 32 * (256 + 63))

// one side of the tile: GLOBAL -> LDS (LOAD) or LDS -> GLOBAL.  `segs` segments of `len` valid floats; element e of segment s lives in global memory at
// g + s * gseg + (e / run) * grun + e % run (runs of `run` contiguous floats `grun` apart; run == len-or-more: one contiguous segment) and in LDS at
// tile[lds_of(s, e)].  G = 4: 16-byte global accesses on whole quads (the caller guarantees their alignment and that a quad never straddles a run), floats on a ragged tail.
template <bool LOAD, int G, typename LdsOf>
__device__ __forceinline__ void permute_side(float* __restrict__ tile, const float* __restrict__ gsrc, float* __restrict__ gdst, int64_t gseg, int64_t grun, int run, int segs,
                                             int len, LdsOf lds_of) {
    const int per = (len + G - 1) / G;
    for (int i = (int)threadIdx.x; i < segs * per; i += 256) {
        const int sg = i / per;
        const int e = (i - sg * per) * G;
        const int k = e / run;
        const int64_t at = (int64_t)sg * gseg + (int64_t)k * grun + (e - k * run);
        if (G == 4 && e + 4 <= len) {
            if (LOAD) {
                const float4 v = *reinterpret_cast<const float4*>(gsrc + at);
                tile[lds_of(sg, e)] = v.x;
                tile[lds_of(sg, e + 1)] = v.y;
                tile[lds_of(sg, e + 2)] = v.z;
                tile[lds_of(sg, e + 3)] = v.w;
            } else {
                float4 v;
                v.x = tile[lds_of(sg, e)];
                v.y = tile[lds_of(sg, e + 1)];
                v.z = tile[lds_of(sg, e + 2)];
                v.w = tile[lds_of(sg, e + 3)];
                *reinterpret_cast<float4*>(gdst + at) = v;
            }
        } else {
            for (int j = 0; j < G && e + j < len; j++) {
                const int kj = (e + j) / run;
                const int64_t aj = (int64_t)sg * gseg + (int64_t)kj * grun + (e + j - kj * run);
                if (LOAD) tile[lds_of(sg, e + j)] = gsrc[aj];
                else gdst[aj] = tile[lds_of(sg, e + j)];
            }
        }
    }
}

template <bool TO_COLUMNS, int GP, int GC>
__global__ __launch_bounds__(256) void planes_columns_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t planes, int64_t rows, int nv, int64_t ps,
                                                             int64_t ldp, int64_t ldc, int T, int sp) {
    __shared__ float tile[PERMUTE_LDS_FLOATS];
    const int64_t r0 = (int64_t)blockIdx.x * T, p0 = (int64_t)blockIdx.y * T;
    const int tr = (rows - r0 < T) ? (int)(rows - r0) : T, tp = (planes - p0 < T) ? (int)(planes - p0) : T;
    const int64_t pl_at = p0 * ps + r0 * ldp;            // the tile's corner on either side (64 bits: a plane may begin beyond 2^31 elements)
    const int64_t co_at = r0 * ldc + p0 * nv;
    // planes side: segment = a plane of the tile, tr rows of nv floats, ldp apart (one contiguous run where ldp == nv); LDS: pl * sp + e
    auto lds_pl = [sp](int pl, int e) { return pl * sp + e; };
    // columns side: segment = a row of the tile, tp * nv contiguous floats; LDS: element o = (pl, b) of row rl at pl * sp + rl * nv + b
    auto lds_co = [sp, nv](int rl, int o) { const int pl = o / nv; return pl * sp + rl * nv + (o - pl * nv); };
    const int prun = (ldp == nv) ? tr * nv : nv;
    if (TO_COLUMNS) {
        permute_side<true, GP>(tile, src + pl_at, nullptr, ps, ldp, prun, tp, tr * nv, lds_pl);
        __syncthreads();
        permute_side<false, GC>(tile, nullptr, dst + co_at, ldc, 0, tp * nv, tr, tp * nv, lds_co);
    } else {
        permute_side<true, GC>(tile, src + co_at, nullptr, ldc, 0, tp * nv, tr, tp * nv, lds_co);
        __syncthreads();
        permute_side<false, GP>(tile, nullptr, dst + pl_at, ps, ldp, prun, tp, tr * nv, lds_pl);
    }
}

template <bool TO_COLUMNS>
static int planes_columns(const float* src, float* dst, const float* pl, const float* co, int64_t planes, int64_t rows, int64_t nv, int64_t ps, int64_t ldp, int64_t ldc,
                          hipStream_t s) {
    if (planes <= 0 || rows <= 0 || nv <= 0) return KN_OK;
    const int T = nv <= 2 ? 64 : (nv <= 8 ? 32 : 16);
    const int sp = T * (int)nv + (int)((((nv - T * nv) % 64) + 64) % 64);
    if ((int64_t)T * sp > PERMUTE_LDS_FLOATS) return fail(KN_ERR_UNSUPPORTED, "planes <-> columns: the tile does not fit the LDS array");
    // 16 bytes per lane on a side: its base and every stride a multiple of four floats (tile corners are: T % 4 == 0), and quads that stay inside a contiguous run --
    // the planes side where rows follow each other without a gap (ldp == nv) or a row is whole quads; the columns side always (a ragged end moves float by float)
    const bool vp = ((uintptr_t)pl) % 16 == 0 && (ps % 4 == 0 || planes == 1) && (ldp == nv || (nv % 4 == 0 && ldp % 4 == 0));
    const bool vc = ((uintptr_t)co) % 16 == 0 && ldc % 4 == 0;
    const int64_t ymax = 65535;                          // planes beyond 65 535 tiles: further launches
    for (int64_t pt = 0; pt * T < planes; pt += ymax) {
        const int64_t np = std::min<int64_t>(planes - pt * T, ymax * T);
        const dim3 grid((unsigned)((rows + T - 1) / T), (unsigned)((np + T - 1) / T));
        const float* sp_ = src + (TO_COLUMNS ? pt * T * ps : pt * T * nv);
        float* dp_ = dst + (TO_COLUMNS ? pt * T * nv : pt * T * ps);
        if (vp && vc) hipLaunchKernelGGL((planes_columns_kernel<TO_COLUMNS, 4, 4>), grid, dim3(256), 0, s, sp_, dp_, np, rows, (int)nv, ps, ldp, ldc, T, sp);
        else if (vp) hipLaunchKernelGGL((planes_columns_kernel<TO_COLUMNS, 4, 1>), grid, dim3(256), 0, s, sp_, dp_, np, rows, (int)nv, ps, ldp, ldc, T, sp);
        else if (vc) hipLaunchKernelGGL((planes_columns_kernel<TO_COLUMNS, 1, 4>), grid, dim3(256), 0, s, sp_, dp_, np, rows, (int)nv, ps, ldp, ldc, T, sp);
        else hipLaunchKernelGGL((planes_columns_kernel<TO_COLUMNS, 1, 1>), grid, dim3(256), 0, s, sp_, dp_, np, rows, (int)nv, ps, ldp, ldc, T, sp);
    }
    KN_HIP(hipGetLastError());
    return KN_OK;
}

int planes_to_columns(const float* in, int64_t plane_stride, int64_t ld, int64_t planes, int64_t rows, int64_t n_vecs, float* out, int64_t ld_out, hipStream_t s) {
    return planes_columns<true>(in, out, in, out, planes, rows, n_vecs, plane_stride, ld, ld_out, s);
}

int columns_to_planes(const float* in, int64_t ld_in, int64_t planes, int64_t rows, int64_t n_vecs, float* out, int64_t plane_stride, int64_t ld, hipStream_t s) {
    return planes_columns<false>(in, out, out, in, planes, rows, n_vecs, plane_stride, ld, ld_in, s);
}

int linear_to_affine(const float* y, int64_t ldy, int64_t n, int64_t d, float* out, float* maxdev, hipStream_t s) {
    if (n <= 0) return KN_OK;
    if (d > 0) {
        dim3 grid((unsigned)((n + 63) / 64), (unsigned)((d + 63) / 64));
        hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, s, y, d, n, ldy, out, d);
    }
    if (maxdev) hipLaunchKernelGGL(lastrow_dev_kernel, dim3(1), dim3(256), 0, s, y + d * ldy, n, maxdev);
    KN_HIP(hipGetLastError());
    return KN_OK;
}

}  // namespace kn
