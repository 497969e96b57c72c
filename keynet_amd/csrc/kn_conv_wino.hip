// kn_conv_wino.hip -- KN_MODIFIER_WINO: a keyed 3 x 3 convolution in its 1-D Winograd F(2,3) form along the image rows (kn_wino.h has the identity and the host derivation).
// The product itself is the derived conv-taps operator on convtaps_mfma_kernel, unchanged (kn_conv.hip); this file holds the two transforms around it -- memory-bound
// element-wise kernels, 16 bytes per lane, additions only -- their launcher, and the workspace pool of the V and M blocks.
//
//   wino_in_kernel    V[ci][4 p + j][:]  from the activation rows d0 .. d3 of input pair p:   V0 = d0 - d2,  V1 = d1 + d2,  V2 = d2 - d1,  V3 = d1 - d3   (a row outside the image is zero)
//   wino_out_kernel   Y[co][oA][:] = M0 + M1 + M2 (+ lastcol * x_last),  Y[co][oB][:] = M1 - M2 - M3 (+ lastcol * x_last)   of output pair P = (oA, oB), M = M[co][4 P + j][:];
//                     ReLU, nontemporal stores, max |Y| into the screen's slot like kn_store_tile
// The order of the additions is the one written here and the build has -ffp-contract=off: a column's bits do not depend on the batch width.  Every row offset is formed in 64 bits.
#include "kn_internal.h"
#include <map>
#include <utility>

namespace kn {

typedef float wf32x4 __attribute__((ext_vector_type(4)));

struct WinoInArgs {
    const float* X;
    float* V;
    const int32_t* in_d;      // [n_pairs][4]
    int64_t ldx;
    int32_t n_pairs, HiWi, nv4, lanes_log2;      // nv4: 16-byte segments of a row (n_vecs / 4); a pair's row segments are walked by 1 << lanes_log2 (32 | 64) lanes
};

struct WinoOutArgs {
    const float* M;
    float* Y;
    const int32_t* out_pair;      // [n_pairs][2]
    const float* lastcol;         // [Cout * HoWo + 1] or null
    const float* xlast;           // the homogeneous row of X
    int64_t ldy;
    int32_t n_pairs, HoWo, nv4, lanes_log2, relu;
    float* absmax;
};

// grid (pair blocks, Cin), 256 threads: a wavefront owns one pair (n_vecs a multiple of 256) or two (128, 384, ...), a lane 16 bytes of each of the pair's rows
__global__ __launch_bounds__(256) void wino_in_kernel(WinoInArgs p) {
    const int lanes = 1 << p.lanes_log2;
    const int pr = (int)blockIdx.x * (256 >> p.lanes_log2) + ((int)threadIdx.x >> p.lanes_log2);
    if (pr >= p.n_pairs) return;
    const int ci = (int)blockIdx.y;
    const int4 d = *reinterpret_cast<const int4*>(p.in_d + 4 * (int64_t)pr);
    const float* xc = p.X + (int64_t)ci * p.HiWi * p.ldx;
    float* v = p.V + ((int64_t)ci * p.n_pairs + pr) * 16 * p.nv4;      // four rows of 4 * nv4 floats
    const wf32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c4 = (int)threadIdx.x & (lanes - 1); c4 < p.nv4; c4 += lanes) {
        const wf32x4 d0 = d.x >= 0 ? *reinterpret_cast<const wf32x4*>(xc + (int64_t)d.x * p.ldx + 4 * c4) : zero;
        const wf32x4 d1 = d.y >= 0 ? *reinterpret_cast<const wf32x4*>(xc + (int64_t)d.y * p.ldx + 4 * c4) : zero;
        const wf32x4 d2 = d.z >= 0 ? *reinterpret_cast<const wf32x4*>(xc + (int64_t)d.z * p.ldx + 4 * c4) : zero;
        const wf32x4 d3 = d.w >= 0 ? *reinterpret_cast<const wf32x4*>(xc + (int64_t)d.w * p.ldx + 4 * c4) : zero;
        wf32x4* o = reinterpret_cast<wf32x4*>(v + 4 * c4);
        o[0] = d0 - d2;
        o[p.nv4] = d1 + d2;
        o[2 * p.nv4] = d2 - d1;
        o[3 * p.nv4] = d1 - d3;
    }
}

// grid (pair blocks, Cout), 256 threads, the same shape.  No lane leaves early: the wavefront's max |y| is committed by lane 63.
__global__ __launch_bounds__(256) void wino_out_kernel(WinoOutArgs p) {
    const int lanes = 1 << p.lanes_log2;
    const int pr0 = (int)blockIdx.x * (256 >> p.lanes_log2) + ((int)threadIdx.x >> p.lanes_log2);
    const bool valid = pr0 < p.n_pairs;
    const int pr = valid ? pr0 : 0;
    const int co = (int)blockIdx.y;
    const int2 o = *reinterpret_cast<const int2*>(p.out_pair + 2 * (int64_t)pr);
    const float* m = p.M + ((int64_t)co * p.n_pairs + pr) * 16 * p.nv4;
    float* ya = p.Y + ((int64_t)co * p.HoWo + o.x) * p.ldy;
    float* yb = p.Y + ((int64_t)co * p.HoWo + o.y) * p.ldy;
    const float la = p.lastcol ? p.lastcol[(int64_t)co * p.HoWo + o.x] : 0.0f;
    const float lb = p.lastcol ? p.lastcol[(int64_t)co * p.HoWo + o.y] : 0.0f;
    const float lo = p.relu ? 0.0f : -__builtin_inff();
    float am = 0.0f;
    for (int c4 = (int)threadIdx.x & (lanes - 1); valid && c4 < p.nv4; c4 += lanes) {
        const wf32x4* mi = reinterpret_cast<const wf32x4*>(m + 4 * c4);
        const wf32x4 m0 = mi[0], m1 = mi[p.nv4], m2 = mi[2 * p.nv4], m3 = mi[3 * p.nv4];
        wf32x4 a = m0 + m1;
        a = a + m2;
        wf32x4 b = m1 - m2;
        b = b - m3;
        if (la != 0.0f || lb != 0.0f) {                       // the last column: one product, one add, as the tile kernels do it (a zero entry contributes nothing)
            const wf32x4 xl = *reinterpret_cast<const wf32x4*>(p.xlast + 4 * c4);
            if (la != 0.0f) {
                const wf32x4 t = xl * la;
                a = a + t;
            }
            if (lb != 0.0f) {
                const wf32x4 t = xl * lb;
                b = b + t;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            a[k] = (a[k] < lo) ? lo : a[k];
            b[k] = (b[k] < lo) ? lo : b[k];
            am = fmaxf(am, fmaxf(fabsf(a[k]), fabsf(b[k])));      // NaN operands are ignored, +-Inf counts
        }
        __builtin_nontemporal_store(a, reinterpret_cast<wf32x4*>(ya + 4 * c4));
        __builtin_nontemporal_store(b, reinterpret_cast<wf32x4*>(yb + 4 * c4));
    }
    if (p.absmax) kn_wave_absmax_commit(am, p.absmax, (int)threadIdx.x & 63);
}

int64_t wino_workspace_floats(const kn_operator* h, int64_t n_vecs) {
    const ConvTapsDev& A = h->ct;
    return 2 * (A.Cin * A.Hin * A.Win + A.Cout * A.Hout * A.Wout) * n_vecs;
}

// ONE block per (device, stream), shared by every handle (launches on one stream are ordered; the overlapped forward calls one handle on two streams at once, so a
// block per handle would race and a block per call would cost a layer's V and M on every launch).  It grows to the largest request; an outgrown block is retired behind
// an event recorded on its stream and freed by a later growing call once the event has completed (the dense workspace's scheme, kn_api.hip).  Blocks live as long as
// the library.  A growing call is not capturable: kn_reserve_workspace_flags sizes the pool ahead of a HIP-graph capture.
namespace {
struct WinoPool {
    float* ptr = nullptr;
    int64_t floats = 0;
};
struct WinoRetired {
    float* ptr = nullptr;
    hipEvent_t done = nullptr;
};
std::mutex g_wino_mu;
std::map<std::pair<int, hipStream_t>, WinoPool> g_wino_pool;
std::vector<WinoRetired> g_wino_retired;
}  // namespace

int wino_workspace(int device, hipStream_t s, int64_t floats, float** out) {
    std::lock_guard<std::mutex> g(g_wino_mu);
    WinoPool& w = g_wino_pool[std::make_pair(device, s)];
    if (w.floats < floats) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
        KN_REQUIRE(cap == hipStreamCaptureStatusNone, KN_ERR_HIP,
                   "Winograd workspace must grow (during a HIP-graph capture: run one eager kn_spmm on the capture stream first, or call kn_reserve_workspace)");
        for (size_t k = 0; k < g_wino_retired.size();) {
            WinoRetired& r = g_wino_retired[k];
            if (r.done == nullptr || hipEventQuery(r.done) == hipSuccess) {
                if (r.done) (void)hipEventDestroy(r.done);
                (void)hipFree(r.ptr);
                g_wino_retired.erase(g_wino_retired.begin() + (long)k);
            } else {
                k++;
            }
        }
        (void)hipGetLastError();                            // hipEventQuery's hipErrorNotReady is not an error of this call
        if (w.ptr) {
            WinoRetired r;
            r.ptr = w.ptr;                                  // launches already queued on `s` may still use it
            if (hipEventCreateWithFlags(&r.done, hipEventDisableTiming) != hipSuccess || hipEventRecord(r.done, s) != hipSuccess) {
                if (r.done) (void)hipEventDestroy(r.done);
                r.done = nullptr;
                (void)hipStreamSynchronize(s);
            }
            g_wino_retired.push_back(r);
        }
        w.ptr = nullptr;
        w.floats = 0;
        hipError_t e = hipMalloc((void**)&w.ptr, sizeof(float) * (size_t)floats);
        if (e != hipSuccess) {
            w.ptr = nullptr;
            return fail(e == hipErrorOutOfMemory ? KN_ERR_NOMEM : KN_ERR_HIP, std::string("Winograd workspace hipMalloc: ") + hipGetErrorString(e));
        }
        w.floats = floats;
    }
    *out = w.ptr;
    return KN_OK;
}

int wino_spmm(const kn_operator* h, const float* x, int64_t ldx, int64_t n_vecs, float* y, int64_t ldy, uint32_t flags, hipStream_t s, float* absmax) {
    const ConvTapsDev& A = h->ct;
    const ConvTapsDev& S = h->wino_sub->ct;
    const int64_t HiWi = A.Hin * A.Win, HoWo = A.Hout * A.Wout;
    KN_REQUIRE(A.Cin <= 65535 && A.Cout <= 65535, KN_ERR_UNSUPPORTED, "KN_MODIFIER_WINO: more than 65 535 channels");
    float* ws = reinterpret_cast<float*>((uintptr_t)1 << 20);      // kn_spmm_plan: an aligned stand-in, nothing is launched or allocated
    if (plan_sink() == nullptr) {
        if (int rc = wino_workspace(h->device, s, wino_workspace_floats(h, n_vecs), &ws)) return rc;
    }
    float* V = ws;
    float* M = ws + 2 * A.Cin * HiWi * n_vecs;
    const int nv4 = (int)(n_vecs / 4), lanes_log2 = nv4 % 64 == 0 ? 6 : 5, ppb = 256 >> lanes_log2;
    const int relu = (flags & KN_FLAG_RELU) ? 1 : 0;
    WinoInArgs in = {x, V, h->wino_in, ldx, (int32_t)(HiWi / 2), (int32_t)HiWi, nv4, lanes_log2};
    KN_LAUNCH("wino_in_kernel", wino_in_kernel, dim3((unsigned)((HiWi / 2 + ppb - 1) / ppb), (unsigned)A.Cin), dim3(256), 0, s, in);
    if (int rc = convtaps_spmm(S, V, n_vecs, n_vecs, M, n_vecs, 0, s)) return rc;
    WinoOutArgs out = {M, y, h->wino_out, A.has_last ? A.lastcol : nullptr, x + A.Cin * HiWi * ldx, ldy, (int32_t)(HoWo / 2), (int32_t)HoWo, nv4, lanes_log2, relu, absmax};
    KN_LAUNCH("wino_out_kernel", wino_out_kernel, dim3((unsigned)((HoWo / 2 + ppb - 1) / ppb), (unsigned)A.Cout), dim3(256), 0, s, out);
    if (int rc = convtaps_lastrow(A, x, ldx, n_vecs, y, ldy, relu, absmax, s)) return rc;
    KN_HIP(hipGetLastError());
    return KN_OK;
}

}  // namespace kn
