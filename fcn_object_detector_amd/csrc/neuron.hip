// One-bottom activations without a learned parameter, on NHWC views (Caffe ELULayer, ClipLayer - and with it the MobileNet forks' ReLU6 -,
// AbsValLayer, BNLLLayer, SwishLayer).  a = alpha (ELU), beta (Swish) or lo (Clip); b = hi (Clip):
//   ELU     y = x > 0 ? x : a * expm1(x)                             dx (+)= dy * (y > 0 ? 1 : y + a)               reads y
//   Clip    y = min(max(x, a), b)                                    dx (+)= dy * [a < y < b]                       reads y
//   AbsVal  y = |x|                                                  dx (+)= dy * sign(x), sign(0) = 0              reads x
//   BNLL    y = x > 0 ? x + log1p(exp(-x)) : log1p(exp(x))           dx (+)= dy * (-expm1(-y))                      reads y
//   Swish   y = x * s, s = 1 / (1 + exp(-a x))                       dx (+)= dy * (a y + s (1 - a y))               reads x
//
// Work layout, that of act.hip: a lane owns ONE 16-byte channel group of a pixel (4 floats / 8 halves), the `tg` lanes next to each
// other own consecutive groups of the same pixel, the 256 / tg rows of a workgroup own consecutive pixels; the workgroups along the
// pixels are capped (NEURON_MAX_GROUPS in all) and stride over the rest.  A C that is no multiple of the group stores its last group in
// pieces (unrolled and predicated): channels outside coffset .. coffset + C - 1 are never written; loads of whole groups stay inside the
// pixel because strides and offsets are multiples of the group.  No LDS, no atomics, one writer per element: the same call gives the
// same bits.  The mode is a template parameter: no per-element branch on it survives.
#include "common.h"

#include <hip/hip_fp16.h>

namespace fcn {
namespace {

constexpr int NEURON_THREADS = 256;
constexpr int NEURON_MAX_GROUPS = 2048;      // workgroups of a launch: 8 per CU of a 256-CU part, every wave slot taken

struct NeuronTile {
    int tg;      // channel groups side by side in a workgroup (power of two, <= 16)
    int gx;      // workgroups along the channel groups
    int gy;      // workgroups along the pixels (grid-stride over the rest)
};

inline NeuronTile neuron_tile(int pixels, int C, int epg) {
    NeuronTile t;
    const int cg = (C + epg - 1) / epg;
    t.tg = 1;
    while (t.tg < cg && t.tg < 16) t.tg <<= 1;
    const int rows = NEURON_THREADS / t.tg;
    t.gx = (cg + t.tg - 1) / t.tg;
    const long long gy = ((long long)pixels + rows - 1) / rows;
    long long cap = NEURON_MAX_GROUPS / t.gx;
    if (cap < 1) cap = 1;
    t.gy = (int)(gy < cap ? gy : cap);
    return t;
}

template <int MODE>
__device__ inline float neuron_fwd(float v, float a, float b) {
    if (MODE == FCN_NEURON_ELU) return v > 0.f ? v : a * expm1f(v);
    if (MODE == FCN_NEURON_CLIP) return fminf(fmaxf(v, a), b);
    if (MODE == FCN_NEURON_ABSVAL) return fabsf(v);
    if (MODE == FCN_NEURON_BNLL) return v > 0.f ? v + log1pf(expf(-v)) : log1pf(expf(v));
    return v / (1.f + expf(-a * v));
}

// dy -> dx; r is the layer's output y (ELU, Clip, BNLL) or its input x (AbsVal, Swish)
template <int MODE>
__device__ inline float neuron_bwd(float d, float r, float a, float b) {
    if (MODE == FCN_NEURON_ELU) return r > 0.f ? d : d * (r + a);
    if (MODE == FCN_NEURON_CLIP) return (r > a && r < b) ? d : 0.f;
    if (MODE == FCN_NEURON_ABSVAL) return r > 0.f ? d : (r < 0.f ? -d : 0.f);
    if (MODE == FCN_NEURON_BNLL) return d * -expm1f(-r);
    const float s = 1.f / (1.f + expf(-a * r)), ay = a * (r * s);
    return d * (ay + s * (1.f - ay));
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (gx, gy).  y may be x: a lane reads its group of a pixel before it writes it, and no other lane touches that group.
template <int MODE>
__global__ __launch_bounds__(NEURON_THREADS) void neuron_fwd_f32_kernel(const float* x, float* y, float* __restrict__ keep, int pixels, int C, int xcs,
                                                                         int xco, int ycs, int yco, int kcs, float a, float b, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = NEURON_THREADS / tg;
    const int c0 = 4 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(4, C - c0);
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        const float4 v4 = *reinterpret_cast<const float4*>(x + (size_t)p * xcs + xco + c0);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = neuron_fwd<MODE>(v[j], a, b);
        float* yp = y + (size_t)p * ycs + yco + c0;
        float* kp = keep ? keep + (size_t)p * kcs + c0 : nullptr;
        if (nv == 4) {
            if (kp) *reinterpret_cast<float4*>(kp) = v4;
            *reinterpret_cast<float4*>(yp) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) {
                    if (kp) kp[j] = v[j];
                    yp[j] = o[j];
                }
        }
    }
}

// halves in, halves out, float32 arithmetic, one rounding to half; a lane owns 8 channels.  Three store forms: a whole group as 16
// bytes; of a last, partial group the whole pairs as 32-bit words and an odd last channel as one half - the pad half that shares its
// word is not written.
template <int MODE>
__global__ __launch_bounds__(NEURON_THREADS) void neuron_fwd_f16_kernel(const __half* x, __half* y, int pixels, int C, int xcs, int xco, int ycs, int yco,
                                                                         float a, float b, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = NEURON_THREADS / tg;
    const int c0 = 8 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(8, C - c0);
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        union { uint4 u; __half h[8]; } in;
        union { uint4 u; unsigned w[4]; __half h[8]; } out;
        in.u = *reinterpret_cast<const uint4*>(x + (size_t)p * xcs + xco + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) out.h[j] = __float2half_rn(neuron_fwd<MODE>(__half2float(in.h[j]), a, b));
        __half* yp = y + (size_t)p * ycs + yco + c0;
        if (nv == 8) {
            *reinterpret_cast<uint4*>(yp) = out.u;
        } else {      // (unrolled and predicated: an index that is no constant would move the unions out of the registers)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (2 * k + 1 < nv) reinterpret_cast<unsigned*>(yp)[k] = out.w[k];
                else if (2 * k < nv) yp[2 * k] = out.h[2 * k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- data gradient
// grid (gx, gy).  dx may be dy (accumulate 0): the same one-lane-one-group argument as in the forward.
template <int MODE>
__global__ __launch_bounds__(NEURON_THREADS) void neuron_bwd_kernel(const float* dy, const float* __restrict__ ref, float* dx, int pixels, int C, int dcs,
                                                                     int dco, int rcs, int rco, int xcs, int xco, float a, float b, int accumulate,
                                                                     int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = NEURON_THREADS / tg;
    const int c0 = 4 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(4, C - c0);
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        const float4 d4 = *reinterpret_cast<const float4*>(dy + (size_t)p * dcs + dco + c0);
        const float4 r4 = *reinterpret_cast<const float4*>(ref + (size_t)p * rcs + rco + c0);
        const float d[4] = {d4.x, d4.y, d4.z, d4.w}, r[4] = {r4.x, r4.y, r4.z, r4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = neuron_bwd<MODE>(d[j], r[j], a, b);
        float* xp = dx + (size_t)p * xcs + xco + c0;
        if (nv == 4) {
            if (accumulate) {
                const float4 old = *reinterpret_cast<const float4*>(xp);
                o[0] += old.x; o[1] += old.y; o[2] += old.z; o[3] += old.w;
            }
            *reinterpret_cast<float4*>(xp) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) xp[j] = accumulate ? xp[j] + o[j] : o[j];
        }
    }
}

inline bool neuron_view_in(int C, int cstride, int coffset) { return coffset >= 0 && cstride >= coffset + C; }
inline bool neuron_view_ok(int cstride, int coffset, int epg) { return cstride % epg == 0 && coffset % epg == 0; }
inline bool neuron_mode_ok(int mode) { return mode >= FCN_NEURON_ELU && mode <= FCN_NEURON_SWISH; }
// (written so that a NaN is refused as well)
inline bool neuron_params_ok(int mode, float a, float b) {
    if (mode == FCN_NEURON_ELU) return a >= 0.f;
    if (mode == FCN_NEURON_CLIP) return a < b;
    return true;
}

#define NEURON_LAUNCH(KERNEL, mode, grid, block, st, ...)                                                                     \
    switch (mode) {                                                                                                           \
        case FCN_NEURON_ELU: hipLaunchKernelGGL(KERNEL<FCN_NEURON_ELU>, grid, block, 0, st, __VA_ARGS__); break;            \
        case FCN_NEURON_CLIP: hipLaunchKernelGGL(KERNEL<FCN_NEURON_CLIP>, grid, block, 0, st, __VA_ARGS__); break;          \
        case FCN_NEURON_ABSVAL: hipLaunchKernelGGL(KERNEL<FCN_NEURON_ABSVAL>, grid, block, 0, st, __VA_ARGS__); break;      \
        case FCN_NEURON_BNLL: hipLaunchKernelGGL(KERNEL<FCN_NEURON_BNLL>, grid, block, 0, st, __VA_ARGS__); break;          \
        default: hipLaunchKernelGGL(KERNEL<FCN_NEURON_SWISH>, grid, block, 0, st, __VA_ARGS__); break;                      \
    }

}  // namespace
}  // namespace fcn

using namespace fcn;

int fcn_neuron_fwd_f32(const float* x, float* y, float* keep, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                       int keep_cstride, int mode, float a, float b, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "neuron_fwd: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "neuron_fwd: non-positive extent");
    FCN_REQUIRE(neuron_mode_ok(mode), FCN_E_ARG, "neuron_fwd: unknown mode %d", mode);
    FCN_REQUIRE(neuron_params_ok(mode, a, b), FCN_E_ARG, "neuron_fwd: ELU needs alpha >= 0, Clip needs lo < hi (got %g, %g)", (double)a, (double)b);
    FCN_REQUIRE(neuron_view_in(C, x_cstride, x_coffset) && neuron_view_in(C, y_cstride, y_coffset) && (!keep || keep_cstride >= C), FCN_E_ARG,
                "neuron_fwd: channel slice out of range");
    FCN_REQUIRE(neuron_view_ok(x_cstride, x_coffset, 4) && neuron_view_ok(y_cstride, y_coffset, 4) && (!keep || keep_cstride % 4 == 0), FCN_E_ALIGN,
                "neuron_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)keep) & 15) == 0, FCN_E_ALIGN, "neuron_fwd: x, y and keep must be 16-byte aligned");
    const NeuronTile t = neuron_tile(pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(NEURON_THREADS);
    NEURON_LAUNCH(neuron_fwd_f32_kernel, mode, grid, block, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset,
                  keep_cstride, a, b, t.tg);
    FCN_LAUNCH_CHECK("neuron_fwd_f32_kernel");
    return 0;
}

int fcn_neuron_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset, int mode, float a,
                       float b, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "neuron_fwd_f16: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "neuron_fwd_f16: non-positive extent");
    FCN_REQUIRE(neuron_mode_ok(mode), FCN_E_ARG, "neuron_fwd_f16: unknown mode %d", mode);
    FCN_REQUIRE(neuron_params_ok(mode, a, b), FCN_E_ARG, "neuron_fwd_f16: ELU needs alpha >= 0, Clip needs lo < hi (got %g, %g)", (double)a,
                (double)b);
    FCN_REQUIRE(neuron_view_in(C, x_cstride, x_coffset) && neuron_view_in(C, y_cstride, y_coffset), FCN_E_ARG,
                "neuron_fwd_f16: channel slice out of range");
    FCN_REQUIRE(neuron_view_ok(x_cstride, x_coffset, 8) && neuron_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "neuron_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, FCN_E_ALIGN, "neuron_fwd_f16: x and y must be 16-byte aligned");
    const NeuronTile t = neuron_tile(pixels, C, 8);
    const dim3 grid(t.gx, t.gy), block(NEURON_THREADS);
    const __half* xh = static_cast<const __half*>(x);
    __half* yh = static_cast<__half*>(y);
    NEURON_LAUNCH(neuron_fwd_f16_kernel, mode, grid, block, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset, a, b, t.tg);
    FCN_LAUNCH_CHECK("neuron_fwd_f16_kernel");
    return 0;
}

int fcn_neuron_bwd_f32(const float* dy, const float* ref, float* dx, int pixels, int C, int dy_cstride, int dy_coffset, int ref_cstride,
                       int ref_coffset, int dx_cstride, int dx_coffset, int mode, float a, float b, int accumulate, fcn_stream_t s) {
    FCN_REQUIRE(dy && ref && dx, FCN_E_ARG, "neuron_bwd: null dy / ref / dx");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "neuron_bwd: non-positive extent");
    FCN_REQUIRE(neuron_mode_ok(mode), FCN_E_ARG, "neuron_bwd: unknown mode %d", mode);
    FCN_REQUIRE(neuron_params_ok(mode, a, b), FCN_E_ARG, "neuron_bwd: ELU needs alpha >= 0, Clip needs lo < hi (got %g, %g)", (double)a, (double)b);
    FCN_REQUIRE(neuron_view_in(C, dy_cstride, dy_coffset) && neuron_view_in(C, dx_cstride, dx_coffset) && neuron_view_in(C, ref_cstride, ref_coffset),
                FCN_E_ARG, "neuron_bwd: channel slice out of range");
    FCN_REQUIRE(neuron_view_ok(dy_cstride, dy_coffset, 4) && neuron_view_ok(dx_cstride, dx_coffset, 4) && neuron_view_ok(ref_cstride, ref_coffset, 4),
                FCN_E_ALIGN, "neuron_bwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)dy | (uintptr_t)dx | (uintptr_t)ref) & 15) == 0, FCN_E_ALIGN, "neuron_bwd: dy, ref and dx must be 16-byte aligned");
    const NeuronTile t = neuron_tile(pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(NEURON_THREADS);
    const int acc = accumulate ? 1 : 0;
    NEURON_LAUNCH(neuron_bwd_kernel, mode, grid, block, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset, ref_cstride, ref_coffset,
                  dx_cstride, dx_coffset, a, b, acc, t.tg);
    FCN_LAUNCH_CHECK("neuron_bwd_kernel");
    return 0;
}
