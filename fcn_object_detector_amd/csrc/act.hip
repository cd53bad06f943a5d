// One-bottom activations with (PReLU, Bias) or without (TanH) a learned per-channel parameter, on NHWC views (Caffe PReLULayer,
// BiasLayer over the channel axis, TanHLayer):
//   PReLU  y = x > 0 ? x : a[c] * x      dx (+)= x > 0 ? dy : a[c] * dy      da[c] = sum_p dy * x * [x <= 0]
//   TanH   y = tanh(x)                   dx (+)= dy * (1 - y * y)
//   Bias   y = x + b[c]                  dx (+)= dy                          db[c] = sum_p dy
//
// Work layout, that of batchnorm.hip: a lane owns ONE 16-byte channel group of a pixel (4 floats / 8 halves), the `tg` lanes next to
// each other own consecutive groups of the same pixel (tg = 16 where C allows: 256 contiguous bytes per pixel row), the 256 / tg rows
// of a workgroup own consecutive pixels.  The parameters of the lane's group are read once, in its prologue - never per pixel.  A C
// that is no multiple of the group stores its last group element by element (unrolled and predicated): channels outside coffset ..
// coffset + C - 1 are never written; loads of whole groups stay inside the pixel because strides and offsets are multiples of the group.
//
// The parameter gradient uses no atomics: a workgroup folds its slab of pixels (rows ascending), the slabs' partial sums go to the
// workspace, and a second launch folds them per channel in a fixed order - lane l of the channel's wave folds slabs l, l + 64, ...
// ascending, then the lanes fold by halves (32, 16, .. 1).  A shared parameter (Caffe's channel_shared) is the fold of those
// per-channel sums over the channels, ascending, by one thread of a third launch.  The same call gives the same bits.
#include "common.h"

#include <hip/hip_fp16.h>

namespace fcn {
namespace {

constexpr int ACT_THREADS = 256;
constexpr int ACT_MAX_SLABS = 1024;

struct ActTile {
    int tg;        // channel groups side by side in a workgroup (power of two, <= 16)
    int rows;      // pixels side by side: ACT_THREADS / tg
    int gx;        // workgroups along the channel groups
    int gy;        // workgroups along the pixels (the streaming launches: grid-stride over the rest)
    int slabs;     // slabs of pixels (the parameter gradient) ...
    int slab_px;   // ... of this many pixels each (the last one shorter); never below `rows`
};

inline ActTile act_tile(int pixels, int C, int epg) {
    ActTile t;
    const int cg = (C + epg - 1) / epg;
    t.tg = 1;
    while (t.tg < cg && t.tg < 16) t.tg <<= 1;
    t.rows = ACT_THREADS / t.tg;
    t.gx = (cg + t.tg - 1) / t.tg;
    long long gy = ((long long)pixels + t.rows - 1) / t.rows;
    long long cap = 16384 / t.gx;
    if (cap < 1) cap = 1;
    t.gy = (int)(gy < cap ? gy : cap);
    int want = 2048 / t.gx;
    if (want < 1) want = 1;
    if (want > ACT_MAX_SLABS) want = ACT_MAX_SLABS;
    t.slab_px = (pixels + want - 1) / want;
    if (t.slab_px < t.rows) t.slab_px = t.rows;      // every row of a workgroup gets a pixel
    t.slabs = (pixels + t.slab_px - 1) / t.slab_px;
    return t;
}

template <int MODE>
__device__ inline float act_fwd(float v, float a) {
    if (MODE == FCN_ACT_PRELU) return v > 0.f ? v : a * v;
    if (MODE == FCN_ACT_TANH) return tanhf(v);
    return v + a;
}

// dy -> dx; r is the layer's input x (PReLU) or its output y (TanH)
template <int MODE>
__device__ inline float act_bwd(float d, float r, float a) {
    if (MODE == FCN_ACT_PRELU) return r > 0.f ? d : a * d;
    if (MODE == FCN_ACT_TANH) return d * (1.f - r * r);
    return d;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (gx, gy).  y may be x: a lane reads its group of a pixel before it writes it, and no other lane touches that group.
template <int MODE>
__global__ __launch_bounds__(ACT_THREADS) void act_fwd_f32_kernel(const float* x, float* y, float* __restrict__ keep, int pixels, int C, int xcs, int xco,
                                                                   int ycs, int yco, int kcs, const float* __restrict__ param, int shared, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = ACT_THREADS / tg;
    const int c0 = 4 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(4, C - c0);
    float pa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[j] = (MODE != FCN_ACT_TANH && j < nv) ? param[shared ? 0 : c0 + j] : 0.f;
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        const float4 v4 = *reinterpret_cast<const float4*>(x + (size_t)p * xcs + xco + c0);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = act_fwd<MODE>(v[j], pa[j]);
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

// halves in, halves out, float32 parameters and arithmetic, one rounding to half; a lane owns 8 channels
template <int MODE>
__global__ __launch_bounds__(ACT_THREADS) void act_fwd_f16_kernel(const __half* x, __half* y, int pixels, int C, int xcs, int xco, int ycs, int yco,
                                                                   const float* __restrict__ param, int shared, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = ACT_THREADS / tg;
    const int c0 = 8 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(8, C - c0);
    float pa[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) pa[j] = (MODE != FCN_ACT_TANH && j < nv) ? param[shared ? 0 : c0 + j] : 0.f;
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        union { uint4 u; __half h[8]; } in, out;
        in.u = *reinterpret_cast<const uint4*>(x + (size_t)p * xcs + xco + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) out.h[j] = __float2half_rn(act_fwd<MODE>(__half2float(in.h[j]), pa[j]));
        __half* yp = y + (size_t)p * ycs + yco + c0;
        if (nv == 8) {
            *reinterpret_cast<uint4*>(yp) = out.u;
        } else {      // (unrolled and predicated: an index that is no constant would move the unions out of the registers)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) yp[j] = out.h[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- data gradient
// grid (gx, gy).  dx may be dy (accumulate 0): the same one-lane-one-group argument as in the forward.
template <int MODE>
__global__ __launch_bounds__(ACT_THREADS) void act_bwd_data_kernel(const float* dy, const float* __restrict__ ref, float* dx, int pixels, int C, int dcs, int dco,
                                                                    int rcs, int rco, int xcs, int xco, const float* __restrict__ param, int shared,
                                                                    int accumulate, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = ACT_THREADS / tg;
    const int c0 = 4 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(4, C - c0);
    float pa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[j] = (MODE == FCN_ACT_PRELU && j < nv) ? param[shared ? 0 : c0 + j] : 0.f;
    for (long long p = (long long)blockIdx.y * rows + row; p < pixels; p += (long long)gridDim.y * rows) {
        const float4 d4 = *reinterpret_cast<const float4*>(dy + (size_t)p * dcs + dco + c0);
        float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE != FCN_ACT_BIAS) r4 = *reinterpret_cast<const float4*>(ref + (size_t)p * rcs + rco + c0);
        const float d[4] = {d4.x, d4.y, d4.z, d4.w}, r[4] = {r4.x, r4.y, r4.z, r4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = act_bwd<MODE>(d[j], r[j], pa[j]);
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

// ---------------------------------------------------------------------------------------------------------------- parameter gradient
// grid (gx, slabs): workspace[slab * C4 + c] = the slab's sum of dy * x * [x <= 0] (PReLU) or of dy (Bias)
template <int MODE>
__global__ __launch_bounds__(ACT_THREADS) void act_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ x, int pixels, int C, int dcs, int dco,
                                                                    int xcs, int xco, int tg, int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[ACT_THREADS];
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = ACT_THREADS / tg;
    const int g = blockIdx.x * tg + gl;
    const bool live = 4 * g < C;
    const int c0 = 4 * (live ? g : 0);
    const int p0 = blockIdx.y * slab_px;
    const int p1 = min(pixels, p0 + slab_px);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int p = p0 + row; p < p1; p += rows) {
            const float4 d = *reinterpret_cast<const float4*>(dy + (size_t)p * dcs + dco + c0);
            if (MODE == FCN_ACT_PRELU) {
                const float4 v = *reinterpret_cast<const float4*>(x + (size_t)p * xcs + xco + c0);
                s.x += v.x <= 0.f ? d.x * v.x : 0.f;
                s.y += v.y <= 0.f ? d.y * v.y : 0.f;
                s.z += v.z <= 0.f ? d.z * v.z : 0.f;
                s.w += v.w <= 0.f ? d.w * v.w : 0.f;
            } else {
                s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
            }
        }
    red[tid] = s;
    __syncthreads();
    if (live && row == 0) {      // rows ascending, by the row-0 thread of each group column
        float4 t = red[gl];
        for (int q = 1; q < rows; ++q) {
            const float4 u = red[q * tg + gl];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        *reinterpret_cast<float4*>(ws + (size_t)blockIdx.y * C4 + 4 * g) = t;
    }
}

// grid ((C + 3) / 4): one wave per channel, four channels per workgroup; out[c] is overwritten
__global__ __launch_bounds__(ACT_THREADS) void act_bwd_final_kernel(const float* __restrict__ ws, int slabs, int C, int C4, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;      // (uniform over the wave)
    float a = 0.f;
    for (int s = lane; s < slabs; s += 64) a += ws[(size_t)s * C4 + c];
    for (int off = 32; off >= 1; off >>= 1) {
        const float a2 = __shfl_down(a, off, 64);
        if (lane < off) a += a2;
    }
    if (lane == 0) out[c] = a;
}

// channel_shared: one value, the per-channel sums folded in ascending order by one thread
__global__ void act_bwd_shared_kernel(const float* __restrict__ sums, int C, float* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += sums[c];
    out[0] = a;
}

inline bool act_view_in(int C, int cstride, int coffset) { return coffset >= 0 && cstride >= coffset + C; }
inline bool act_view_ok(int cstride, int coffset, int epg) { return cstride % epg == 0 && coffset % epg == 0; }
inline bool act_mode_ok(int mode) { return mode == FCN_ACT_PRELU || mode == FCN_ACT_TANH || mode == FCN_ACT_BIAS; }

}  // namespace
}  // namespace fcn

using namespace fcn;

size_t fcn_act_workspace_bytes(int pixels, int C) {
    if (pixels <= 0 || C <= 0) return 0;
    const ActTile t = act_tile(pixels, C, 4);
    return ((size_t)t.slabs + 1) * ((C + 3) / 4 * 4) * sizeof(float);      // the slabs' sums, then the per-channel sums of a shared parameter
}

int fcn_act_fwd_f32(const float* x, float* y, float* keep, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                    int keep_cstride, int mode, const float* param, int param_shared, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "act_fwd: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_fwd: non-positive extent");
    FCN_REQUIRE(act_mode_ok(mode), FCN_E_ARG, "act_fwd: unknown mode %d", mode);
    FCN_REQUIRE(mode == FCN_ACT_TANH || param, FCN_E_ARG, "act_fwd: PReLU and Bias need their parameter");
    FCN_REQUIRE(act_view_in(C, x_cstride, x_coffset) && act_view_in(C, y_cstride, y_coffset) && (!keep || keep_cstride >= C), FCN_E_ARG,
                "act_fwd: channel slice out of range");
    FCN_REQUIRE(act_view_ok(x_cstride, x_coffset, 4) && act_view_ok(y_cstride, y_coffset, 4) && (!keep || keep_cstride % 4 == 0), FCN_E_ALIGN,
                "act_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)keep) & 15) == 0 && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_fwd: x, y and keep must be 16-byte aligned");
    const ActTile t = act_tile(pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(ACT_THREADS);
    const int sh = param_shared ? 1 : 0;
    if (mode == FCN_ACT_PRELU)
        hipLaunchKernelGGL(act_fwd_f32_kernel<FCN_ACT_PRELU>, grid, block, 0, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, keep_cstride, param, sh, t.tg);
    else if (mode == FCN_ACT_TANH)
        hipLaunchKernelGGL(act_fwd_f32_kernel<FCN_ACT_TANH>, grid, block, 0, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, keep_cstride, param, sh, t.tg);
    else
        hipLaunchKernelGGL(act_fwd_f32_kernel<FCN_ACT_BIAS>, grid, block, 0, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, keep_cstride, param, sh, t.tg);
    FCN_LAUNCH_CHECK("act_fwd_f32_kernel");
    return 0;
}

int fcn_act_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset, int mode,
                    const float* param, int param_shared, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "act_fwd_f16: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_fwd_f16: non-positive extent");
    FCN_REQUIRE(act_mode_ok(mode), FCN_E_ARG, "act_fwd_f16: unknown mode %d", mode);
    FCN_REQUIRE(mode == FCN_ACT_TANH || param, FCN_E_ARG, "act_fwd_f16: PReLU and Bias need their parameter");
    FCN_REQUIRE(act_view_in(C, x_cstride, x_coffset) && act_view_in(C, y_cstride, y_coffset), FCN_E_ARG, "act_fwd_f16: channel slice out of range");
    FCN_REQUIRE(act_view_ok(x_cstride, x_coffset, 8) && act_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "act_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_fwd_f16: x and y must be 16-byte aligned");
    const ActTile t = act_tile(pixels, C, 8);
    const dim3 grid(t.gx, t.gy), block(ACT_THREADS);
    const __half* xh = static_cast<const __half*>(x);
    __half* yh = static_cast<__half*>(y);
    const int sh = param_shared ? 1 : 0;
    if (mode == FCN_ACT_PRELU)
        hipLaunchKernelGGL(act_fwd_f16_kernel<FCN_ACT_PRELU>, grid, block, 0, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, param, sh, t.tg);
    else if (mode == FCN_ACT_TANH)
        hipLaunchKernelGGL(act_fwd_f16_kernel<FCN_ACT_TANH>, grid, block, 0, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, param, sh, t.tg);
    else
        hipLaunchKernelGGL(act_fwd_f16_kernel<FCN_ACT_BIAS>, grid, block, 0, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, param, sh, t.tg);
    FCN_LAUNCH_CHECK("act_fwd_f16_kernel");
    return 0;
}

int fcn_act_bwd_data_f32(const float* dy, const float* ref, float* dx, int pixels, int C, int dy_cstride, int dy_coffset, int ref_cstride,
                         int ref_coffset, int dx_cstride, int dx_coffset, int mode, const float* param, int param_shared, int accumulate,
                         fcn_stream_t s) {
    FCN_REQUIRE(dy && dx, FCN_E_ARG, "act_bwd_data: null dy / dx");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_bwd_data: non-positive extent");
    FCN_REQUIRE(act_mode_ok(mode), FCN_E_ARG, "act_bwd_data: unknown mode %d", mode);
    const bool need_ref = mode != FCN_ACT_BIAS;
    FCN_REQUIRE(!need_ref || ref, FCN_E_ARG, "act_bwd_data: PReLU needs the layer's input, TanH its output");
    FCN_REQUIRE(mode != FCN_ACT_PRELU || param, FCN_E_ARG, "act_bwd_data: PReLU needs its slopes");
    FCN_REQUIRE(act_view_in(C, dy_cstride, dy_coffset) && act_view_in(C, dx_cstride, dx_coffset) &&
                    (!need_ref || act_view_in(C, ref_cstride, ref_coffset)),
                FCN_E_ARG, "act_bwd_data: channel slice out of range");
    FCN_REQUIRE(act_view_ok(dy_cstride, dy_coffset, 4) && act_view_ok(dx_cstride, dx_coffset, 4) &&
                    (!need_ref || act_view_ok(ref_cstride, ref_coffset, 4)),
                FCN_E_ALIGN, "act_bwd_data: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)dy | (uintptr_t)dx | (need_ref ? (uintptr_t)ref : 0)) & 15) == 0 && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_bwd_data: dy, ref and dx must be 16-byte aligned");
    const ActTile t = act_tile(pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(ACT_THREADS);
    const int sh = param_shared ? 1 : 0, acc = accumulate ? 1 : 0;
    if (mode == FCN_ACT_PRELU)
        hipLaunchKernelGGL(act_bwd_data_kernel<FCN_ACT_PRELU>, grid, block, 0, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset,
                           ref_cstride, ref_coffset, dx_cstride, dx_coffset, param, sh, acc, t.tg);
    else if (mode == FCN_ACT_TANH)
        hipLaunchKernelGGL(act_bwd_data_kernel<FCN_ACT_TANH>, grid, block, 0, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset,
                           ref_cstride, ref_coffset, dx_cstride, dx_coffset, param, sh, acc, t.tg);
    else
        hipLaunchKernelGGL(act_bwd_data_kernel<FCN_ACT_BIAS>, grid, block, 0, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset,
                           ref_cstride, ref_coffset, dx_cstride, dx_coffset, param, sh, acc, t.tg);
    FCN_LAUNCH_CHECK("act_bwd_data_kernel");
    return 0;
}

int fcn_act_bwd_param_f32(const float* dy, const float* x, float* dparam, int pixels, int C, int dy_cstride, int dy_coffset, int x_cstride,
                          int x_coffset, int mode, int param_shared, void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(mode == FCN_ACT_PRELU || mode == FCN_ACT_BIAS, FCN_E_ARG, "act_bwd_param: mode %d has no parameter", mode);
    FCN_REQUIRE(dy && dparam && d_workspace, FCN_E_ARG, "act_bwd_param: null dy / dparam / workspace");
    const bool need_x = mode == FCN_ACT_PRELU;
    FCN_REQUIRE(!need_x || x, FCN_E_ARG, "act_bwd_param: PReLU needs the layer's input");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_bwd_param: non-positive extent");
    FCN_REQUIRE(act_view_in(C, dy_cstride, dy_coffset) && (!need_x || act_view_in(C, x_cstride, x_coffset)), FCN_E_ARG,
                "act_bwd_param: channel slice out of range");
    FCN_REQUIRE(act_view_ok(dy_cstride, dy_coffset, 4) && (!need_x || act_view_ok(x_cstride, x_coffset, 4)), FCN_E_ALIGN,
                "act_bwd_param: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)dy | (need_x ? (uintptr_t)x : 0) | (uintptr_t)d_workspace) & 15) == 0 && ((uintptr_t)dparam & 3) == 0, FCN_E_ALIGN,
                "act_bwd_param: dy, x and the workspace must be 16-byte aligned");
    const ActTile t = act_tile(pixels, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    float* sums = param_shared ? ws + (size_t)t.slabs * C4 : dparam;
    if (mode == FCN_ACT_PRELU)
        hipLaunchKernelGGL(act_bwd_slab_kernel<FCN_ACT_PRELU>, dim3(t.gx, t.slabs), dim3(ACT_THREADS), 0, as_stream(s), dy, x, pixels, C, dy_cstride,
                           dy_coffset, x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    else
        hipLaunchKernelGGL(act_bwd_slab_kernel<FCN_ACT_BIAS>, dim3(t.gx, t.slabs), dim3(ACT_THREADS), 0, as_stream(s), dy, x, pixels, C, dy_cstride,
                           dy_coffset, x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("act_bwd_slab_kernel");
    hipLaunchKernelGGL(act_bwd_final_kernel, dim3((C + 3) / 4), dim3(ACT_THREADS), 0, as_stream(s), ws, t.slabs, C, C4, sums);
    FCN_LAUNCH_CHECK("act_bwd_final_kernel");
    if (param_shared) {
        hipLaunchKernelGGL(act_bwd_shared_kernel, dim3(1), dim3(64), 0, as_stream(s), sums, C, dparam);
        FCN_LAUNCH_CHECK("act_bwd_shared_kernel");
    }
    return 0;
}
