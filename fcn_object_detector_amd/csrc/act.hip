// One-bottom activations with (PReLU, Bias) or without (TanH) a learned per-channel parameter, on NHWC views (Caffe PReLULayer,
// BiasLayer over the channel axis, TanHLayer):
//   PReLU  y = x > 0 ? x : a[c] * x      dx (+)= x > 0 ? dy : a[c] * dy      da[c] = sum_p dy * x * [x <= 0]
//   TanH   y = tanh(x)                   dx (+)= dy * (1 - y * y)
//   Bias   y = x + b[c]                  dx (+)= dy                          db[c] = sum_p dy
//
// Work layout: that of chan_group.h.  The forward and the data gradient are its streaming templates over ActFn, whose prologue reads
// the parameters of the lane's group once - never per pixel.
//
// The parameter gradient uses no atomics: a workgroup folds its slab of pixels, the slabs' partial sums go to the workspace, and a second
// launch folds them per channel (both folds are chan_group.h's, in their fixed orders).  A shared parameter (Caffe's channel_shared) is
// the fold of those per-channel sums over the channels, ascending, by one thread of a third launch.  The same call gives the same bits.
#include "chan_group.h"

namespace fcn {
namespace {

template <int MODE>
struct ActFn {
    typedef float Op;      // the channel's slope or bias
    static constexpr bool BWD_REF = MODE != FCN_ACT_BIAS;
    const float* __restrict__ param;
    int shared;

    __device__ Op fwd_op(int c, bool live) const { return (MODE != FCN_ACT_TANH && live) ? param[shared ? 0 : c] : 0.f; }
    __device__ Op bwd_op(int c, bool live) const { return (MODE == FCN_ACT_PRELU && live) ? param[shared ? 0 : c] : 0.f; }

    __device__ float fwd(float v, float a) const {
        if (MODE == FCN_ACT_PRELU) return v > 0.f ? v : a * v;
        if (MODE == FCN_ACT_TANH) return tanhf(v);
        return v + a;
    }

    // dy -> dx; r is the layer's input x (PReLU) or its output y (TanH)
    __device__ float bwd(float d, float r, float a) const {
        if (MODE == FCN_ACT_PRELU) return r > 0.f ? d : a * d;
        if (MODE == FCN_ACT_TANH) return d * (1.f - r * r);
        return d;
    }
};

// ---------------------------------------------------------------------------------------------------------------- parameter gradient
// grid (gx, slabs): workspace[slab * C4 + c] = the slab's sum of dy * x * [x <= 0] (PReLU) or of dy (Bias)
template <int MODE>
__global__ __launch_bounds__(CG_THREADS) void act_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ x, int pixels, int C, int dcs, int dco,
                                                                   int xcs, int xco, int tg, int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[CG_THREADS];
    const CgLane l = cg_lane<4>(tg, C);
    const bool live = l.nv > 0;
    const int p0 = blockIdx.y * slab_px;
    const int p1 = min(pixels, p0 + slab_px);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int p = p0 + l.row; p < p1; p += l.rows) {
            const float4 d = *reinterpret_cast<const float4*>(dy + (size_t)p * dcs + dco + l.c0);
            if (MODE == FCN_ACT_PRELU) {
                const float4 v = *reinterpret_cast<const float4*>(x + (size_t)p * xcs + xco + l.c0);
                s.x += v.x <= 0.f ? d.x * v.x : 0.f;
                s.y += v.y <= 0.f ? d.y * v.y : 0.f;
                s.z += v.z <= 0.f ? d.z * v.z : 0.f;
                s.w += v.w <= 0.f ? d.w * v.w : 0.f;
            } else {
                s = cg_add(s, d);
            }
        }
    s = cg_fold_rows(s, red, l, tg);
    if (live && l.row == 0) *reinterpret_cast<float4*>(ws + (size_t)blockIdx.y * C4 + l.c0) = s;
}

// grid ((C + 3) / 4): one wave per channel, four channels per workgroup; out[c] is overwritten
__global__ __launch_bounds__(CG_THREADS) void act_bwd_final_kernel(const float* __restrict__ ws, int slabs, int C, int C4, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;      // (uniform over the wave)
    float a[1];
    cg_fold_slabs(ws + c, slabs, C4, lane, a);
    if (lane == 0) out[c] = a[0];
}

// channel_shared: one value, the per-channel sums folded in ascending order by one thread
__global__ void act_bwd_shared_kernel(const float* __restrict__ sums, int C, float* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += sums[c];
    out[0] = a;
}

inline bool act_mode_ok(int mode) { return mode == FCN_ACT_PRELU || mode == FCN_ACT_TANH || mode == FCN_ACT_BIAS; }

// go(functor of the mode): the launch, written once per entry point
template <class Launch>
inline void act_dispatch(int mode, const float* param, int shared, Launch go) {
    if (mode == FCN_ACT_PRELU) go(ActFn<FCN_ACT_PRELU>{param, shared});
    else if (mode == FCN_ACT_TANH) go(ActFn<FCN_ACT_TANH>{param, shared});
    else go(ActFn<FCN_ACT_BIAS>{param, shared});
}

}  // namespace
}  // namespace fcn

using namespace fcn;

size_t fcn_act_workspace_bytes(int pixels, int C) {
    if (pixels <= 0 || C <= 0) return 0;
    const CgTile t = cg_tile(1, pixels, C, 4);
    return ((size_t)t.slabs + 1) * ((C + 3) / 4 * 4) * sizeof(float);      // the slabs' sums, then the per-channel sums of a shared parameter
}

int fcn_act_fwd_f32(const float* x, float* y, float* keep, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                    int keep_cstride, int mode, const float* param, int param_shared, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "act_fwd: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_fwd: non-positive extent");
    FCN_REQUIRE(act_mode_ok(mode), FCN_E_ARG, "act_fwd: unknown mode %d", mode);
    FCN_REQUIRE(mode == FCN_ACT_TANH || param, FCN_E_ARG, "act_fwd: PReLU and Bias need their parameter");
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset) && (!keep || keep_cstride >= C), FCN_E_ARG,
                "act_fwd: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4) && cg_view_ok(y_cstride, y_coffset, 4) && (!keep || keep_cstride % 4 == 0), FCN_E_ALIGN,
                "act_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, y, keep) && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_fwd: x, y and keep must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    const int sh = param_shared ? 1 : 0;
    act_dispatch(mode, param, sh, [&](auto f) {
        hipLaunchKernelGGL(cg_map_f32_kernel<decltype(f)>, grid, block, 0, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, keep_cstride, t.tg, f);
    });
    FCN_LAUNCH_CHECK("act_fwd_f32_kernel");
    return 0;
}

int fcn_act_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset, int mode,
                    const float* param, int param_shared, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "act_fwd_f16: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "act_fwd_f16: non-positive extent");
    FCN_REQUIRE(act_mode_ok(mode), FCN_E_ARG, "act_fwd_f16: unknown mode %d", mode);
    FCN_REQUIRE(mode == FCN_ACT_TANH || param, FCN_E_ARG, "act_fwd_f16: PReLU and Bias need their parameter");
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset), FCN_E_ARG, "act_fwd_f16: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 8) && cg_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "act_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE(cg_aligned16(x, y) && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_fwd_f16: x and y must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 8);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    const __half* xh = static_cast<const __half*>(x);
    __half* yh = static_cast<__half*>(y);
    const int sh = param_shared ? 1 : 0;
    act_dispatch(mode, param, sh, [&](auto f) {
        hipLaunchKernelGGL(cg_map_f16_kernel<decltype(f)>, grid, block, 0, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset,
                           t.tg, f);
    });
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
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, dx_cstride, dx_coffset) &&
                    (!need_ref || cg_view_in(C, ref_cstride, ref_coffset)),
                FCN_E_ARG, "act_bwd_data: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(dx_cstride, dx_coffset, 4) &&
                    (!need_ref || cg_view_ok(ref_cstride, ref_coffset, 4)),
                FCN_E_ALIGN, "act_bwd_data: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, dx, need_ref ? ref : nullptr) && ((uintptr_t)param & 3) == 0, FCN_E_ALIGN,
                "act_bwd_data: dy, ref and dx must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    const int sh = param_shared ? 1 : 0, acc = accumulate ? 1 : 0;
    act_dispatch(mode, param, sh, [&](auto f) {
        hipLaunchKernelGGL(cg_bwd_f32_kernel<decltype(f)>, grid, block, 0, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset, ref_cstride,
                           ref_coffset, dx_cstride, dx_coffset, acc, t.tg, f);
    });
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
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && (!need_x || cg_view_in(C, x_cstride, x_coffset)), FCN_E_ARG,
                "act_bwd_param: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && (!need_x || cg_view_ok(x_cstride, x_coffset, 4)), FCN_E_ALIGN,
                "act_bwd_param: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, need_x ? x : nullptr, d_workspace) && ((uintptr_t)dparam & 3) == 0, FCN_E_ALIGN,
                "act_bwd_param: dy, x and the workspace must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    float* sums = param_shared ? ws + (size_t)t.slabs * C4 : dparam;
    if (mode == FCN_ACT_PRELU)
        hipLaunchKernelGGL(act_bwd_slab_kernel<FCN_ACT_PRELU>, dim3(t.gx, t.slabs), dim3(CG_THREADS), 0, as_stream(s), dy, x, pixels, C, dy_cstride,
                           dy_coffset, x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    else
        hipLaunchKernelGGL(act_bwd_slab_kernel<FCN_ACT_BIAS>, dim3(t.gx, t.slabs), dim3(CG_THREADS), 0, as_stream(s), dy, x, pixels, C, dy_cstride,
                           dy_coffset, x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("act_bwd_slab_kernel");
    hipLaunchKernelGGL(act_bwd_final_kernel, dim3((C + 3) / 4), dim3(CG_THREADS), 0, as_stream(s), ws, t.slabs, C, C4, sums);
    FCN_LAUNCH_CHECK("act_bwd_final_kernel");
    if (param_shared) {
        hipLaunchKernelGGL(act_bwd_shared_kernel, dim3(1), dim3(64), 0, as_stream(s), sums, C, dparam);
        FCN_LAUNCH_CHECK("act_bwd_shared_kernel");
    }
    return 0;
}
