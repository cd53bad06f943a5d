// One-bottom activations without a learned parameter, on NHWC views (Caffe ELULayer, ClipLayer - and with it the MobileNet forks' ReLU6 -,
// AbsValLayer, BNLLLayer, SwishLayer).  a = alpha (ELU), beta (Swish) or lo (Clip); b = hi (Clip):
//   ELU     y = x > 0 ? x : a * expm1(x)                             dx (+)= dy * (y > 0 ? 1 : y + a)               reads y
//   Clip    y = min(max(x, a), b)                                    dx (+)= dy * [a < y < b]                       reads y
//   AbsVal  y = |x|                                                  dx (+)= dy * sign(x), sign(0) = 0              reads x
//   BNLL    y = x > 0 ? x + log1p(exp(-x)) : log1p(exp(x))           dx (+)= dy * (-expm1(-y))                      reads y
//   Swish   y = x * s, s = 1 / (1 + exp(-a x))                       dx (+)= dy * (a y + s (1 - a y))               reads x
//
// Work layout and kernels: the streaming templates of chan_group.h over NeuronFn, with the workgroups of a launch capped at
// NEURON_MAX_GROUPS in all.  No LDS, no atomics, one writer per element: the same call gives the same bits.  The mode is a template
// parameter: no per-element branch on it survives.
#include "chan_group.h"

namespace fcn {
namespace {

constexpr int NEURON_MAX_GROUPS = 2048;      // workgroups of a launch: 8 per CU of a 256-CU part, every wave slot taken

template <int MODE>
struct NeuronFn {
    struct Op {};      // no per-channel operand
    static constexpr bool BWD_REF = true;
    float a, b;

    __device__ Op fwd_op(int, bool) const { return Op(); }
    __device__ Op bwd_op(int, bool) const { return Op(); }

    __device__ float fwd(float v, Op) const {
        if (MODE == FCN_NEURON_ELU) return v > 0.f ? v : a * expm1f(v);
        if (MODE == FCN_NEURON_CLIP) return fminf(fmaxf(v, a), b);
        if (MODE == FCN_NEURON_ABSVAL) return fabsf(v);
        if (MODE == FCN_NEURON_BNLL) return v > 0.f ? v + log1pf(expf(-v)) : log1pf(expf(v));
        return v / (1.f + expf(-a * v));
    }

    // dy -> dx; r is the layer's output y (ELU, Clip, BNLL) or its input x (AbsVal, Swish)
    __device__ float bwd(float d, float r, Op) const {
        if (MODE == FCN_NEURON_ELU) return r > 0.f ? d : d * (r + a);
        if (MODE == FCN_NEURON_CLIP) return (r > a && r < b) ? d : 0.f;
        if (MODE == FCN_NEURON_ABSVAL) return r > 0.f ? d : (r < 0.f ? -d : 0.f);
        if (MODE == FCN_NEURON_BNLL) return d * -expm1f(-r);
        const float s = 1.f / (1.f + expf(-a * r)), ay = a * (r * s);
        return d * (ay + s * (1.f - ay));
    }
};

inline bool neuron_mode_ok(int mode) { return mode >= FCN_NEURON_ELU && mode <= FCN_NEURON_SWISH; }
// (written so that a NaN is refused as well)
inline bool neuron_params_ok(int mode, float a, float b) {
    if (mode == FCN_NEURON_ELU) return a >= 0.f;
    if (mode == FCN_NEURON_CLIP) return a < b;
    return true;
}

// go(functor of the mode): the launch, written once per entry point
template <class Launch>
inline void neuron_dispatch(int mode, float a, float b, Launch go) {
    switch (mode) {
        case FCN_NEURON_ELU: go(NeuronFn<FCN_NEURON_ELU>{a, b}); break;
        case FCN_NEURON_CLIP: go(NeuronFn<FCN_NEURON_CLIP>{a, b}); break;
        case FCN_NEURON_ABSVAL: go(NeuronFn<FCN_NEURON_ABSVAL>{a, b}); break;
        case FCN_NEURON_BNLL: go(NeuronFn<FCN_NEURON_BNLL>{a, b}); break;
        default: go(NeuronFn<FCN_NEURON_SWISH>{a, b}); break;
    }
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
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset) && (!keep || keep_cstride >= C), FCN_E_ARG,
                "neuron_fwd: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4) && cg_view_ok(y_cstride, y_coffset, 4) && (!keep || keep_cstride % 4 == 0), FCN_E_ALIGN,
                "neuron_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, y, keep), FCN_E_ALIGN, "neuron_fwd: x, y and keep must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4, NEURON_MAX_GROUPS);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    neuron_dispatch(mode, a, b, [&](auto f) {
        hipLaunchKernelGGL(cg_map_f32_kernel<decltype(f)>, grid, block, 0, as_stream(s), x, y, keep, pixels, C, x_cstride, x_coffset, y_cstride,
                           y_coffset, keep_cstride, t.tg, f);
    });
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
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset), FCN_E_ARG,
                "neuron_fwd_f16: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 8) && cg_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "neuron_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE(cg_aligned16(x, y), FCN_E_ALIGN, "neuron_fwd_f16: x and y must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 8, NEURON_MAX_GROUPS);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    const __half* xh = static_cast<const __half*>(x);
    __half* yh = static_cast<__half*>(y);
    neuron_dispatch(mode, a, b, [&](auto f) {
        hipLaunchKernelGGL(cg_map_f16_kernel<decltype(f)>, grid, block, 0, as_stream(s), xh, yh, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset,
                           t.tg, f);
    });
    FCN_LAUNCH_CHECK("neuron_fwd_f16_kernel");
    return 0;
}

int fcn_neuron_bwd_f32(const float* dy, const float* ref, float* dx, int pixels, int C, int dy_cstride, int dy_coffset, int ref_cstride,
                       int ref_coffset, int dx_cstride, int dx_coffset, int mode, float a, float b, int accumulate, fcn_stream_t s) {
    FCN_REQUIRE(dy && ref && dx, FCN_E_ARG, "neuron_bwd: null dy / ref / dx");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "neuron_bwd: non-positive extent");
    FCN_REQUIRE(neuron_mode_ok(mode), FCN_E_ARG, "neuron_bwd: unknown mode %d", mode);
    FCN_REQUIRE(neuron_params_ok(mode, a, b), FCN_E_ARG, "neuron_bwd: ELU needs alpha >= 0, Clip needs lo < hi (got %g, %g)", (double)a, (double)b);
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, dx_cstride, dx_coffset) && cg_view_in(C, ref_cstride, ref_coffset),
                FCN_E_ARG, "neuron_bwd: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(dx_cstride, dx_coffset, 4) && cg_view_ok(ref_cstride, ref_coffset, 4),
                FCN_E_ALIGN, "neuron_bwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, dx, ref), FCN_E_ALIGN, "neuron_bwd: dy, ref and dx must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4, NEURON_MAX_GROUPS);
    const dim3 grid(t.gx, t.gy), block(CG_THREADS);
    const int acc = accumulate ? 1 : 0;
    neuron_dispatch(mode, a, b, [&](auto f) {
        hipLaunchKernelGGL(cg_bwd_f32_kernel<decltype(f)>, grid, block, 0, as_stream(s), dy, ref, dx, pixels, C, dy_cstride, dy_coffset, ref_cstride,
                           ref_coffset, dx_cstride, dx_coffset, acc, t.tg, f);
    });
    FCN_LAUNCH_CHECK("neuron_bwd_kernel");
    return 0;
}
