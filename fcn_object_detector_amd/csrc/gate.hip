// Gated Scale (Caffe ScaleLayer with two bottoms over axis 0, the SENet release's Axpy) on NHWC views: y[n, p, c] = x[n, p, c] *
// gate[n, c] (+ r[n, p, c], relu), and its two gradients dx (+)= dy * gate, dgate[n, c] (+)= sum_p dy[n, p, c] * x[n, p, c].
//
// Work layout: that of chan_group.h with the image as the grid's z axis - the rows of a workgroup own consecutive pixels of ONE image.
// The gate values of the lane's group are read once, in its prologue - never per pixel - and element by element (the gate's rows are C
// floats at any stride >= C, 4-byte aligned).  The forward has a second per-pixel operand, the residual, so it is a kernel of its own
// on chan_group.h's lane, load and store helpers and not a functor of its streaming templates.
//
// The gate gradient uses no atomics: a workgroup folds its slab of one image's pixels, the slabs' partial sums go to the workspace, and a
// second launch folds them per (image, channel) - both folds are chan_group.h's, in their fixed orders.  One launch pair covers all
// images; the same call gives the same bits.
#include "chan_group.h"

namespace fcn {
namespace {

constexpr int GATE_MAX_IMAGES = 65535;      // the grid's z extent

// ---------------------------------------------------------------------------------------------------------------- forward, data gradient
// grid (gx, gy, N).  y may be x or r: a lane reads its group of a pixel before it writes it, and no other lane touches that group.
__global__ __launch_bounds__(CG_THREADS) void gate_fwd_f32_kernel(const float* x, const float* __restrict__ gate, const float* r, float* y, int ppi, int C,
                                                                   int xcs, int xco, int grs, int rcs, int rco, int ycs, int yco, int relu, int tg) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    const int n = blockIdx.z;
    float ga[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ga[j] = j < l.nv ? gate[(size_t)n * grs + l.c0 + j] : 0.f;
    const size_t base = (size_t)n * ppi;
    for (long long p = cg_first(l); p < ppi; p += cg_step(l)) {
        float v[4], o[4];
        cg_load(x + (base + p) * xcs + xco + l.c0, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j] * ga[j];
        if (r) {
            float q[4];
            cg_load(r + (base + p) * rcs + rco + l.c0, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += q[j];
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = o[j] > 0.f ? o[j] : 0.f;
        }
        cg_store(y + (base + p) * ycs + yco + l.c0, o, l.nv);
    }
}

// halves in, halves out, float32 gate and arithmetic, one rounding to half; a lane owns 8 channels
__global__ __launch_bounds__(CG_THREADS) void gate_fwd_f16_kernel(const __half* x, const float* __restrict__ gate, const __half* r, __half* y, int ppi, int C,
                                                                   int xcs, int xco, int grs, int rcs, int rco, int ycs, int yco, int relu, int tg) {
    const CgLane l = cg_lane<8>(tg, C);
    if (l.nv <= 0) return;
    const int n = blockIdx.z;
    float ga[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ga[j] = j < l.nv ? gate[(size_t)n * grs + l.c0 + j] : 0.f;
    const size_t base = (size_t)n * ppi;
    for (long long p = cg_first(l); p < ppi; p += cg_step(l)) {
        const CgH8 in = cg_load_h8(x + (base + p) * xcs + xco + l.c0);
        CgH8 res, out;
        res.u = make_uint4(0u, 0u, 0u, 0u);
        if (r) res = cg_load_h8(r + (base + p) * rcs + rco + l.c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = __half2float(in.h[j]) * ga[j];
            if (r) o += __half2float(res.h[j]);
            if (relu) o = o > 0.f ? o : 0.f;
            out.h[j] = __float2half_rn(o);
        }
        cg_store_h8(y + (base + p) * ycs + yco + l.c0, out, l.nv);
    }
}

// ---------------------------------------------------------------------------------------------------------------- gate gradient
// grid (gx, slabs, N): workspace[(n * slabs + slab) * C4 + c] = sum of dy * x over the slab's pixels of image n
__global__ __launch_bounds__(CG_THREADS) void gate_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ x, int ppi, int C, int dcs, int dco,
                                                                    int xcs, int xco, int tg, int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[CG_THREADS];
    const CgLane l = cg_lane<4>(tg, C);
    const bool live = l.nv > 0;
    const int n = blockIdx.z;
    const long long p0 = (long long)blockIdx.y * slab_px;
    const long long p1 = min((long long)ppi, p0 + slab_px);
    const size_t base = (size_t)n * ppi;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (long long p = p0 + l.row; p < p1; p += l.rows) {
            const float4 d = *reinterpret_cast<const float4*>(dy + (base + p) * dcs + dco + l.c0);
            const float4 v = *reinterpret_cast<const float4*>(x + (base + p) * xcs + xco + l.c0);
            s.x += d.x * v.x; s.y += d.y * v.y; s.z += d.z * v.z; s.w += d.w * v.w;
        }
    s = cg_fold_rows(s, red, l, tg);
    if (live && l.row == 0) *reinterpret_cast<float4*>(ws + ((size_t)n * gridDim.y + blockIdx.y) * C4 + l.c0) = s;
}

// grid ((C + 3) / 4, N): one wave per (image, channel), four channels per workgroup
__global__ __launch_bounds__(CG_THREADS) void gate_bwd_final_kernel(const float* __restrict__ ws, int slabs, int C, int C4, float* __restrict__ dgate, int grs,
                                                                     int accumulate) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;      // (uniform over the wave)
    const int n = blockIdx.y;
    float a[1];
    cg_fold_slabs(ws + (size_t)n * slabs * C4 + c, slabs, C4, lane, a);
    if (lane == 0) {
        float* o = dgate + (size_t)n * grs + c;
        *o = accumulate ? *o + a[0] : a[0];
    }
}

// what every entry point refuses about its extents; 0 when they are fine
int gate_extents(const char* who, int N, int ppi, int C) {
    FCN_REQUIRE(N > 0 && ppi > 0 && C > 0, FCN_E_ARG, "%s: non-positive extent", who);
    FCN_REQUIRE(N <= GATE_MAX_IMAGES && (long long)N * ppi < (1ll << 31), FCN_E_UNSUPPORTED, "%s: more than %d images or 2^31 pixels", who,
                GATE_MAX_IMAGES);
    return 0;
}

}  // namespace
}  // namespace fcn

using namespace fcn;

size_t fcn_scale_gate_workspace_bytes(int N, int ppi, int C) {
    if (N <= 0 || ppi <= 0 || C <= 0 || N > GATE_MAX_IMAGES) return 0;
    const CgTile t = cg_tile(N, ppi, C, 4);
    return (size_t)N * t.slabs * ((C + 3) / 4 * 4) * sizeof(float);
}

int fcn_scale_gate_fwd_f32(const float* x, const float* gate, const float* r, float* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                           int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && gate && y, FCN_E_ARG, "scale_gate_fwd: null x / gate / y");
    if (int rc = gate_extents("scale_gate_fwd", N, ppi, C)) return rc;
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset) && (!r || cg_view_in(C, r_cstride, r_coffset)) &&
                    g_rstride >= C,
                FCN_E_ARG, "scale_gate_fwd: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4) && cg_view_ok(y_cstride, y_coffset, 4) && (!r || cg_view_ok(r_cstride, r_coffset, 4)),
                FCN_E_ALIGN, "scale_gate_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, y, r) && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_fwd: x, r and y must be 16-byte aligned");
    const CgTile t = cg_tile(N, ppi, C, 4);
    hipLaunchKernelGGL(gate_fwd_f32_kernel, dim3(t.gx, t.gy, N), dim3(CG_THREADS), 0, as_stream(s), x, gate, r, y, ppi, C, x_cstride, x_coffset,
                       g_rstride, r_cstride, r_coffset, y_cstride, y_coffset, relu, t.tg);
    FCN_LAUNCH_CHECK("gate_fwd_f32_kernel");
    return 0;
}

int fcn_scale_gate_fwd_f16(const void* x, const float* gate, const void* r, void* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                           int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && gate && y, FCN_E_ARG, "scale_gate_fwd_f16: null x / gate / y");
    if (int rc = gate_extents("scale_gate_fwd_f16", N, ppi, C)) return rc;
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset) && (!r || cg_view_in(C, r_cstride, r_coffset)) &&
                    g_rstride >= C,
                FCN_E_ARG, "scale_gate_fwd_f16: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 8) && cg_view_ok(y_cstride, y_coffset, 8) && (!r || cg_view_ok(r_cstride, r_coffset, 8)),
                FCN_E_ALIGN, "scale_gate_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE(cg_aligned16(x, y, r) && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_fwd_f16: x, r and y must be 16-byte aligned");
    const CgTile t = cg_tile(N, ppi, C, 8);
    hipLaunchKernelGGL(gate_fwd_f16_kernel, dim3(t.gx, t.gy, N), dim3(CG_THREADS), 0, as_stream(s), static_cast<const __half*>(x), gate,
                       static_cast<const __half*>(r), static_cast<__half*>(y), ppi, C, x_cstride, x_coffset, g_rstride, r_cstride, r_coffset,
                       y_cstride, y_coffset, relu, t.tg);
    FCN_LAUNCH_CHECK("gate_fwd_f16_kernel");
    return 0;
}

// the forward launch with dy as x and, when it accumulates, dx as the residual: dx = dy * gate (+ dx)
int fcn_scale_gate_bwd_data_f32(const float* dy, const float* gate, float* dx, int N, int ppi, int C, int dy_cstride, int dy_coffset,
                                int g_rstride, int dx_cstride, int dx_coffset, int accumulate, fcn_stream_t s) {
    FCN_REQUIRE(dy && gate && dx, FCN_E_ARG, "scale_gate_bwd_data: null dy / gate / dx");
    if (int rc = gate_extents("scale_gate_bwd_data", N, ppi, C)) return rc;
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, dx_cstride, dx_coffset) && g_rstride >= C, FCN_E_ARG,
                "scale_gate_bwd_data: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(dx_cstride, dx_coffset, 4), FCN_E_ALIGN,
                "scale_gate_bwd_data: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, dx) && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_bwd_data: dy and dx must be 16-byte aligned");
    const CgTile t = cg_tile(N, ppi, C, 4);
    hipLaunchKernelGGL(gate_fwd_f32_kernel, dim3(t.gx, t.gy, N), dim3(CG_THREADS), 0, as_stream(s), dy, gate, accumulate ? dx : nullptr, dx, ppi, C,
                       dy_cstride, dy_coffset, g_rstride, dx_cstride, dx_coffset, dx_cstride, dx_coffset, 0, t.tg);
    FCN_LAUNCH_CHECK("gate_fwd_f32_kernel");
    return 0;
}

int fcn_scale_gate_bwd_gate_f32(const float* dy, const float* x, float* dgate, int N, int ppi, int C, int dy_cstride, int dy_coffset,
                                int x_cstride, int x_coffset, int g_rstride, int accumulate, void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(dy && x && dgate && d_workspace, FCN_E_ARG, "scale_gate_bwd_gate: null dy / x / dgate / workspace");
    if (int rc = gate_extents("scale_gate_bwd_gate", N, ppi, C)) return rc;
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, x_cstride, x_coffset) && g_rstride >= C, FCN_E_ARG,
                "scale_gate_bwd_gate: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(x_cstride, x_coffset, 4), FCN_E_ALIGN,
                "scale_gate_bwd_gate: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, x, d_workspace) && ((uintptr_t)dgate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_bwd_gate: dy, x and the workspace must be 16-byte aligned");
    const CgTile t = cg_tile(N, ppi, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    hipLaunchKernelGGL(gate_bwd_slab_kernel, dim3(t.gx, t.slabs, N), dim3(CG_THREADS), 0, as_stream(s), dy, x, ppi, C, dy_cstride, dy_coffset,
                       x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("gate_bwd_slab_kernel");
    hipLaunchKernelGGL(gate_bwd_final_kernel, dim3((C + 3) / 4, N), dim3(CG_THREADS), 0, as_stream(s), ws, t.slabs, C, C4, dgate, g_rstride,
                       accumulate);
    FCN_LAUNCH_CHECK("gate_bwd_final_kernel");
    return 0;
}
