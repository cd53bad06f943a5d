// Gated Scale (Caffe ScaleLayer with two bottoms over axis 0, the SENet release's Axpy) on NHWC views: y[n, p, c] = x[n, p, c] *
// gate[n, c] (+ r[n, p, c], relu), and its two gradients dx (+)= dy * gate, dgate[n, c] (+)= sum_p dy[n, p, c] * x[n, p, c].
//
// Work layout, that of batchnorm.hip with the image as the grid's z axis: a lane owns ONE 16-byte channel group of a pixel (4 floats /
// 8 halves), the `tg` lanes next to each other own consecutive groups of the same pixel, the 256 / tg rows of a workgroup own
// consecutive pixels of ONE image.  The gate values of the lane's group are read once, in its prologue - never per pixel.  A C that
// is no multiple of the group stores its last group element by element: channels outside coffset .. coffset + C - 1 are never
// written; loads of whole groups stay inside the pixel because strides and offsets are multiples of the group.  The gate is read
// element by element (its rows are C floats at any stride >= C, 4-byte aligned).
//
// The gate gradient uses no atomics: a workgroup folds its slab of one image's pixels (rows ascending), the slabs' partial sums go to
// the workspace, and a second launch folds them per (image, channel) in a fixed order - lane l of the wave folds slabs l, l + 64, ...
// ascending, then the lanes fold by halves (32, 16, .. 1).  One launch pair covers all images; the same call gives the same bits.
#include "common.h"

#include <hip/hip_fp16.h>

namespace fcn {
namespace {

constexpr int GATE_THREADS = 256;
constexpr int GATE_MAX_SLABS = 1024;
constexpr int GATE_MAX_IMAGES = 65535;      // the grid's z extent

struct GateTile {
    int tg;        // channel groups side by side in a workgroup (power of two, <= 16)
    int rows;      // pixels side by side: GATE_THREADS / tg
    int gx;        // workgroups along the channel groups
    int gy;        // workgroups along the pixels of an image (the streaming launches: grid-stride over the rest)
    int slabs;     // slabs of pixels per image (the gate gradient) ...
    int slab_px;   // ... of this many pixels each (the last one shorter); never below `rows`
};

inline GateTile gate_tile(int N, int ppi, int C, int epg) {
    GateTile t;
    const int cg = (C + epg - 1) / epg;
    t.tg = 1;
    while (t.tg < cg && t.tg < 16) t.tg <<= 1;
    t.rows = GATE_THREADS / t.tg;
    t.gx = (cg + t.tg - 1) / t.tg;
    const long long per_image = (long long)t.gx * N;
    long long gy = ((long long)ppi + t.rows - 1) / t.rows;
    long long cap = 16384 / per_image;
    if (cap < 1) cap = 1;
    t.gy = (int)(gy < cap ? gy : cap);
    long long want = 2048 / per_image;
    if (want < 1) want = 1;
    if (want > GATE_MAX_SLABS) want = GATE_MAX_SLABS;
    t.slab_px = (int)((ppi + want - 1) / want);
    if (t.slab_px < t.rows) t.slab_px = t.rows;      // every row of a workgroup gets a pixel
    t.slabs = (ppi + t.slab_px - 1) / t.slab_px;
    return t;
}

// ---------------------------------------------------------------------------------------------------------------- forward, data gradient
// grid (gx, gy, N).  y may be x or r: a lane reads its group of a pixel before it writes it, and no other lane touches that group.
__global__ __launch_bounds__(GATE_THREADS) void gate_fwd_f32_kernel(const float* x, const float* __restrict__ gate, const float* r, float* y, int ppi, int C,
                                                                     int xcs, int xco, int grs, int rcs, int rco, int ycs, int yco, int relu, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = GATE_THREADS / tg;
    const int c0 = 4 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(4, C - c0);
    const int n = blockIdx.z;
    float ga[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ga[j] = j < nv ? gate[(size_t)n * grs + c0 + j] : 0.f;
    const size_t base = (size_t)n * ppi;
    for (long long p = (long long)blockIdx.y * rows + row; p < ppi; p += (long long)gridDim.y * rows) {
        const float4 v4 = *reinterpret_cast<const float4*>(x + (base + p) * xcs + xco + c0);
        float o[4] = {v4.x * ga[0], v4.y * ga[1], v4.z * ga[2], v4.w * ga[3]};
        if (r) {
            const float4 r4 = *reinterpret_cast<const float4*>(r + (base + p) * rcs + rco + c0);
            o[0] += r4.x; o[1] += r4.y; o[2] += r4.z; o[3] += r4.w;
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = o[j] > 0.f ? o[j] : 0.f;
        }
        float* yp = y + (base + p) * ycs + yco + c0;
        if (nv == 4) {
            *reinterpret_cast<float4*>(yp) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) yp[j] = o[j];
        }
    }
}

// halves in, halves out, float32 gate and arithmetic, one rounding to half; a lane owns 8 channels
__global__ __launch_bounds__(GATE_THREADS) void gate_fwd_f16_kernel(const __half* x, const float* __restrict__ gate, const __half* r, __half* y, int ppi, int C,
                                                                     int xcs, int xco, int grs, int rcs, int rco, int ycs, int yco, int relu, int tg) {
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = GATE_THREADS / tg;
    const int c0 = 8 * (blockIdx.x * tg + gl);
    if (c0 >= C) return;
    const int nv = min(8, C - c0);
    const int n = blockIdx.z;
    float ga[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ga[j] = j < nv ? gate[(size_t)n * grs + c0 + j] : 0.f;
    const size_t base = (size_t)n * ppi;
    for (long long p = (long long)blockIdx.y * rows + row; p < ppi; p += (long long)gridDim.y * rows) {
        union { uint4 u; __half h[8]; } in, res, out;
        in.u = *reinterpret_cast<const uint4*>(x + (base + p) * xcs + xco + c0);
        res.u = make_uint4(0u, 0u, 0u, 0u);
        if (r) res.u = *reinterpret_cast<const uint4*>(r + (base + p) * rcs + rco + c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = __half2float(in.h[j]) * ga[j];
            if (r) o += __half2float(res.h[j]);
            if (relu) o = o > 0.f ? o : 0.f;
            out.h[j] = __float2half_rn(o);
        }
        __half* yp = y + (base + p) * ycs + yco + c0;
        if (nv == 8) {
            *reinterpret_cast<uint4*>(yp) = out.u;
        } else {      // (unrolled and predicated: an index that is no constant would move the three unions out of the registers)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < nv) yp[j] = out.h[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- gate gradient
// grid (gx, slabs, N): workspace[(n * slabs + slab) * C4 + c] = sum of dy * x over the slab's pixels of image n
__global__ __launch_bounds__(GATE_THREADS) void gate_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ x, int ppi, int C, int dcs, int dco,
                                                                      int xcs, int xco, int tg, int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[GATE_THREADS];
    const int tid = threadIdx.x, gl = tid % tg, row = tid / tg, rows = GATE_THREADS / tg;
    const int g = blockIdx.x * tg + gl;
    const bool live = 4 * g < C;
    const int c0 = 4 * (live ? g : 0);
    const int n = blockIdx.z;
    const long long p0 = (long long)blockIdx.y * slab_px;
    const long long p1 = min((long long)ppi, p0 + slab_px);
    const size_t base = (size_t)n * ppi;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (long long p = (long long)p0 + row; p < p1; p += rows) {
            const float4 d = *reinterpret_cast<const float4*>(dy + (base + p) * dcs + dco + c0);
            const float4 v = *reinterpret_cast<const float4*>(x + (base + p) * xcs + xco + c0);
            s.x += d.x * v.x; s.y += d.y * v.y; s.z += d.z * v.z; s.w += d.w * v.w;
        }
    red[tid] = s;
    __syncthreads();
    if (live && row == 0) {      // rows ascending, by the row-0 thread of each group column
        float4 t = red[gl];
        for (int q = 1; q < rows; ++q) {
            const float4 u = red[q * tg + gl];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        *reinterpret_cast<float4*>(ws + ((size_t)n * gridDim.y + blockIdx.y) * C4 + 4 * g) = t;
    }
}

// grid ((C + 3) / 4, N): one wave per (image, channel), four channels per workgroup
__global__ __launch_bounds__(GATE_THREADS) void gate_bwd_final_kernel(const float* __restrict__ ws, int slabs, int C, int C4, float* __restrict__ dgate, int grs,
                                                                       int accumulate) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;      // (uniform over the wave)
    const int n = blockIdx.y;
    float a = 0.f;
    for (int s = lane; s < slabs; s += 64) a += ws[((size_t)n * slabs + s) * C4 + c];
    for (int off = 32; off >= 1; off >>= 1) {
        const float a2 = __shfl_down(a, off, 64);
        if (lane < off) a += a2;
    }
    if (lane == 0) {
        float* o = dgate + (size_t)n * grs + c;
        *o = accumulate ? *o + a : a;
    }
}

inline bool gate_view_ok(int cstride, int coffset, int epg) { return cstride % epg == 0 && coffset % epg == 0; }
inline bool gate_view_in(int C, int cstride, int coffset) { return coffset >= 0 && cstride >= coffset + C; }

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
    const GateTile t = gate_tile(N, ppi, C, 4);
    return (size_t)N * t.slabs * ((C + 3) / 4 * 4) * sizeof(float);
}

int fcn_scale_gate_fwd_f32(const float* x, const float* gate, const float* r, float* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                           int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && gate && y, FCN_E_ARG, "scale_gate_fwd: null x / gate / y");
    if (int rc = gate_extents("scale_gate_fwd", N, ppi, C)) return rc;
    FCN_REQUIRE(gate_view_in(C, x_cstride, x_coffset) && gate_view_in(C, y_cstride, y_coffset) && (!r || gate_view_in(C, r_cstride, r_coffset)) &&
                    g_rstride >= C,
                FCN_E_ARG, "scale_gate_fwd: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(gate_view_ok(x_cstride, x_coffset, 4) && gate_view_ok(y_cstride, y_coffset, 4) && (!r || gate_view_ok(r_cstride, r_coffset, 4)),
                FCN_E_ALIGN, "scale_gate_fwd: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)r) & 15) == 0 && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_fwd: x, r and y must be 16-byte aligned");
    const GateTile t = gate_tile(N, ppi, C, 4);
    hipLaunchKernelGGL(gate_fwd_f32_kernel, dim3(t.gx, t.gy, N), dim3(GATE_THREADS), 0, as_stream(s), x, gate, r, y, ppi, C, x_cstride, x_coffset,
                       g_rstride, r_cstride, r_coffset, y_cstride, y_coffset, relu, t.tg);
    FCN_LAUNCH_CHECK("gate_fwd_f32_kernel");
    return 0;
}

int fcn_scale_gate_fwd_f16(const void* x, const float* gate, const void* r, void* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                           int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && gate && y, FCN_E_ARG, "scale_gate_fwd_f16: null x / gate / y");
    if (int rc = gate_extents("scale_gate_fwd_f16", N, ppi, C)) return rc;
    FCN_REQUIRE(gate_view_in(C, x_cstride, x_coffset) && gate_view_in(C, y_cstride, y_coffset) && (!r || gate_view_in(C, r_cstride, r_coffset)) &&
                    g_rstride >= C,
                FCN_E_ARG, "scale_gate_fwd_f16: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(gate_view_ok(x_cstride, x_coffset, 8) && gate_view_ok(y_cstride, y_coffset, 8) && (!r || gate_view_ok(r_cstride, r_coffset, 8)),
                FCN_E_ALIGN, "scale_gate_fwd_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)r) & 15) == 0 && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_fwd_f16: x, r and y must be 16-byte aligned");
    const GateTile t = gate_tile(N, ppi, C, 8);
    hipLaunchKernelGGL(gate_fwd_f16_kernel, dim3(t.gx, t.gy, N), dim3(GATE_THREADS), 0, as_stream(s), static_cast<const __half*>(x), gate,
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
    FCN_REQUIRE(gate_view_in(C, dy_cstride, dy_coffset) && gate_view_in(C, dx_cstride, dx_coffset) && g_rstride >= C, FCN_E_ARG,
                "scale_gate_bwd_data: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(gate_view_ok(dy_cstride, dy_coffset, 4) && gate_view_ok(dx_cstride, dx_coffset, 4), FCN_E_ALIGN,
                "scale_gate_bwd_data: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)dy | (uintptr_t)dx) & 15) == 0 && ((uintptr_t)gate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_bwd_data: dy and dx must be 16-byte aligned");
    const GateTile t = gate_tile(N, ppi, C, 4);
    hipLaunchKernelGGL(gate_fwd_f32_kernel, dim3(t.gx, t.gy, N), dim3(GATE_THREADS), 0, as_stream(s), dy, gate, accumulate ? dx : nullptr, dx, ppi, C,
                       dy_cstride, dy_coffset, g_rstride, dx_cstride, dx_coffset, dx_cstride, dx_coffset, 0, t.tg);
    FCN_LAUNCH_CHECK("gate_fwd_f32_kernel");
    return 0;
}

int fcn_scale_gate_bwd_gate_f32(const float* dy, const float* x, float* dgate, int N, int ppi, int C, int dy_cstride, int dy_coffset,
                                int x_cstride, int x_coffset, int g_rstride, int accumulate, void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(dy && x && dgate && d_workspace, FCN_E_ARG, "scale_gate_bwd_gate: null dy / x / dgate / workspace");
    if (int rc = gate_extents("scale_gate_bwd_gate", N, ppi, C)) return rc;
    FCN_REQUIRE(gate_view_in(C, dy_cstride, dy_coffset) && gate_view_in(C, x_cstride, x_coffset) && g_rstride >= C, FCN_E_ARG,
                "scale_gate_bwd_gate: channel slice out of range, or a gate row shorter than C");
    FCN_REQUIRE(gate_view_ok(dy_cstride, dy_coffset, 4) && gate_view_ok(x_cstride, x_coffset, 4), FCN_E_ALIGN,
                "scale_gate_bwd_gate: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)d_workspace) & 15) == 0 && ((uintptr_t)dgate & 3) == 0, FCN_E_ALIGN,
                "scale_gate_bwd_gate: dy, x and the workspace must be 16-byte aligned");
    const GateTile t = gate_tile(N, ppi, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    hipLaunchKernelGGL(gate_bwd_slab_kernel, dim3(t.gx, t.slabs, N), dim3(GATE_THREADS), 0, as_stream(s), dy, x, ppi, C, dy_cstride, dy_coffset,
                       x_cstride, x_coffset, t.tg, t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("gate_bwd_slab_kernel");
    hipLaunchKernelGGL(gate_bwd_final_kernel, dim3((C + 3) / 4, N), dim3(GATE_THREADS), 0, as_stream(s), ws, t.slabs, C, C4, dgate, g_rstride,
                       accumulate);
    FCN_LAUNCH_CHECK("gate_bwd_final_kernel");
    return 0;
}
