// BatchNorm / Scale (Caffe BatchNormLayer, ScaleLayer over the channel axis) on NHWC views: the statistics, the fused
// apply y = relu?(gamma * (x - mean) * invstd + beta) and the two backward launches (per-channel reduce, apply).
//
// Work layout of every kernel here: that of chan_group.h, whose tile, lane, load / store and fold helpers they use.  Per-channel
// operands (mean, invstd, gamma, beta, the two backward sums) are read once per thread, in its prologue.
//
// Reductions over pixels (statistics, backward sums) go through chan_group.h's slabs and fixed-order folds, without atomics: the same
// call gives the same bits.  The variance is centred: a slab's M2 = sum (x - slab mean)^2 from a second pass over the slab (which the
// first pass left in the caches), and slabs combine by Chan's parallel formula  M2 = M2a + M2b + (mean_b - mean_a)^2 * na * nb / (na + nb).
#include "chan_group.h"

namespace fcn {
namespace {

// chan_group.h's fold of a workgroup's rows, broadcast to all of them
__device__ inline float4 bn_fold_rows(float4 v, float4* red, float4* bcast, const CgLane& l, int tg) {
    __syncthreads();      // (red / bcast may still be read from the fold before)
    v = cg_fold_rows(v, red, l, tg);
    if (l.row == 0) bcast[l.gl] = v;
    __syncthreads();
    return bcast[l.gl];
}

// Chan et al.: (n, mean, M2) of a set joined with (nb, mb, qb) of the next one
__device__ inline void bn_chan(float& n, float& mean, float& m2, float nb, float mb, float qb) {
    if (nb == 0.f) return;
    if (n == 0.f) {
        n = nb; mean = mb; m2 = qb;
        return;
    }
    const float nt = n + nb, d = mb - mean;
    mean = mean + d * (nb / nt);
    m2 = m2 + qb + d * d * (n * nb / nt);
    n = nt;
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// grid (gx, slabs): workspace[(2 * slab + 0) * C4 + c] = slab mean, [(2 * slab + 1) * C4 + c] = slab M2
__global__ __launch_bounds__(CG_THREADS) void bn_stats_slab_kernel(const float* __restrict__ x, int pixels, int C, int cstride, int coffset,
                                                                    int tg, int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[CG_THREADS];
    __shared__ float4 bcast[16];
    const CgLane l = cg_lane<4>(tg, C);
    const bool live = l.nv > 0;
    const int p0 = blockIdx.y * slab_px;
    const int p1 = min(pixels, p0 + slab_px);
    const float* xp = x + coffset + (live ? l.c0 : 0);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int p = p0 + l.row; p < p1; p += l.rows) s = cg_add(s, *reinterpret_cast<const float4*>(xp + (size_t)p * cstride));
    s = bn_fold_rows(s, red, bcast, l, tg);
    const float inv_n = 1.0f / (float)(p1 - p0);
    const float4 mean = make_float4(s.x * inv_n, s.y * inv_n, s.z * inv_n, s.w * inv_n);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int p = p0 + l.row; p < p1; p += l.rows) {
            const float4 v = *reinterpret_cast<const float4*>(xp + (size_t)p * cstride);
            const float dx = v.x - mean.x, dy = v.y - mean.y, dz = v.z - mean.z, dw = v.w - mean.w;
            q = cg_add(q, make_float4(dx * dx, dy * dy, dz * dz, dw * dw));
        }
    q = bn_fold_rows(q, red, bcast, l, tg);
    if (live && l.row == 0) {
        *reinterpret_cast<float4*>(ws + (size_t)(2 * blockIdx.y) * C4 + l.c0) = mean;
        *reinterpret_cast<float4*>(ws + (size_t)(2 * blockIdx.y + 1) * C4 + l.c0) = q;
    }
}

// one wave per channel, four channels per workgroup
__global__ __launch_bounds__(CG_THREADS) void bn_stats_final_kernel(const float* __restrict__ ws, int slabs, int slab_px, int pixels, int C, int C4,
                                                                     float* __restrict__ b_mean, float* __restrict__ b_var,
                                                                     float* __restrict__ b_factor, float maf, float eps, float* __restrict__ save) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;      // (uniform over the wave)
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int s = lane; s < slabs; s += 64) {
        const float nb = (float)min(slab_px, pixels - s * slab_px);
        bn_chan(n, mean, m2, nb, ws[(size_t)(2 * s) * C4 + c], ws[(size_t)(2 * s + 1) * C4 + c]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const float nb = __shfl_down(n, off, 64), mb = __shfl_down(mean, off, 64), qb = __shfl_down(m2, off, 64);
        if (lane < off) bn_chan(n, mean, m2, nb, mb, qb);
    }
    if (lane != 0) return;
    const float m = (float)pixels;
    const float var = m2 / m;
    save[c] = mean;
    save[C + c] = 1.0f / sqrtf(var + eps);
    if (b_mean) {
        // Caffe's BatchNormLayer::Forward_cpu: the sums decay by the moving-average fraction, the variance enters unbiased
        const float corr = pixels > 1 ? m / (m - 1.0f) : 1.0f;
        b_mean[c] = b_mean[c] * maf + mean;
        b_var[c] = b_var[c] * maf + var * corr;
        if (c == 0) b_factor[0] = b_factor[0] * maf + 1.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- per-channel operands
struct BnOps {
    float mean, inv;
};

// mean / invstd of channel c: the save area, or the three blobs (global statistics), or (0, 1) for Scale alone
__device__ inline BnOps bn_channel(int c, int C, const float* save, const float* b_mean, const float* b_var, const float* b_factor, float eps) {
    BnOps o;
    o.mean = 0.f;
    o.inv = 1.f;
    if (save) {
        o.mean = save[c];
        o.inv = save[C + c];
    } else if (b_mean) {
        const float f = b_factor[0];
        const float sc = f == 0.f ? 0.f : 1.0f / f;
        o.mean = sc * b_mean[c];
        o.inv = 1.0f / sqrtf(sc * b_var[c] + eps);
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(CG_THREADS) void bn_apply_f32_kernel(const float* x, float* y, float* __restrict__ xhat, int pixels, int C, int xcs, int xco,
                                                                   int ycs, int yco, int hcs, const float* __restrict__ save,
                                                                   const float* __restrict__ b_mean, const float* __restrict__ b_var,
                                                                   const float* __restrict__ b_factor, float eps, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, int relu, int tg) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    const int c0 = l.c0, nv = l.nv;
    float mean[4], inv[4], ga[4], be[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mean[j] = 0.f; inv[j] = 1.f; ga[j] = 1.f; be[j] = 0.f;
        if (j < nv) {
            const BnOps o = bn_channel(c0 + j, C, save, b_mean, b_var, b_factor, eps);
            mean[j] = o.mean;
            inv[j] = o.inv;
            if (gamma) ga[j] = gamma[c0 + j];
            if (beta) be[j] = beta[c0 + j];
        }
    }
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        float v[4], h[4], o[4];
        cg_load(x + (size_t)p * xcs + xco + c0, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = (v[j] - mean[j]) * inv[j];
            o[j] = ga[j] * h[j] + be[j];
            if (relu) o[j] = o[j] > 0.f ? o[j] : 0.f;
        }
        cg_store(y + (size_t)p * ycs + yco + c0, o, nv);
        if (xhat) cg_store(xhat + (size_t)p * hcs + c0, h, nv);
    }
}

// halves in, halves out, float32 operands and arithmetic; a lane owns 8 channels.  With its 32 operand registers the kernel is the one
// here that the compiler would let grow past 64 VGPRs (74: 6 waves per SIMD); asked for 8 it needs 54, without scratch.
__global__ __launch_bounds__(CG_THREADS) __attribute__((amdgpu_waves_per_eu(8))) void bn_apply_f16_kernel(const __half* x, __half* y, int pixels, int C, int xcs, int xco, int ycs, int yco,
                                                                   const float* __restrict__ b_mean, const float* __restrict__ b_var,
                                                                   const float* __restrict__ b_factor, float eps, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, int relu, int tg) {
    const CgLane l = cg_lane<8>(tg, C);
    if (l.nv <= 0) return;
    const int c0 = l.c0, nv = l.nv;
    float mean[8], inv[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mean[j] = 0.f; inv[j] = 1.f; ga[j] = 1.f; be[j] = 0.f;
        if (j < nv) {
            const BnOps o = bn_channel(c0 + j, C, nullptr, b_mean, b_var, b_factor, eps);
            mean[j] = o.mean;
            inv[j] = o.inv;
            if (gamma) ga[j] = gamma[c0 + j];
            if (beta) be[j] = beta[c0 + j];
        }
    }
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        const CgH8 in = cg_load_h8(x + (size_t)p * xcs + xco + c0);
        CgH8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float o = ga[j] * ((__half2float(in.h[j]) - mean[j]) * inv[j]) + be[j];
            if (relu) o = o > 0.f ? o : 0.f;
            out.h[j] = __float2half_rn(o);
        }
        cg_store_h8(y + (size_t)p * ycs + yco + c0, out, nv);
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// grid (gx, slabs): workspace[(2 * slab + 0) * C4 + c] = sum dy', [(2 * slab + 1) * C4 + c] = sum dy' * xhat over the slab
__global__ __launch_bounds__(CG_THREADS) void bn_bwd_slab_kernel(const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ y,
                                                                  int pixels, int C, int dcs, int dco, int hcs, int hco, int ycs, int yco, int tg,
                                                                  int slab_px, float* __restrict__ ws, int C4) {
    __shared__ float4 red[CG_THREADS];
    __shared__ float4 bcast[16];
    const CgLane l = cg_lane<4>(tg, C);
    const bool live = l.nv > 0;
    const int c0 = l.c0;
    const int p0 = blockIdx.y * slab_px;
    const int p1 = min(pixels, p0 + slab_px);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live)
        for (int p = p0 + l.row; p < p1; p += l.rows) {
            float4 d = *reinterpret_cast<const float4*>(dy + (size_t)p * dcs + dco + c0);
            const float4 h = *reinterpret_cast<const float4*>(xhat + (size_t)p * hcs + hco + c0);
            if (y) {
                const float4 a = *reinterpret_cast<const float4*>(y + (size_t)p * ycs + yco + c0);
                d.x = a.x > 0.f ? d.x : 0.f; d.y = a.y > 0.f ? d.y : 0.f; d.z = a.z > 0.f ? d.z : 0.f; d.w = a.w > 0.f ? d.w : 0.f;
            }
            s = cg_add(s, d);
            t = cg_add(t, make_float4(d.x * h.x, d.y * h.y, d.z * h.z, d.w * h.w));
        }
    s = bn_fold_rows(s, red, bcast, l, tg);
    t = bn_fold_rows(t, red, bcast, l, tg);
    if (live && l.row == 0) {
        *reinterpret_cast<float4*>(ws + (size_t)(2 * blockIdx.y) * C4 + c0) = s;
        *reinterpret_cast<float4*>(ws + (size_t)(2 * blockIdx.y + 1) * C4 + c0) = t;
    }
}

__global__ __launch_bounds__(CG_THREADS) void bn_bwd_final_kernel(const float* __restrict__ ws, int slabs, int C, int C4, float* __restrict__ sum_dy,
                                                                   float* __restrict__ sum_dyx) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    float a[2];
    cg_fold_slabs(ws + c, slabs, C4, lane, a);
    if (lane == 0) {
        sum_dy[c] = a[0];
        sum_dyx[c] = a[1];
    }
}

__global__ __launch_bounds__(CG_THREADS) void bn_bwd_apply_kernel(const float* dy, const float* __restrict__ xhat, const float* __restrict__ y, float* dx,
                                                                   int pixels, int C, int dcs, int dco, int hcs, int hco, int ycs, int yco, int xcs,
                                                                   int xco, const float* __restrict__ save, const float* __restrict__ b_var,
                                                                   const float* __restrict__ b_factor, float eps, const float* __restrict__ gamma,
                                                                   const float* __restrict__ sum_dy, const float* __restrict__ sum_dyx,
                                                                   int accumulate, int tg) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    const int c0 = l.c0, nv = l.nv;
    const float inv_m = 1.0f / (float)pixels;
    float k[4], a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k[j] = 1.f; a[j] = 0.f; b[j] = 0.f;
        if (j < nv) {
            // (the mean is not needed here: b_var stands in for the mean blob so that the global-statistics branch is taken)
            const BnOps o = bn_channel(c0 + j, C, save, b_var, b_var, b_factor, eps);
            k[j] = (gamma ? gamma[c0 + j] : 1.f) * o.inv;
            if (sum_dy) {
                a[j] = sum_dy[c0 + j] * inv_m;
                b[j] = sum_dyx[c0 + j] * inv_m;
            }
        }
    }
    const bool centred = sum_dy != nullptr;
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        float d[4];
        cg_load(dy + (size_t)p * dcs + dco + c0, d);
        if (y) {
            float m[4];
            cg_load(y + (size_t)p * ycs + yco + c0, m);
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = m[j] > 0.f ? d[j] : 0.f;
        }
        float o[4];
        if (centred) {
            float h[4];
            cg_load(xhat + (size_t)p * hcs + hco + c0, h);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = k[j] * (d[j] - a[j] - h[j] * b[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = k[j] * d[j];
        }
        cg_store_acc(dx + (size_t)p * xcs + xco + c0, o, nv, accumulate);
    }
}

}  // namespace
}  // namespace fcn

using namespace fcn;

size_t fcn_batchnorm_workspace_bytes(int pixels, int C) {
    if (pixels <= 0 || C <= 0) return 0;
    const CgTile t = cg_tile(1, pixels, C, 4);
    return (size_t)t.slabs * 2 * ((C + 3) / 4 * 4) * sizeof(float);
}

int fcn_batchnorm_stats_f32(const float* x, int pixels, int C, int x_cstride, int x_coffset, float* blob_mean, float* blob_var,
                            float* blob_factor, float moving_average_fraction, float eps, float* save, void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(x && save && d_workspace, FCN_E_ARG, "batchnorm_stats: null x / save / workspace");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "batchnorm_stats: non-positive extent");
    FCN_REQUIRE((blob_mean != nullptr) == (blob_var != nullptr) && (blob_mean != nullptr) == (blob_factor != nullptr), FCN_E_ARG,
                "batchnorm_stats: the three blobs come together or not at all");
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset), FCN_E_ARG, "batchnorm_stats: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4), FCN_E_ALIGN, "batchnorm_stats: channel stride and offset must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, d_workspace) && ((uintptr_t)save & 3) == 0, FCN_E_ALIGN,
                "batchnorm_stats: x and the workspace must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    hipLaunchKernelGGL(bn_stats_slab_kernel, dim3(t.gx, t.slabs), dim3(CG_THREADS), 0, as_stream(s), x, pixels, C, x_cstride, x_coffset, t.tg,
                       t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("bn_stats_slab_kernel");
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 3) / 4), dim3(CG_THREADS), 0, as_stream(s), ws, t.slabs, t.slab_px, pixels, C, C4, blob_mean,
                       blob_var, blob_factor, moving_average_fraction, eps, save);
    FCN_LAUNCH_CHECK("bn_stats_final_kernel");
    return 0;
}

int fcn_batchnorm_apply_f32(const float* x, float* y, float* xhat, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                            int xhat_cstride, const float* save, const float* blob_mean, const float* blob_var, const float* blob_factor, float eps,
                            const float* gamma, const float* beta, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "batchnorm_apply: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "batchnorm_apply: non-positive extent");
    FCN_REQUIRE((blob_mean != nullptr) == (blob_var != nullptr) && (blob_mean != nullptr) == (blob_factor != nullptr), FCN_E_ARG,
                "batchnorm_apply: the three blobs come together or not at all");
    FCN_REQUIRE(!(save && blob_mean), FCN_E_ARG, "batchnorm_apply: statistics from the save area or from the blobs, not both");
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset) && (!xhat || xhat_cstride >= C), FCN_E_ARG,
                "batchnorm_apply: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4) && cg_view_ok(y_cstride, y_coffset, 4) && (!xhat || xhat_cstride % 4 == 0), FCN_E_ALIGN,
                "batchnorm_apply: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, y, xhat), FCN_E_ALIGN, "batchnorm_apply: x, y and xhat must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    hipLaunchKernelGGL(bn_apply_f32_kernel, dim3(t.gx, t.gy), dim3(CG_THREADS), 0, as_stream(s), x, y, xhat, pixels, C, x_cstride,
                       x_coffset, y_cstride, y_coffset, xhat_cstride, save, blob_mean, blob_var, blob_factor, eps, gamma, beta, relu, t.tg);
    FCN_LAUNCH_CHECK("bn_apply_f32_kernel");
    return 0;
}

int fcn_batchnorm_apply_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                            const float* blob_mean, const float* blob_var, const float* blob_factor, float eps, const float* gamma,
                            const float* beta, int relu, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "batchnorm_apply_f16: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "batchnorm_apply_f16: non-positive extent");
    FCN_REQUIRE((blob_mean != nullptr) == (blob_var != nullptr) && (blob_mean != nullptr) == (blob_factor != nullptr), FCN_E_ARG,
                "batchnorm_apply_f16: the three blobs come together or not at all");
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset), FCN_E_ARG,
                "batchnorm_apply_f16: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 8) && cg_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "batchnorm_apply_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE(cg_aligned16(x, y), FCN_E_ALIGN, "batchnorm_apply_f16: x and y must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 8);
    hipLaunchKernelGGL(bn_apply_f16_kernel, dim3(t.gx, t.gy), dim3(CG_THREADS), 0, as_stream(s), static_cast<const __half*>(x),
                       static_cast<__half*>(y), pixels, C, x_cstride, x_coffset, y_cstride, y_coffset, blob_mean, blob_var, blob_factor, eps, gamma,
                       beta, relu, t.tg);
    FCN_LAUNCH_CHECK("bn_apply_f16_kernel");
    return 0;
}

int fcn_batchnorm_bwd_reduce_f32(const float* dy, const float* xhat, const float* relu_y, int pixels, int C, int dy_cstride, int dy_coffset,
                                 int xhat_cstride, int xhat_coffset, int y_cstride, int y_coffset, float* sum_dy, float* sum_dyx,
                                 void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(dy && xhat && sum_dy && sum_dyx && d_workspace, FCN_E_ARG, "batchnorm_bwd_reduce: null pointer");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "batchnorm_bwd_reduce: non-positive extent");
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, xhat_cstride, xhat_coffset) &&
                    (!relu_y || cg_view_in(C, y_cstride, y_coffset)),
                FCN_E_ARG, "batchnorm_bwd_reduce: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(xhat_cstride, xhat_coffset, 4) &&
                    (!relu_y || cg_view_ok(y_cstride, y_coffset, 4)),
                FCN_E_ALIGN, "batchnorm_bwd_reduce: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, xhat, relu_y, d_workspace) && (((uintptr_t)sum_dy | (uintptr_t)sum_dyx) & 3) == 0,
                FCN_E_ALIGN, "batchnorm_bwd_reduce: dy, xhat, relu_y and the workspace must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    const int C4 = (C + 3) / 4 * 4;
    float* ws = static_cast<float*>(d_workspace);
    hipLaunchKernelGGL(bn_bwd_slab_kernel, dim3(t.gx, t.slabs), dim3(CG_THREADS), 0, as_stream(s), dy, xhat, relu_y, pixels, C, dy_cstride, dy_coffset,
                       xhat_cstride, xhat_coffset, y_cstride, y_coffset, t.tg, t.slab_px, ws, C4);
    FCN_LAUNCH_CHECK("bn_bwd_slab_kernel");
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 3) / 4), dim3(CG_THREADS), 0, as_stream(s), ws, t.slabs, C, C4, sum_dy, sum_dyx);
    FCN_LAUNCH_CHECK("bn_bwd_final_kernel");
    return 0;
}

int fcn_batchnorm_bwd_apply_f32(const float* dy, const float* xhat, const float* relu_y, float* dx, int pixels, int C, int dy_cstride,
                                int dy_coffset, int xhat_cstride, int xhat_coffset, int y_cstride, int y_coffset, int dx_cstride, int dx_coffset,
                                const float* save, const float* blob_var, const float* blob_factor, float eps, const float* gamma,
                                const float* sum_dy, const float* sum_dyx, int accumulate, fcn_stream_t s) {
    FCN_REQUIRE(dy && dx, FCN_E_ARG, "batchnorm_bwd_apply: null dy / dx");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "batchnorm_bwd_apply: non-positive extent");
    FCN_REQUIRE((sum_dy != nullptr) == (sum_dyx != nullptr) && (!sum_dy || xhat), FCN_E_ARG,
                "batchnorm_bwd_apply: the two sums come together, and with them xhat");
    FCN_REQUIRE((blob_var != nullptr) == (blob_factor != nullptr) && !(save && blob_var), FCN_E_ARG,
                "batchnorm_bwd_apply: invstd from the save area or from the variance and factor blobs, not both");
    FCN_REQUIRE(cg_view_in(C, dy_cstride, dy_coffset) && cg_view_in(C, dx_cstride, dx_coffset) &&
                    (!xhat || cg_view_in(C, xhat_cstride, xhat_coffset)) && (!relu_y || cg_view_in(C, y_cstride, y_coffset)),
                FCN_E_ARG, "batchnorm_bwd_apply: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(dy_cstride, dy_coffset, 4) && cg_view_ok(dx_cstride, dx_coffset, 4) &&
                    (!xhat || cg_view_ok(xhat_cstride, xhat_coffset, 4)) && (!relu_y || cg_view_ok(y_cstride, y_coffset, 4)),
                FCN_E_ALIGN, "batchnorm_bwd_apply: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(dy, xhat, relu_y, dx), FCN_E_ALIGN,
                "batchnorm_bwd_apply: dy, xhat, relu_y and dx must be 16-byte aligned");
    const CgTile t = cg_tile(1, pixels, C, 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(t.gx, t.gy), dim3(CG_THREADS), 0, as_stream(s), dy, xhat, relu_y, dx, pixels, C,
                       dy_cstride, dy_coffset, xhat_cstride, xhat_coffset, y_cstride, y_coffset, dx_cstride, dx_coffset, save, blob_var, blob_factor,
                       eps, gamma, sum_dy, sum_dyx, accumulate, t.tg);
    FCN_LAUNCH_CHECK("bn_bwd_apply_kernel");
    return 0;
}
