// Upsample (the SegNet fork's UpsampleLayer: unpooling by the encoder's max-pooling indices) for gfx950, its adjoint, the half-float MAX
// pooling that writes those indices, and the read-back of the indices as Caffe's float mask.
//
// Layout as everywhere in this library: activations are NHWC views with a channel stride and a channel offset.  idx is the packed
// [N * PH * PW][C] int32 argmax that fcn_maxpool_fwd_f32 writes: iy * W + ix in the H x W plane of the pooling's bottom, the plane the
// Upsample writes.  x is the pooled-size blob (N x PH x PW), y the unpooled one (N x H x W).
//
// Forward is a GATHER over the output: a lane owns one 16-byte channel group of one pixel of y, walks the pooling windows that cover the
// pixel (ceil(k / stride)^2 of them: one for the 2 x 2 / stride 2 poolings of SegNet) in ascending (py, px) order and keeps x where idx
// names its own pixel.  A later window overwrites an earlier one - what Caffe's serial scatter leaves where overlapping windows share an
// argmax - and a lane that finds nothing stores zeros: one launch, no memset, no atomics, exactly one writer per element.  Only windows
// that cover a pixel are asked about it, so an index outside its own window (not an argmax of that window) is never followed.
//
// The kernels move bytes and do no arithmetic: floor = bytes(x + idx + y).  The (k / stride)^2 outputs under one window read the same
// idx and x vectors; neighbouring lanes of a workgroup do, so the repeats are cache hits.
#include "common.h"

using namespace fcn;

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

struct UnpoolGeom {
    int PH, PW, C, H, W, k, stride, pad;
    int x_cstride, x_coffset;      // the pooled-size view: x / dX
    int y_cstride, y_coffset;      // the unpooled view: y / dY
    int xv, iv, yv;                // whole 16-byte accesses are possible on x, idx, y
};

typedef float f4_t __attribute__((ext_vector_type(4)));
typedef int i4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

template <int E> __device__ inline void load_vec(const float* p, float* v) {
    const f4_t t = *reinterpret_cast<const f4_t*>(p);
    for (int e = 0; e < 4; ++e) v[e] = t[e];
}
template <int E> __device__ inline void load_vec(const _Float16* p, _Float16* v) {
    const h8_t t = *reinterpret_cast<const h8_t*>(p);
    for (int e = 0; e < 8; ++e) v[e] = t[e];
}
template <int E> __device__ inline void store_vec(float* p, const float* v) {
    for (int q = 0; q < E; q += 4) {      // (E = 8: the float32 output of a half segment is two 16-byte stores)
        const f4_t t = {v[q], v[q + 1], v[q + 2], v[q + 3]};
        *reinterpret_cast<f4_t*>(p + q) = t;
    }
}
template <int E> __device__ inline void store_vec(_Float16* p, const _Float16* v) {
    h8_t t;
    for (int e = 0; e < 8; ++e) t[e] = v[e];
    *reinterpret_cast<h8_t*>(p) = t;
}

// the indices of channels c .. c + cnt - 1 of pooled pixel p; -1 (no pixel) behind cnt
template <int E> __device__ inline void load_idx(const int32_t* ip, int cnt, bool vec, int* id) {
    if (vec && cnt == E) {
        for (int q = 0; q < E; q += 4) {
            const i4_t t = *reinterpret_cast<const i4_t*>(ip + q);
            for (int e = 0; e < 4; ++e) id[q + e] = t[e];
        }
    } else {
        for (int e = 0; e < E; ++e) id[e] = e < cnt ? ip[e] : -1;
    }
}

// first and last window index along one axis whose extent [p * stride - pad, p * stride - pad + k) holds o, clipped to [0, P)
__device__ inline void covering(int o, int k, int stride, int pad, int P, int& lo, int& hi) {
    const int a = o + pad - k + 1;
    lo = a <= 0 ? 0 : (a + stride - 1) / stride;
    hi = min((o + pad) / stride, P - 1);
}

// y[n, oy, ox, y_coffset + c] = x[n, py, px, x_coffset + c] of the last window (py, px) with idx[n, py, px, c] == oy * W + ox, else 0.
// TI: element type of x, E = 16 / sizeof(TI) channels per lane; TO: element type of y (half -> float32 is exact).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void unpool_fwd_kernel(const TI* __restrict__ x, const int32_t* __restrict__ idx, TO* __restrict__ y, UnpoolGeom g,
                                                         unsigned total) {
    constexpr int E = 16 / (int)sizeof(TI);
    const unsigned per = (unsigned)(g.C + E - 1) / E;
    // (32-bit lane arithmetic: the host refuses views of 2^31 elements, and there are fewer lanes than elements of y)
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned pix = t / per;
        const int c = (int)(t - pix * per) * E;
        const unsigned row = pix / (unsigned)g.W;
        const int ox = (int)(pix - row * (unsigned)g.W);
        const int n = (int)(row / (unsigned)g.H), oy = (int)(row - (unsigned)n * (unsigned)g.H);
        const int cnt = min(E, g.C - c), target = oy * g.W + ox;
        int ylo, yhi, xlo, xhi;
        covering(oy, g.k, g.stride, g.pad, g.PH, ylo, yhi);
        covering(ox, g.k, g.stride, g.pad, g.PW, xlo, xhi);
        TI v[E];
        for (int e = 0; e < E; ++e) v[e] = (TI)0;
        for (int py = ylo; py <= yhi; ++py)
            for (int px = xlo; px <= xhi; ++px) {
                const size_t p = ((size_t)n * g.PH + py) * g.PW + px;
                int id[E];
                load_idx<E>(idx + p * g.C + c, cnt, g.iv != 0, id);
                bool any = false;
                for (int e = 0; e < E; ++e) any |= id[e] == target;
                if (!any) continue;
                const TI* xp = x + p * g.x_cstride + g.x_coffset + c;
                TI xe[E];
                if (g.xv) {
                    load_vec<E>(xp, xe);      // (behind cnt: pad channels of the pixel, which id == -1 never selects)
                } else {
                    for (int e = 0; e < E; ++e) xe[e] = e < cnt ? xp[e] : (TI)0;
                }
                for (int e = 0; e < E; ++e) v[e] = id[e] == target ? xe[e] : v[e];
            }
        TO* yp = y + (size_t)pix * g.y_cstride + g.y_coffset + c;
        TO o[E];
        for (int e = 0; e < E; ++e) o[e] = (TO)v[e];
        if (g.yv && cnt == E) {
            store_vec<E>(yp, o);
        } else {
            for (int e = 0; e < cnt; ++e) yp[e] = o[e];
        }
    }
}

// dx[n, py, px, dx_coffset + c] (+)= dy[n, idx[n, py, px, c], dy_coffset + c]: a lane owns one 16-byte channel group of a dX pixel; every
// channel follows its own index (an index outside the plane - the -1 of a window without a maximum - contributes 0).
template <bool ACC>
__global__ __launch_bounds__(256) void unpool_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ idx, float* __restrict__ dx,
                                                         UnpoolGeom g, unsigned total) {
    constexpr int E = 4;
    const unsigned per = (unsigned)(g.C + E - 1) / E;
    const unsigned HW = (unsigned)g.H * (unsigned)g.W;
    const unsigned ppi = (unsigned)g.PH * (unsigned)g.PW;      // pooled pixels per image
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned pq = t / per;
        const int c = (int)(t - pq * per) * E;
        const size_t p = pq;
        const size_t n = pq / ppi;
        const int cnt = min(E, g.C - c);
        int id[E];
        load_idx<E>(idx + p * g.C + c, cnt, g.iv != 0, id);
        const float* dyn = dy + n * HW * g.y_cstride + g.y_coffset + c;
        float a[E];
        for (int e = 0; e < E; ++e) a[e] = (e < cnt && (unsigned)id[e] < HW) ? dyn[(size_t)id[e] * g.y_cstride + e] : 0.f;
        float* dp = dx + p * g.x_cstride + g.x_coffset + c;
        if (g.xv && cnt == E) {
            if (ACC) {
                float old[E];
                load_vec<E>(dp, old);
                for (int e = 0; e < E; ++e) a[e] = old[e] + a[e];
            }
            store_vec<E>(dp, a);
        } else {
            for (int e = 0; e < cnt; ++e) dp[e] = ACC ? dp[e] + a[e] : a[e];
        }
    }
}

// MAX pooling of halves with the argmax: the rule of maxpool_kernel (window clipped to the image, strict '>' so the first maximum in
// raster order stays, -1 where nothing in the window exceeds the lowest finite half).  One lane = 8 channels of one output pixel.
__global__ __launch_bounds__(256) void maxpool_idx_f16_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int32_t* __restrict__ idx,
                                                              int N, int H, int W, int C, int x_cstride, int k, int stride, int pad, int OH, int OW,
                                                              int y_cstride, int y_coffset) {
    const int cg = C / 8;
    const long long total = (long long)N * OH * OW * cg;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int grp = (int)(t % cg);
        const long long pix = t / cg;
        const int ox = (int)(pix % OW);
        const long long row = pix / OW;
        const int oy = (int)(row % OH), n = (int)(row / OH);
        int hs = oy * stride - pad, ws = ox * stride - pad;
        const int he = min(hs + k, H), we = min(ws + k, W);
        hs = max(hs, 0);
        ws = max(ws, 0);
        const _Float16* xb = x + (size_t)n * H * W * x_cstride + grp * 8;
        h8_t m;
        int mi[8];
        for (int e = 0; e < 8; ++e) {
            m[e] = (_Float16)-65504.f;
            mi[e] = -1;
        }
        for (int iy = hs; iy < he; ++iy)
            for (int ix = ws; ix < we; ++ix) {
                const int id = iy * W + ix;
                const h8_t v = *reinterpret_cast<const h8_t*>(xb + (size_t)id * x_cstride);
                for (int e = 0; e < 8; ++e)
                    if (v[e] > m[e]) { m[e] = v[e]; mi[e] = id; }
            }
        *reinterpret_cast<h8_t*>(y + (size_t)pix * y_cstride + y_coffset + grp * 8) = m;
        int32_t* ip = idx + (size_t)pix * C + grp * 8;
        for (int q = 0; q < 8; q += 4) {
            const i4_t o = {mi[q], mi[q + 1], mi[q + 2], mi[q + 3]};
            *reinterpret_cast<i4_t*>(ip + q) = o;
        }
    }
}

// dst (NCHW float32) = idx (packed NHWC int32): one lane per element of dst
__global__ __launch_bounds__(256) void mask_to_nchw_kernel(const int32_t* __restrict__ idx, float* __restrict__ dst, int PHW, int C, long long total) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(t % PHW);
        const long long nc = t / PHW;
        const int c = (int)(nc % C);
        const long long n = nc / C;
        dst[t] = (float)idx[((size_t)n * PHW + p) * C + c];
    }
}

// Caffe's pooled extent: ceil mode, and the last window must start inside the image or the left padding
inline long long pooled_extent(int h, int k, int s, int p) {
    const long long span = (long long)h + 2ll * p - k;
    long long o = (span >= 0 ? (span + s - 1) / s : -((-span) / s)) + 1;
    if (p > 0 && (o - 1) * s >= (long long)h + p) --o;
    return o;
}

// The checks the Upsample entry points share; every one precedes the first HIP call.  small / large: the pooled-size and the unpooled view.
int unpool_check(const char* who, const void* small, const void* idx, const void* large, int N, int PH, int PW, int C, int s_cstride,
                 int s_coffset, int k, int stride, int pad, int H, int W, int l_cstride, int l_coffset, UnpoolGeom* g) {
    FCN_REQUIRE(small && idx && large, FCN_E_ARG, "%s: null pointer", who);
    FCN_REQUIRE(N > 0 && PH > 0 && PW > 0 && C > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0 && pad < k, FCN_E_ARG,
                "%s: non-positive extent, kernel or stride, or a pad outside [0, kernel)", who);
    FCN_REQUIRE(PH == pooled_extent(H, k, stride, pad) && PW == pooled_extent(W, k, stride, pad), FCN_E_ARG,
                "%s: %d x %d is not the pooled extent of %d x %d under kernel %d stride %d pad %d (%lld x %lld)", who, PH, PW, H, W, k, stride, pad,
                pooled_extent(H, k, stride, pad), pooled_extent(W, k, stride, pad));
    FCN_REQUIRE(s_coffset >= 0 && l_coffset >= 0 && s_cstride >= s_coffset + C && l_cstride >= l_coffset + C, FCN_E_ARG, "%s: slice out of range", who);
    FCN_REQUIRE(aligned4(idx), FCN_E_ALIGN, "%s: idx must be a multiple of 4 bytes", who);
    const long long lim = 1ll << 31;
    const long long sp = (long long)N * PH * PW, lp = (long long)N * H * W;
    FCN_REQUIRE(sp * s_cstride < lim && lp * l_cstride < lim && sp * C < lim && (long long)H * W < lim, FCN_E_UNSUPPORTED,
                "%s: a view past 2^31 elements", who);
    *g = UnpoolGeom{PH, PW, C, H, W, k, stride, pad, s_cstride, s_coffset, l_cstride, l_coffset, 0, C % 4 == 0 && aligned16(idx) ? 1 : 0, 0};
    return 0;
}

inline int whole(const void* p, int cstride, int coffset, int e) { return aligned16(p) && cstride % e == 0 && coffset % e == 0 ? 1 : 0; }

template <typename TI, typename TO>
int unpool_fwd(const char* who, const TI* x, const int32_t* idx, TO* y, const UnpoolGeom& g, int N, fcn_stream_t s) {
    constexpr int E = 16 / (int)sizeof(TI);
    const long long total = (long long)N * g.H * g.W * ((g.C + E - 1) / E);
    hipLaunchKernelGGL((unpool_fwd_kernel<TI, TO>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), x, idx, y, g, (unsigned)total);
    FCN_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" {

int fcn_unpool_fwd_f32(const float* x, const int32_t* idx, float* y, int N, int PH, int PW, int C, int x_cstride, int x_coffset, int k, int stride,
                       int pad, int H, int W, int y_cstride, int y_coffset, fcn_stream_t s) {
    UnpoolGeom g;
    if (int rc = unpool_check("unpool_fwd", x, idx, y, N, PH, PW, C, x_cstride, x_coffset, k, stride, pad, H, W, y_cstride, y_coffset, &g)) return rc;
    FCN_REQUIRE(aligned4(x) && aligned4(y), FCN_E_ALIGN, "unpool_fwd: pointers must be multiples of 4 bytes");
    g.xv = whole(x, x_cstride, x_coffset, 4);
    g.yv = whole(y, y_cstride, y_coffset, 4);
    return unpool_fwd<float, float>("unpool_fwd", x, idx, y, g, N, s);
}

int fcn_unpool_fwd_f16(const void* x, const int32_t* idx, void* y, int N, int PH, int PW, int C, int x_cstride, int x_coffset, int k, int stride,
                       int pad, int H, int W, int y_cstride, int y_coffset, int out_f32, fcn_stream_t s) {
    UnpoolGeom g;
    FCN_REQUIRE(out_f32 == 0 || out_f32 == 1, FCN_E_ARG, "unpool_fwd_f16: out_f32 must be 0 or 1");
    if (int rc = unpool_check("unpool_fwd_f16", x, idx, y, N, PH, PW, C, x_cstride, x_coffset, k, stride, pad, H, W, y_cstride, y_coffset, &g)) return rc;
    FCN_REQUIRE(whole(x, x_cstride, x_coffset, 8), FCN_E_ALIGN, "unpool_fwd_f16: x must be 16-byte aligned, its stride and offset multiples of 8 halves");
    g.xv = 1;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x);
    if (out_f32) {
        FCN_REQUIRE(aligned4(y), FCN_E_ALIGN, "unpool_fwd_f16: a float32 y must be a multiple of 4 bytes");
        g.yv = whole(y, y_cstride, y_coffset, 4);
        return unpool_fwd<_Float16, float>("unpool_fwd_f16", xh, idx, reinterpret_cast<float*>(y), g, N, s);
    }
    FCN_REQUIRE(whole(y, y_cstride, y_coffset, 8), FCN_E_ALIGN, "unpool_fwd_f16: a half y must be 16-byte aligned, its stride and offset multiples of 8 halves");
    g.yv = 1;
    return unpool_fwd<_Float16, _Float16>("unpool_fwd_f16", xh, idx, reinterpret_cast<_Float16*>(y), g, N, s);
}

int fcn_unpool_bwd_f32(const float* dy, const int32_t* idx, float* dx, int N, int PH, int PW, int C, int dx_cstride, int dx_coffset, int k, int stride,
                       int pad, int H, int W, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s) {
    UnpoolGeom g;
    FCN_REQUIRE(accumulate == 0 || accumulate == 1, FCN_E_ARG, "unpool_bwd: accumulate must be 0 or 1");
    if (int rc = unpool_check("unpool_bwd", dx, idx, dy, N, PH, PW, C, dx_cstride, dx_coffset, k, stride, pad, H, W, dy_cstride, dy_coffset, &g)) return rc;
    FCN_REQUIRE(aligned4(dx) && aligned4(dy), FCN_E_ALIGN, "unpool_bwd: pointers must be multiples of 4 bytes");
    g.xv = whole(dx, dx_cstride, dx_coffset, 4);
    const long long total = (long long)N * PH * PW * ((C + 3) / 4);
    const dim3 grid(stream_grid(total, 256)), block(256);
    if (accumulate) hipLaunchKernelGGL(unpool_bwd_kernel<true>, grid, block, 0, as_stream(s), dy, idx, dx, g, (unsigned)total);
    else hipLaunchKernelGGL(unpool_bwd_kernel<false>, grid, block, 0, as_stream(s), dy, idx, dx, g, (unsigned)total);
    FCN_LAUNCH_CHECK("unpool_bwd");
    return 0;
}

int fcn_maxpool_idx_fwd_f16(const void* x, void* y, int32_t* idx, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad, int OH, int OW,
                            int y_cstride, int y_coffset, fcn_stream_t s) {
    FCN_REQUIRE(x && y && idx && N > 0 && H > 0 && W > 0 && C > 0 && k > 0 && stride > 0 && pad >= 0 && pad < k && OH > 0 && OW > 0, FCN_E_ARG,
                "maxpool_idx_f16: bad args");
    FCN_REQUIRE(OH == pooled_extent(H, k, stride, pad) && OW == pooled_extent(W, k, stride, pad), FCN_E_ARG,
                "maxpool_idx_f16: %d x %d is not the pooled extent of %d x %d under kernel %d stride %d pad %d", OH, OW, H, W, k, stride, pad);
    FCN_REQUIRE(x_cstride >= C && y_coffset >= 0 && y_cstride >= y_coffset + C, FCN_E_ARG, "maxpool_idx_f16: channel slice out of range");
    FCN_REQUIRE(C % 8 == 0 && x_cstride % 8 == 0 && y_cstride % 8 == 0 && y_coffset % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(idx), FCN_E_ALIGN,
                "maxpool_idx_f16: channels / strides must be multiples of 8, the pointers of 16 bytes");
    const long long lim = 1ll << 31;
    FCN_REQUIRE((long long)N * H * W * x_cstride < lim && (long long)N * OH * OW * y_cstride < lim && (long long)N * OH * OW * C < lim, FCN_E_UNSUPPORTED,
                "maxpool_idx_f16: a view past 2^31 elements");
    hipLaunchKernelGGL(maxpool_idx_f16_kernel, dim3(stream_grid((long long)N * OH * OW * (C / 8), 256)), dim3(256), 0, as_stream(s),
                       reinterpret_cast<const _Float16*>(x), reinterpret_cast<_Float16*>(y), idx, N, H, W, C, x_cstride, k, stride, pad, OH, OW, y_cstride,
                       y_coffset);
    FCN_LAUNCH_CHECK("maxpool_idx_f16");
    return 0;
}

int fcn_pool_mask_to_nchw_f32(const int32_t* idx, float* dst, int N, int PH, int PW, int C, fcn_stream_t s) {
    FCN_REQUIRE(idx && dst && N > 0 && PH > 0 && PW > 0 && C > 0, FCN_E_ARG, "pool_mask_to_nchw: null pointer or non-positive extent");
    FCN_REQUIRE(aligned4(idx) && aligned4(dst), FCN_E_ALIGN, "pool_mask_to_nchw: pointers must be multiples of 4 bytes");
    const long long total = (long long)N * PH * PW * C;
    FCN_REQUIRE(total < (1ll << 31), FCN_E_UNSUPPORTED, "pool_mask_to_nchw: a view past 2^31 elements");
    hipLaunchKernelGGL(mask_to_nchw_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), idx, dst, PH * PW, C, total);
    FCN_LAUNCH_CHECK("pool_mask_to_nchw");
    return 0;
}

}  // extern "C"
