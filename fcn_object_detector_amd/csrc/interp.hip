// Interp (DeepLab-Caffe's InterpLayer) for gfx950: bilinear resampling with aligned corners between two NHWC views with channel
// strides, and its adjoint.
//
// The DeepLab test / deploy nets upsample their stride-8 score map with it (fc8_interp, zoom_factor 8), the v2 training nets shrink the
// label (label_shrink, shrink_factor 8), and the pyramid-pooling heads resize their pooled branches back to the feature map.  Output
// index o of n2 lies at input position o (n1 - 1) / (n2 - 1) of the effective input (the bottom with -pad_beg rows / columns cropped
// in front and -pad_end behind); the position is kept in integers - cell i0 = num / (n2 - 1), weight lam = (num % (n2 - 1)) / (n2 - 1)
// with num = o (n1 - 1) - so the cell is exact and the weight is one correctly rounded division.  A weight of zero selects the pixel
// itself: equal extents copy bit for bit, and so does every output that falls on an input pixel (label_shrink keeps its 255s).
//
// Layout as in crop.hip: a lane moves one 16-byte channel segment, consecutive lanes run along the channels of a pixel and then along
// x.  One workgroup walks one output row (forward) or one row of dX (backward): the row's own position is uniform, what a lane computes
// is its column's.  All offsets are 64-bit: a batch of 513 x 513 x 24 floats passes 2^31 bytes.  The backward pass is a gather with a
// fixed order of summation (ascending output row, ascending output column inside a row): no atomics, no memset, the same bits every run.
#include "interp_common.h"

using namespace fcn;

namespace {

// the outputs [lo, hi) of n2 whose cell is j - 1 or j: all that can feed input index j of n1
__device__ inline void interp_feeders(int j, int n1, int n2, int& lo, int& hi) {
    if (n1 == 1) {
        lo = 0, hi = n2;
    } else if (n2 == 1) {
        lo = 0, hi = j == 0 ? 1 : 0;
    } else {
        const unsigned d1 = (unsigned)(n1 - 1), d2 = (unsigned)(n2 - 1);      // cell(o) == k  <=>  k d2 <= o d1 < (k + 1) d2
        lo = (int)(((unsigned)max(j - 1, 0) * d2 + d1 - 1) / d1);
        hi = min((int)(((unsigned)(j + 1) * d2 + d1 - 1) / d1), n2);
    }
}

template <int E> __device__ inline void store_seg(float* p, const float* v) {
    typedef float V __attribute__((ext_vector_type(4)));
    if (E == 1) {
        *p = v[0];
    } else {
        for (int q = 0; q < E; q += 4) {      // (E = 8: the float32 output of a half segment is two 16-byte stores)
            const V t = {v[q], v[q + 1], v[q + 2], v[q + 3]};
            *reinterpret_cast<V*>(p + q) = t;
        }
    }
}
template <int E> __device__ inline void store_seg(_Float16* p, const float* v) {
    if (E == 1) {
        *p = (_Float16)v[0];
    } else {
        typedef _Float16 V __attribute__((ext_vector_type(8)));
        V t;
        for (int e = 0; e < 8; ++e) t[e] = (_Float16)v[e];
        *reinterpret_cast<V*>(p) = t;
    }
}

// y[n, oy, ox, out_coffset + c] = the blend of the four pixels around (oy, ox)'s position, c < C.  VEC: a lane takes a whole 16-byte
// segment of the input's elements, the last C % E channels one by one (only they are read and written); otherwise one lane per element.
template <typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(256) void interp_fwd_kernel(const TI* __restrict__ x, TO* __restrict__ y, InterpGeom g, unsigned rows) {
    constexpr int E = VEC ? 16 / (int)sizeof(TI) : 1;
    const unsigned per = (unsigned)(g.C + E - 1) / E, row = (unsigned)g.OW * per;
    for (unsigned r = blockIdx.x; r < rows; r += gridDim.x) {
        const unsigned n = r / (unsigned)g.OH, oy = r - n * (unsigned)g.OH;
        int y0, y1;
        float ly;
        interp_pos((int)oy, g.He, g.OH, y0, y1, ly);
        const TI* r0 = x + (((size_t)n * g.H + y0 + g.off) * g.W + g.off) * g.in_cstride + g.in_coffset;
        const TI* r1 = x + (((size_t)n * g.H + y1 + g.off) * g.W + g.off) * g.in_cstride + g.in_coffset;
        TO* yr = y + (size_t)r * g.OW * g.out_cstride + g.out_coffset;
        for (unsigned t = threadIdx.x; t < row; t += blockDim.x) {
            const unsigned ox = t / per, c = (t - ox * per) * E;
            int x0, x1;
            float lx;
            interp_pos((int)ox, g.We, g.OW, x0, x1, lx);
            const size_t a = (size_t)x0 * g.in_cstride + c, b = (size_t)x1 * g.in_cstride + c;
            TO* dp = yr + (size_t)ox * g.out_cstride + c;
            if (VEC && (int)c + E <= g.C) {
                float p00[E], p01[E], p10[E], p11[E], v[E];
                load_seg<E>(r0 + a, p00);
                load_seg<E>(r0 + b, p01);
                load_seg<E>(r1 + a, p10);
                load_seg<E>(r1 + b, p11);
                for (int e = 0; e < E; ++e) v[e] = blend(p00[e], p01[e], p10[e], p11[e], lx, ly);
                store_seg<E>(dp, v);
            } else {
                for (int e = 0; e < E && (int)c + e < g.C; ++e)
                    dp[e] = (TO)blend((float)r0[a + e], (float)r0[b + e], (float)r1[a + e], (float)r1[b + e], lx, ly);
            }
        }
    }
}

// The adjoint, one lane per channel segment of a dX pixel: input row j is fed by the run of output rows whose cell is j - 1 (weight ly,
// where it is not zero) and by the run whose cell is j (weight 1 - ly); columns alike.  A row's columns are summed first, ascending, then
// the rows, ascending.  ACC = false: every pixel of dX's channel window is written - zero where nothing feeds it (cropped away, or
// skipped by a shrink).  ACC = true: dX += the sum where something feeds the pixel; nothing else is touched.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(256) void interp_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, InterpGeom g, unsigned rows) {
    constexpr int E = VEC ? 4 : 1;
    const unsigned per = (unsigned)(g.C + E - 1) / E, row = (unsigned)g.W * per;
    for (unsigned r = blockIdx.x; r < rows; r += gridDim.x) {
        const unsigned n = r / (unsigned)g.H;
        const int j = (int)(r - n * (unsigned)g.H) - g.off;
        int olo = 0, ohi = 0;
        if (j >= 0 && j < g.He) interp_feeders(j, g.He, g.OH, olo, ohi);
        const float* dyn = dy + (size_t)n * g.OH * g.OW * g.out_cstride + g.out_coffset;
        for (unsigned t = threadIdx.x; t < row; t += blockDim.x) {
            const unsigned ix = t / per, c = (t - ix * per) * E;
            const int i = (int)ix - g.off;
            int plo = 0, phi = 0;
            if (olo < ohi && i >= 0 && i < g.We) interp_feeders(i, g.We, g.OW, plo, phi);
            const int cnt = VEC ? min(E, g.C - (int)c) : 1;
            float acc[E];
            for (int e = 0; e < E; ++e) acc[e] = 0.f;
            bool fed = false;
            for (int oy = olo; oy < ohi; ++oy) {
                int y0, y1;
                float ly;
                interp_pos(oy, g.He, g.OH, y0, y1, ly);
                const float wy = y0 == j ? 1.f - ly : ly;
                if (wy == 0.f) continue;
                const float* dr = dyn + (size_t)oy * g.OW * g.out_cstride + c;
                float sum[E];
                for (int e = 0; e < E; ++e) sum[e] = 0.f;
                bool any = false;
                for (int ox = plo; ox < phi; ++ox) {
                    int x0, x1;
                    float lx;
                    interp_pos(ox, g.We, g.OW, x0, x1, lx);
                    const float wx = x0 == i ? 1.f - lx : lx;
                    if (wx == 0.f) continue;
                    const float* sp = dr + (size_t)ox * g.out_cstride;
                    float v[E];
                    if (cnt == E) {
                        load_seg<E>(sp, v);
                    } else {
                        for (int e = 0; e < E; ++e) v[e] = e < cnt ? sp[e] : 0.f;
                    }
                    for (int e = 0; e < E; ++e) sum[e] += wx * v[e];
                    any = true;
                }
                if (any) {
                    for (int e = 0; e < E; ++e) acc[e] += wy * sum[e];
                    fed = true;
                }
            }
            float* dp = dx + ((size_t)r * g.W + ix) * g.in_cstride + g.in_coffset + c;
            if (ACC && !fed) continue;
            if (cnt == E) {
                if (ACC) {
                    float old[E];
                    load_seg<E>(dp, old);
                    for (int e = 0; e < E; ++e) acc[e] = old[e] + acc[e];
                }
                store_seg<E>(dp, acc);
            } else {
                for (int e = 0; e < cnt; ++e) dp[e] = ACC ? dp[e] + acc[e] : acc[e];
            }
        }
    }
}

inline int row_grid(long long rows) { return (int)(rows < 65536 ? rows : 65536); }

template <typename TI, typename TO, bool VEC>
int interp_fwd(const char* who, const TI* x, TO* y, const InterpGeom& g, int N, fcn_stream_t s) {
    const long long rows = (long long)N * g.OH;
    hipLaunchKernelGGL((interp_fwd_kernel<TI, TO, VEC>), dim3(row_grid(rows)), dim3(256), 0, as_stream(s), x, y, g, (unsigned)rows);
    FCN_LAUNCH_CHECK(who);
    return 0;
}

inline bool whole_segments_f32(const void* a, const void* b, const InterpGeom& g) {
    return aligned16(a) && aligned16(b) && g.in_cstride % 4 == 0 && g.in_coffset % 4 == 0 && g.out_cstride % 4 == 0 && g.out_coffset % 4 == 0;
}

}  // namespace

extern "C" {

int fcn_interp_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end, int OH,
                       int OW, int y_cstride, int y_coffset, fcn_stream_t s) {
    InterpGeom g;
    if (int rc = interp_check("interp_fwd", x, y, N, H, W, C, x_cstride, x_coffset, pad_beg, pad_end, OH, OW, C, y_cstride, y_coffset, 0, 0, &g)) return rc;
    if (whole_segments_f32(x, y, g)) return interp_fwd<float, float, true>("interp_fwd", x, y, g, N, s);
    return interp_fwd<float, float, false>("interp_fwd", x, y, g, N, s);
}

int fcn_interp_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end, int OH,
                       int OW, int y_cstride, int y_coffset, int out_f32, fcn_stream_t s) {
    InterpGeom g;
    FCN_REQUIRE(out_f32 == 0 || out_f32 == 1, FCN_E_ARG, "interp_fwd_f16: out_f32 must be 0 or 1");
    if (int rc = interp_check("interp_fwd_f16", x, y, N, H, W, C, x_cstride, x_coffset, pad_beg, pad_end, OH, OW, C, y_cstride, y_coffset, 8,
                              out_f32 ? 4 : 8, &g))
        return rc;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x);
    if (out_f32) return interp_fwd<_Float16, float, true>("interp_fwd_f16", xh, reinterpret_cast<float*>(y), g, N, s);
    return interp_fwd<_Float16, _Float16, true>("interp_fwd_f16", xh, reinterpret_cast<_Float16*>(y), g, N, s);
}

int fcn_interp_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset, int pad_beg, int pad_end, int OH,
                       int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s) {
    InterpGeom g;
    if (int rc = interp_check("interp_bwd", dx, dy, N, H, W, C, dx_cstride, dx_coffset, pad_beg, pad_end, OH, OW, C, dy_cstride, dy_coffset, 0, 0, &g)) return rc;
    FCN_REQUIRE(accumulate == 0 || accumulate == 1, FCN_E_ARG, "interp_bwd: accumulate must be 0 or 1");
    const bool vec = whole_segments_f32(dx, dy, g);
    const long long rows = (long long)N * H;
    const dim3 grid(row_grid(rows)), block(256);
#define FCN_INTERP_BWD(VEC, ACC) hipLaunchKernelGGL((interp_bwd_kernel<VEC, ACC>), grid, block, 0, as_stream(s), dy, dx, g, (unsigned)rows)
    if (vec && accumulate) FCN_INTERP_BWD(true, true);
    else if (vec) FCN_INTERP_BWD(true, false);
    else if (accumulate) FCN_INTERP_BWD(false, true);
    else FCN_INTERP_BWD(false, false);
#undef FCN_INTERP_BWD
    FCN_LAUNCH_CHECK("interp_bwd");
    return 0;
}

}  // extern "C"
