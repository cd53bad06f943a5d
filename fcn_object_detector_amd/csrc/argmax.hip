// ArgMax (Caffe's ArgMaxLayer over the channel axis) for gfx950, on its own and fused behind Interp and / or a Softmax.
//
// Order: Caffe sorts (value, index) pairs with std::greater, so rank 0 is the largest value and OF EQUAL VALUES THE LARGER INDEX COMES
// FIRST.  The pairs of a pixel are all different (the indices are), so the order is total: rank r is the largest pair below rank r - 1,
// found by one more walk over the pixel's channels - k walks for top_k = k, no per-lane array, and whatever order lanes or waves
// combine their partial results in, the maximum of a total order is one pair: the same bits every run, no atomics.  A NaN score
// compares false both ways and never takes a rank (a pixel with fewer than k comparable scores reports index -1 for the ranks left).
//
// Only channels x_coffset .. x_coffset + C - 1 enter the comparison.  A 16-byte load at the end of the window may bring pad channels
// or a neighbouring window's along (they lie inside the pixel's stride, so the load is in bounds); they are masked by channel number.
//
// Two launch shapes, both bandwidth-bound:
//   lane per pixel   a segmentation tail - few channels, many pixels.  A lane walks its pixel's 16-byte segments; consecutive lanes
//                    take consecutive pixels, so a wave's loads stay inside 64 neighbouring windows while those fit the L1.
//   wave per pixel   a classifier's rows - few pixels, many channels.  Lane l takes segments l, l + 64, ...; the 64 partial pairs
//                    meet in a butterfly of __shfl_xor steps (32, 16, .. 1), after which every lane holds the winner.
// The switch (use_wave below) is measured, tools/argmax_bench.py --sweep on an MI355X, top_k 1, microseconds per launch, float32 / half:
//     pixels   C     lane            wave                 pixels   C     lane            wave
//     263169   24    8.1 / 6.0       60.7 / 82.2          4096     24    3.8 / 3.8       3.6 / 3.6
//     263169   64    28.2 / 13.9     62.0 / 84.5          4096     32    5.0 / 4.5       3.6 / 3.6
//     263169   128   60.1 / 34.2     62.0 / 86.1          4096     64    8.1 / 7.9       3.6 / 3.6
//     263169   192   127.7 / 62.4    62.7 / 85.0          4096     256   27.2 / 26.2     3.6 / 3.6   (64 pixels: the same within 0.3)
// The lane form's time follows the bytes of a window (its wave strides over 64 windows: past 512 bytes each they no longer share
// cache lines in time); the wave form's follows the number of waves, and is the launch floor while every pixel's wave is resident
// at once (256 CUs x 32 waves = 8192).  So: a wave per pixel above FCN_ARGMAX_WAVE_BYTES per window, and for up to
// FCN_ARGMAX_WAVE_PIXELS pixels of at least FCN_ARGMAX_WAVE_MIN_C channels (below that the two tie at the launch floor).  Between
// 8192 pixels and a segmentation map's the crossing was not measured; the lane form keeps that ground.
//
// FCN_ARGMAX_SOFTMAX: x holds the scores in front of a Softmax that the caller fused away; the reported values are the
// probabilities exp(v - max) / sum exp(v' - max), the sum taken online beside the first walk (running maximum m, running sum s,
// rescaled when m moves; partial (m, s) of the wave form merge in the same butterfly).  Ranks are decided on the scores.
//
// The fused pass (fcn_interp_argmax_fwd_*) is a lane per OUTPUT pixel: it blends each channel from the four input pixels with the
// positions kept in integers - cell = num / (n2 - 1), weight = float(num % (n2 - 1)) / float(n2 - 1), num = o (n1 - 1), exactly
// interp_pos / blend of interp_common.h, in float32 without contraction - and keeps the best pair (and m, s) as it goes: the
// resampled map is never written.  top_k is 1.
#include "interp_common.h"

#include <limits.h>

using namespace fcn;

namespace {

inline bool use_wave(int pixels, int C, int esize) {
#ifdef FCN_EXP_ARGMAX_KERNEL      // elimination builds (Makefile `exp`, EXPSRC=argmax): 0 the lane form everywhere, 1 the wave form
    return FCN_EXP_ARGMAX_KERNEL != 0;
#else
    return (long long)C * esize > FCN_ARGMAX_WAVE_BYTES || (C >= FCN_ARGMAX_WAVE_MIN_C && pixels <= FCN_ARGMAX_WAVE_PIXELS);
#endif
}

constexpr int KNOWN_FLAGS = FCN_ARGMAX_VALUES | FCN_ARGMAX_PAIRS | FCN_ARGMAX_SOFTMAX;

struct ArgGeom {
    unsigned pixels;
    int C, top_k, flags;
    int x_cstride, x_coffset, y_cstride, y_coffset;
};

// std::greater<std::pair<float, int>>: (v, i) sorts in front of (w, j)
__device__ inline bool beats(float v, int i, float w, int j) { return v > w || (v == w && i > j); }

// the running softmax denominator: s = sum exp(v' - m) over the values seen, m their maximum
__device__ inline void online_add(float v, float& m, float& s) {
    if (v > m) {
        s = (m == -INFINITY ? 0.f : s * expf(m - v)) + 1.f;
        m = v;
    } else if (v == v) {      // (a NaN joins nothing)
        s += v == -INFINITY && m == -INFINITY ? 0.f : expf(v - m);
    }
}

// rank r of a pixel: index, or value, or both (PAIRS: the k indices, then the k values)
__device__ inline void write_rank(float* py, int r, int k, int flags, float bv, int bi, float m, float s) {
    const float val = (flags & FCN_ARGMAX_SOFTMAX) ? expf(bv - m) / s : bv;
    if (flags & FCN_ARGMAX_VALUES) {
        py[r] = val;
    } else {
        py[r] = (float)bi;
        if (flags & FCN_ARGMAX_PAIRS) py[k + r] = val;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void argmax_lane_kernel(const T* __restrict__ x, float* __restrict__ y, ArgGeom g) {
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    const bool soft = g.flags & FCN_ARGMAX_SOFTMAX;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < g.pixels; p += gridDim.x * blockDim.x) {
        const T* px = x + (size_t)p * g.x_cstride + g.x_coffset;
        float* py = y + (size_t)p * g.y_cstride + g.y_coffset;
        float pv = INFINITY, m = -INFINITY, s = 0.f;      // (pv, pi): the rank before; everything sorts behind (+inf, INT_MAX)
        int pi = INT_MAX;
        for (int r = 0; r < g.top_k; ++r) {
            float bv = -INFINITY;
            int bi = -1;
            for (int c0 = 0; c0 < g.C; c0 += E) {
                float v[E];
                load_seg<E>(px + c0, v);
                for (int e = 0; e < E; ++e) {
                    const int c = c0 + e;
                    if (c < g.C) {      // (pad channels and a neighbouring window's: loaded, never compared)
                        if (soft && r == 0) online_add(v[e], m, s);
                        if (beats(pv, pi, v[e], c) && beats(v[e], c, bv, bi)) bv = v[e], bi = c;
                    }
                }
            }
            write_rank(py, r, g.top_k, g.flags, bv, bi, m, s);
            pv = bv, pi = bi;
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void argmax_wave_kernel(const T* __restrict__ x, float* __restrict__ y, ArgGeom g) {
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    const bool soft = g.flags & FCN_ARGMAX_SOFTMAX;
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    for (unsigned p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < g.pixels; p += waves) {      // (uniform in a wave)
        const T* px = x + (size_t)p * g.x_cstride + g.x_coffset;
        float* py = y + (size_t)p * g.y_cstride + g.y_coffset;
        float pv = INFINITY, m = -INFINITY, s = 0.f;
        int pi = INT_MAX;
        for (int r = 0; r < g.top_k; ++r) {
            float bv = -INFINITY;
            int bi = -1;
            for (int c0 = lane * E; c0 < g.C; c0 += 64 * E) {
                float v[E];
                load_seg<E>(px + c0, v);
                for (int e = 0; e < E; ++e) {
                    const int c = c0 + e;
                    if (c < g.C) {      // (pad channels and a neighbouring window's: loaded, never compared)
                        if (soft && r == 0) online_add(v[e], m, s);
                        if (beats(pv, pi, v[e], c) && beats(v[e], c, bv, bi)) bv = v[e], bi = c;
                    }
                }
            }
            for (int d = 32; d >= 1; d >>= 1) {      // fixed order; both partners keep the same pair
                const float ov = __shfl_xor(bv, d, 64);
                const int oi = __shfl_xor(bi, d, 64);
                if (beats(ov, oi, bv, bi)) bv = ov, bi = oi;
            }
            if (soft && r == 0) {
                for (int d = 32; d >= 1; d >>= 1) {
                    const float om = __shfl_xor(m, d, 64), os = __shfl_xor(s, d, 64);
                    const float mm = fmaxf(m, om);
                    // (a + b on one partner is b + a on the other: the same bits in every lane)
                    const float a = m == -INFINITY ? 0.f : s * expf(m - mm), b = om == -INFINITY ? 0.f : os * expf(om - mm);
                    s = a + b;
                    m = mm;
                }
            }
            if (lane == 0) write_rank(py, r, g.top_k, g.flags, bv, bi, m, s);
            pv = bv, pi = bi;
        }
    }
}

// Interp + ArgMax (+ Softmax): one lane per output pixel
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void interp_argmax_kernel(const T* __restrict__ x, float* __restrict__ y, InterpGeom g, unsigned total, int flags) {
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    const bool soft = flags & FCN_ARGMAX_SOFTMAX;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const unsigned r = p / (unsigned)g.OW, ox = p - r * (unsigned)g.OW;
        const unsigned n = r / (unsigned)g.OH, oy = r - n * (unsigned)g.OH;
        int y0, y1, x0, x1;
        float ly, lx;
        interp_pos((int)oy, g.He, g.OH, y0, y1, ly);
        interp_pos((int)ox, g.We, g.OW, x0, x1, lx);
        const T* r0 = x + (((size_t)n * g.H + y0 + g.off) * g.W + g.off) * g.in_cstride + g.in_coffset;
        const T* r1 = x + (((size_t)n * g.H + y1 + g.off) * g.W + g.off) * g.in_cstride + g.in_coffset;
        const size_t a = (size_t)x0 * g.in_cstride, b = (size_t)x1 * g.in_cstride;
        float bv = -INFINITY, m = -INFINITY, s = 0.f;
        int bi = -1;
        for (int c0 = 0; c0 < g.C; c0 += E) {
            float p00[E], p01[E], p10[E], p11[E];
            load_seg<E>(r0 + a + c0, p00);
            load_seg<E>(r0 + b + c0, p01);
            load_seg<E>(r1 + a + c0, p10);
            load_seg<E>(r1 + b + c0, p11);
            for (int e = 0; e < E; ++e) {
                const int c = c0 + e;
                if (c < g.C) {
                    const float v = blend(p00[e], p01[e], p10[e], p11[e], lx, ly);
                    if (soft) online_add(v, m, s);
                    if (beats(v, c, bv, bi)) bv = v, bi = c;
                }
            }
        }
        write_rank(y + (size_t)p * g.out_cstride + g.out_coffset, 0, 1, flags, bv, bi, m, s);
    }
}

inline int out_channels(int top_k, int flags) { return (flags & FCN_ARGMAX_PAIRS) ? 2 * top_k : top_k; }

inline int flags_check(const char* who, int flags) {
    FCN_REQUIRE((flags & ~KNOWN_FLAGS) == 0, FCN_E_ARG, "%s: unknown flags 0x%x", who, flags);
    FCN_REQUIRE(!((flags & FCN_ARGMAX_VALUES) && (flags & FCN_ARGMAX_PAIRS)), FCN_E_ARG, "%s: FCN_ARGMAX_VALUES and FCN_ARGMAX_PAIRS exclude each other", who);
    return 0;
}

// half: x in whole 8-half segments and y in whole 4-float ones under 16-byte pointers, as fcn_interp_fwd_f16 with out_f32 asks;
// float32: 4-byte pointers, any stride (16-byte loads where the view allows)
template <typename T>
int argmax_fwd(const char* who, const T* x, float* y, int pixels, int C, int x_cstride, int x_coffset, int top_k, int y_cstride, int y_coffset,
               int flags, fcn_stream_t s) {
    constexpr bool half = sizeof(T) == 2;
    FCN_REQUIRE(x && y && pixels > 0 && C > 0, FCN_E_ARG, "%s: null pointer or non-positive extent", who);
    if (int rc = flags_check(who, flags)) return rc;
    FCN_REQUIRE(top_k >= 1 && top_k <= C, FCN_E_ARG, "%s: top_k %d is outside [1, %d]", who, top_k, C);
    FCN_REQUIRE(top_k <= FCN_ARGMAX_MAX_TOPK, FCN_E_UNSUPPORTED, "%s: top_k %d above %d", who, top_k, FCN_ARGMAX_MAX_TOPK);
    FCN_REQUIRE(x_coffset >= 0 && y_coffset >= 0 && x_cstride >= x_coffset + C && y_cstride >= y_coffset + out_channels(top_k, flags), FCN_E_ARG,
                "%s: slice out of range", who);
    if (half)
        FCN_REQUIRE(x_cstride % 8 == 0 && x_coffset % 8 == 0 && aligned16(x) && y_cstride % 4 == 0 && y_coffset % 4 == 0 && aligned16(y), FCN_E_ALIGN,
                    "%s: x stride and offset must be multiples of 8 halves, y's of 4 floats, the pointers of 16 bytes", who);
    FCN_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y) & 3u) == 0, FCN_E_ALIGN,
                "%s: pointers must be multiples of 4 bytes", who);
    const ArgGeom g{(unsigned)pixels, C, top_k, flags, x_cstride, x_coffset, y_cstride, y_coffset};
    const bool vec = half || (aligned16(x) && x_cstride % 4 == 0 && x_coffset % 4 == 0);
    const bool wave = use_wave(pixels, C, (int)sizeof(T));
    const dim3 grid(wave ? stream_grid((long long)pixels * 64, 256) : stream_grid(pixels, 256)), block(256);
#define FCN_ARGMAX_LAUNCH(K, V) hipLaunchKernelGGL((K<T, V>), grid, block, 0, as_stream(s), x, y, g)
    if (wave && vec) FCN_ARGMAX_LAUNCH(argmax_wave_kernel, true);
    else if (wave) FCN_ARGMAX_LAUNCH(argmax_wave_kernel, false);
    else if (vec) FCN_ARGMAX_LAUNCH(argmax_lane_kernel, true);
    else FCN_ARGMAX_LAUNCH(argmax_lane_kernel, false);
#undef FCN_ARGMAX_LAUNCH
    FCN_LAUNCH_CHECK(who);
    return 0;
}

template <typename T>
int interp_argmax_fwd(const char* who, const T* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                      int OH, int OW, int y_cstride, int y_coffset, int flags, fcn_stream_t s) {
    constexpr bool half = sizeof(T) == 2;
    if (int rc = flags_check(who, flags)) return rc;
    InterpGeom g;
    if (int rc = interp_check(who, x, y, N, H, W, C, x_cstride, x_coffset, pad_beg, pad_end, OH, OW, out_channels(1, flags), y_cstride, y_coffset,
                              half ? 8 : 0, half ? 4 : 0, &g))
        return rc;
    const long long total = (long long)N * OH * OW;
    FCN_REQUIRE(total < (1ll << 31), FCN_E_UNSUPPORTED, "%s: 2^31 output pixels or more", who);
    const bool vec = half || (aligned16(x) && x_cstride % 4 == 0 && x_coffset % 4 == 0);
    const dim3 grid(stream_grid(total, 256)), block(256);
    if (vec) hipLaunchKernelGGL((interp_argmax_kernel<T, true>), grid, block, 0, as_stream(s), x, y, g, (unsigned)total, flags);
    else hipLaunchKernelGGL((interp_argmax_kernel<T, false>), grid, block, 0, as_stream(s), x, y, g, (unsigned)total, flags);
    FCN_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" {

int fcn_argmax_fwd_f32(const float* x, float* y, int pixels, int C, int x_cstride, int x_coffset, int top_k, int y_cstride, int y_coffset,
                       int flags, fcn_stream_t s) {
    return argmax_fwd<float>("argmax_fwd", x, y, pixels, C, x_cstride, x_coffset, top_k, y_cstride, y_coffset, flags, s);
}

int fcn_argmax_fwd_f16(const void* x, float* y, int pixels, int C, int x_cstride, int x_coffset, int top_k, int y_cstride, int y_coffset,
                       int flags, fcn_stream_t s) {
    return argmax_fwd<_Float16>("argmax_fwd_f16", reinterpret_cast<const _Float16*>(x), y, pixels, C, x_cstride, x_coffset, top_k, y_cstride,
                                y_coffset, flags, s);
}

int fcn_interp_argmax_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                              int OH, int OW, int y_cstride, int y_coffset, int flags, fcn_stream_t s) {
    return interp_argmax_fwd<float>("interp_argmax_fwd", x, y, N, H, W, C, x_cstride, x_coffset, pad_beg, pad_end, OH, OW, y_cstride, y_coffset,
                                    flags, s);
}

int fcn_interp_argmax_fwd_f16(const void* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                              int OH, int OW, int y_cstride, int y_coffset, int flags, fcn_stream_t s) {
    return interp_argmax_fwd<_Float16>("interp_argmax_fwd_f16", reinterpret_cast<const _Float16*>(x), y, N, H, W, C, x_cstride, x_coffset, pad_beg,
                                       pad_end, OH, OW, y_cstride, y_coffset, flags, s);
}

}  // extern "C"
