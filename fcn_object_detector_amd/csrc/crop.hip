// Crop (Caffe CropLayer) for gfx950: a window copy between two NHWC views with channel strides, and its adjoint.
//
// The published FCN-32s / 16s / 8s nets align their skip connections and their final score map with it
// (score_pool4c = Crop(score_pool4, upscore2), score = Crop(upscore, data)).  Both directions are pure bandwidth: one pass,
// a lane moves 16 bytes (4 floats / 8 halves), consecutive lanes run along the channels of a pixel and then along x, so a
// wave touches contiguous bytes of both views; rows start at arbitrary pixels, and a pixel is cstride elements = a multiple
// of 16 bytes, which keeps every lane aligned.  No memset in front of the backward pass and no atomics: every element of dX
// has exactly one writer.
#include "common.h"

using namespace fcn;

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct Vec16<_Float16> { typedef _Float16 type __attribute__((ext_vector_type(8))); };

struct CropGeom {
    int H, W, OH, OW, off_y, off_x, C;
    int big_cstride, big_coffset;        // the uncropped view (x / dX)
    int win_cstride, win_coffset;        // the window-sized view (y / dY)
};

// y[n, oy, ox, win_coffset + c] = x[n, oy + off_y, ox + off_x, big_coffset + c].  VEC: both channel offsets are multiples of the
// 16-byte group - whole groups move as 16 bytes, the last C % E channels one by one (only they are read); otherwise one lane
// per element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void crop_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, CropGeom g, unsigned total) {
    typedef typename Vec16<T>::type V;
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    const unsigned per = (unsigned)(g.C + E - 1) / E, row = (unsigned)g.OW * per;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned r = t / row, in_row = t - r * row;
        const unsigned ox = in_row / per, c = (in_row - ox * per) * E;
        const unsigned n = r / (unsigned)g.OH, oy = r - n * (unsigned)g.OH;
        const T* sp = x + ((size_t)(n * g.H + oy + g.off_y) * g.W + ox + g.off_x) * g.big_cstride + g.big_coffset + c;
        T* dp = y + ((size_t)r * g.OW + ox) * g.win_cstride + g.win_coffset + c;
        if (!VEC) {
            *dp = *sp;
        } else if ((int)c + E <= g.C) {
            *reinterpret_cast<V*>(dp) = *reinterpret_cast<const V*>(sp);
        } else {
            for (int e = 0; (int)c + e < g.C; ++e) dp[e] = sp[e];
        }
    }
}

// The same window, read as halves and written as float32 (exact): the final score map of a half-float FCN net.  VEC: x_coffset is a
// multiple of 8 and y_coffset of 4 - a lane reads 16 bytes (8 halves) and writes 2 x 16 bytes; the last C % 8 channels one by one.
template <bool VEC>
__global__ __launch_bounds__(256) void crop_fwd_f16_f32_kernel(const _Float16* __restrict__ x, float* __restrict__ y, CropGeom g, unsigned total) {
    typedef Vec16<_Float16>::type VH;
    typedef Vec16<float>::type VF;
    constexpr int E = VEC ? 8 : 1;
    const unsigned per = (unsigned)(g.C + E - 1) / E, row = (unsigned)g.OW * per;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned r = t / row, in_row = t - r * row;
        const unsigned ox = in_row / per, c = (in_row - ox * per) * E;
        const unsigned n = r / (unsigned)g.OH, oy = r - n * (unsigned)g.OH;
        const _Float16* sp = x + ((size_t)(n * g.H + oy + g.off_y) * g.W + ox + g.off_x) * g.big_cstride + g.big_coffset + c;
        float* dp = y + ((size_t)r * g.OW + ox) * g.win_cstride + g.win_coffset + c;
        if (!VEC) {
            *dp = (float)*sp;
        } else if ((int)c + E <= g.C) {
            const VH h = *reinterpret_cast<const VH*>(sp);
            reinterpret_cast<VF*>(dp)[0] = VF{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            reinterpret_cast<VF*>(dp)[1] = VF{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
        } else {
            for (int e = 0; (int)c + e < g.C; ++e) dp[e] = (float)sp[e];
        }
    }
}

// The adjoint.  ACC = false: one launch over ALL of dX writes dY inside the window and zeros outside (channels big_coffset ..
// big_coffset + C - 1 of every pixel).  ACC = true: one launch over the window does dX += dY; nothing outside is touched.
// One lane per element group in a fixed assignment: the result does not depend on the run.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(256) void crop_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, CropGeom g, unsigned total) {
    typedef Vec16<float>::type V;
    constexpr int E = VEC ? 4 : 1;
    const unsigned RH = ACC ? g.OH : g.H, RW = ACC ? g.OW : g.W;      // the region this launch walks
    const unsigned per = (unsigned)(g.C + E - 1) / E, row = RW * per;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const unsigned r = t / row, in_row = t - r * row;
        const unsigned px = in_row / per, c = (in_row - px * per) * E;
        const unsigned n = r / RH, py = r - n * RH;
        // (iy, ix): the pixel of dX; (oy, ox): the pixel of dY it takes its value from, when inside the window
        const int iy = ACC ? (int)py + g.off_y : (int)py, ix = ACC ? (int)px + g.off_x : (int)px;
        const int oy = iy - g.off_y, ox = ix - g.off_x;
        const bool inside = ACC || ((unsigned)oy < (unsigned)g.OH && (unsigned)ox < (unsigned)g.OW);
        float* dp = dx + ((size_t)(n * g.H + iy) * g.W + ix) * g.big_cstride + g.big_coffset + c;
        const float* sp = dy + (inside ? ((size_t)(n * g.OH + oy) * g.OW + ox) * g.win_cstride + g.win_coffset + c : 0);      // read only when inside
        if (!VEC) {
            const float v = inside ? *sp : 0.f;
            *dp = ACC ? *dp + v : v;
        } else if ((int)c + E <= g.C) {
            V v = {0.f, 0.f, 0.f, 0.f};
            if (inside) v = *reinterpret_cast<const V*>(sp);
            if (ACC) v += *reinterpret_cast<const V*>(dp);
            *reinterpret_cast<V*>(dp) = v;
        } else {
            for (int e = 0; (int)c + e < g.C; ++e) {
                const float v = inside ? sp[e] : 0.f;
                dp[e] = ACC ? dp[e] + v : v;
            }
        }
    }
}

// the checks the entry points share; `esize` 4 or 2, `win_esize` (0: the same) that of the window-sized view.  Every one precedes the
// first HIP call.
int crop_check(const char* who, const void* big, const void* win, int N, int H, int W, int C, int big_cstride, int big_coffset, int off_y,
               int off_x, int OH, int OW, int win_cstride, int win_coffset, int esize, CropGeom* g, int win_esize = 0) {
    const int E = 16 / esize, EW = win_esize ? 16 / win_esize : E;
    FCN_REQUIRE(big && win && N > 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, FCN_E_ARG, "%s: null pointer or non-positive extent", who);
    FCN_REQUIRE(big_coffset >= 0 && win_coffset >= 0 && big_cstride >= big_coffset + C && win_cstride >= win_coffset + C, FCN_E_ARG,
                "%s: slice out of range", who);
    FCN_REQUIRE(off_y >= 0 && off_x >= 0 && (long long)off_y + OH <= H && (long long)off_x + OW <= W, FCN_E_ARG,
                "%s: window %d+%d x %d+%d leaves the %d x %d view", who, off_y, OH, off_x, OW, H, W);
    if (EW == E)
        FCN_REQUIRE(big_cstride % E == 0 && win_cstride % E == 0 && aligned16(big) && aligned16(win), FCN_E_ALIGN,
                    "%s: strides must be multiples of %d elements, pointers of 16 bytes", who, E);
    else
        FCN_REQUIRE(big_cstride % E == 0 && win_cstride % EW == 0 && aligned16(big) && aligned16(win), FCN_E_ALIGN,
                    "%s: strides must be multiples of %d (x) and %d (y) elements, pointers of 16 bytes", who, E, EW);
    FCN_REQUIRE((long long)N * H * W * big_cstride < (1ll << 31) && (long long)N * OH * OW * win_cstride < (1ll << 31), FCN_E_UNSUPPORTED,
                "%s: views past 2^31 elements", who);
    *g = CropGeom{H, W, OH, OW, off_y, off_x, C, big_cstride, big_coffset, win_cstride, win_coffset};
    return 0;
}

template <typename T>
int crop_fwd(const char* who, const T* x, T* y, const CropGeom& g, int N, fcn_stream_t s) {
    constexpr int E = 16 / (int)sizeof(T);
    const bool vec = g.big_coffset % E == 0 && g.win_coffset % E == 0;
    const long long total = (long long)N * g.OH * g.OW * (vec ? cdiv(g.C, E) : g.C);
    if (vec)
        hipLaunchKernelGGL((crop_fwd_kernel<T, true>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), x, y, g, (unsigned)total);
    else
        hipLaunchKernelGGL((crop_fwd_kernel<T, false>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), x, y, g, (unsigned)total);
    FCN_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" {

int fcn_crop_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x, int OH, int OW,
                     int y_cstride, int y_coffset, fcn_stream_t s) {
    CropGeom g;
    if (int rc = crop_check("crop_fwd", x, y, N, H, W, C, x_cstride, x_coffset, off_y, off_x, OH, OW, y_cstride, y_coffset, 4, &g)) return rc;
    return crop_fwd<float>("crop_fwd", x, y, g, N, s);
}

int fcn_crop_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x, int OH, int OW,
                     int y_cstride, int y_coffset, fcn_stream_t s) {
    CropGeom g;
    if (int rc = crop_check("crop_fwd_f16", x, y, N, H, W, C, x_cstride, x_coffset, off_y, off_x, OH, OW, y_cstride, y_coffset, 2, &g)) return rc;
    return crop_fwd<_Float16>("crop_fwd_f16", reinterpret_cast<const _Float16*>(x), reinterpret_cast<_Float16*>(y), g, N, s);
}

int fcn_crop_fwd_f16_f32(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x, int OH, int OW,
                         int y_cstride, int y_coffset, fcn_stream_t s) {
    CropGeom g;
    if (int rc = crop_check("crop_fwd_f16_f32", x, y, N, H, W, C, x_cstride, x_coffset, off_y, off_x, OH, OW, y_cstride, y_coffset, 2, &g, 4)) return rc;
    const bool vec = x_coffset % 8 == 0 && y_coffset % 4 == 0;
    const long long total = (long long)N * OH * OW * (vec ? cdiv(C, 8) : C);
    const _Float16* xh = reinterpret_cast<const _Float16*>(x);
    float* yf = reinterpret_cast<float*>(y);
    if (vec)
        hipLaunchKernelGGL((crop_fwd_f16_f32_kernel<true>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), xh, yf, g, (unsigned)total);
    else
        hipLaunchKernelGGL((crop_fwd_f16_f32_kernel<false>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(s), xh, yf, g, (unsigned)total);
    FCN_LAUNCH_CHECK("crop_fwd_f16_f32");
    return 0;
}

int fcn_crop_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset, int off_y, int off_x, int OH,
                     int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s) {
    CropGeom g;
    if (int rc = crop_check("crop_bwd", dx, dy, N, H, W, C, dx_cstride, dx_coffset, off_y, off_x, OH, OW, dy_cstride, dy_coffset, 4, &g)) return rc;
    FCN_REQUIRE(accumulate == 0 || accumulate == 1, FCN_E_ARG, "crop_bwd: accumulate must be 0 or 1");
    const bool vec = dx_coffset % 4 == 0 && dy_coffset % 4 == 0;
    const long long pixels = accumulate ? (long long)N * OH * OW : (long long)N * H * W;
    const long long total = pixels * (vec ? cdiv(C, 4) : C);
    const dim3 grid(stream_grid(total, 256)), block(256);
#define FCN_CROP_BWD(VEC, ACC) hipLaunchKernelGGL((crop_bwd_kernel<VEC, ACC>), grid, block, 0, as_stream(s), dy, dx, g, (unsigned)total)
    if (vec && accumulate) FCN_CROP_BWD(true, true);
    else if (vec) FCN_CROP_BWD(true, false);
    else if (accumulate) FCN_CROP_BWD(false, true);
    else FCN_CROP_BWD(false, false);
#undef FCN_CROP_BWD
    FCN_LAUNCH_CHECK("crop_bwd");
    return 0;
}

}  // extern "C"
