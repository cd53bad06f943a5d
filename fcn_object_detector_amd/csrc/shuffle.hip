// Channel shuffle on NHWC views (the ShuffleChannel layer of the ShuffleNet ports).  With n = C / group, for every pixel
//   y[j * group + i] (+)= x[i * n + j]        0 <= i < group, 0 <= j < n
// The inverse permutation is the same operation with group n, so the data gradient is this launch with group C / g.
//
// Work layout: chan_group.h's.  A lane owns one 16-byte group of the OUTPUT (4 floats / 8 halves), gathers the group's source channels
// from the same pixel with scalar loads and stores the group whole; a last, partial group is stored in pieces (cg_store_acc,
// cg_store_h8).  The source channel of each of the lane's outputs is worked out once per lane, never per pixel.  Only channels inside
// x's window are read - a channel of a partial group that lies past C reads the lane's first source again and is not stored - and only
// channels inside y's window are written.  All lanes of a pixel together read its row exactly once.  No LDS, no atomics, no arithmetic
// but the accumulate's add, one writer per element: the same call gives the same bits.
#include "chan_group.h"

namespace fcn {
namespace {

constexpr int SHUFFLE_MAX_GROUPS = 2048;      // workgroups of a launch: 8 per CU of a 256-CU part, every wave slot taken

// the source channels (from x's pixel start, the window's offset included) of the lane's outputs c0 .. c0 + EPG - 1
template <int EPG>
__device__ inline void shuffle_sources(const CgLane& l, int C, int group, int xco, int (&src)[EPG]) {
    const int n = C / group;
#pragma unroll
    for (int k = 0; k < EPG; ++k) {
        const int c = k < l.nv ? l.c0 + k : l.c0;
        src[k] = xco + (c % group) * n + c / group;
    }
}

__global__ __launch_bounds__(CG_THREADS) void shuffle_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int pixels, int C, int group, int xcs,
                                                                  int xco, int ycs, int yco, int accumulate, int tg) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    int src[4];
    shuffle_sources<4>(l, C, group, xco, src);
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        const float* row = x + (size_t)p * xcs;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = row[src[k]];
        cg_store_acc(y + (size_t)p * ycs + yco + l.c0, o, l.nv, accumulate);
    }
}

__global__ __launch_bounds__(CG_THREADS) void shuffle_f16_kernel(const __half* __restrict__ x, __half* __restrict__ y, int pixels, int C, int group, int xcs,
                                                                  int xco, int ycs, int yco, int tg) {
    const CgLane l = cg_lane<8>(tg, C);
    if (l.nv <= 0) return;
    int src[8];
    shuffle_sources<8>(l, C, group, xco, src);
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        const __half* row = x + (size_t)p * xcs;
        CgH8 out;
#pragma unroll
        for (int k = 0; k < 8; ++k) out.h[k] = row[src[k]];
        cg_store_h8(y + (size_t)p * ycs + yco + l.c0, out, l.nv);
    }
}

#ifdef FCN_SHUFFLE_LDS
// Experiment build (make exp EXP=-DFCN_SHUFFLE_LDS EXPNAME=shuffle_lds EXPSRC=shuffle; tools/shuffle_bench.py under $FCN_LIB_PATH): the form
// that stages a workgroup's pixel rows through LDS - whole-group loads, the permutation on the way into LDS (a table of destinations,
// worked out once per workgroup), whole-group reads from LDS and whole-group stores.  DESIGN.md 4.29 has both forms' times; the
// library ships the direct gather above.  A lane still stores only channels inside y's window; the pad channels of x that a whole-group
// load brings along land in LDS slots past C that no store reads.
constexpr int SHUFFLE_LDS_GROUPS = 1024;      // 16 KB of pixel rows per workgroup
constexpr int SHUFFLE_LDS_MAX_C = 1024;       // the table of destinations

template <class T>
__global__ __launch_bounds__(CG_THREADS) void shuffle_lds_kernel(const T* __restrict__ x, T* __restrict__ y, int pixels, int C, int group, int xcs, int xco,
                                                                  int ycs, int yco, int accumulate, int rows) {
    constexpr int EPG = 16 / (int)sizeof(T);
    __shared__ uint4 tile[SHUFFLE_LDS_GROUPS];
    __shared__ short dst[SHUFFLE_LDS_MAX_C + 8];
    const int cg = (C + EPG - 1) / EPG, n = C / group, tid = threadIdx.x;
    for (int s = tid; s < cg * EPG; s += CG_THREADS) dst[s] = (short)(s < C ? (s % n) * group + s / n : s);      // x[i * n + j] -> y[j * group + i]
    __syncthreads();
    T* lds = reinterpret_cast<T*>(tile);
    for (long long p0 = (long long)blockIdx.x * rows; p0 < pixels; p0 += (long long)gridDim.x * rows) {
        const int r = (int)min((long long)rows, pixels - p0);
        for (int i = tid; i < r * cg; i += CG_THREADS) {
            const int pr = i / cg, q = i - pr * cg;
            union { uint4 u; T e[EPG]; } v;
            v.u = *reinterpret_cast<const uint4*>(x + (size_t)(p0 + pr) * xcs + xco + q * EPG);
#pragma unroll
            for (int k = 0; k < EPG; ++k) lds[pr * cg * EPG + dst[q * EPG + k]] = v.e[k];
        }
        __syncthreads();
        for (int i = tid; i < r * cg; i += CG_THREADS) {
            const int pr = i / cg, q = i - pr * cg, nv = min(EPG, C - q * EPG);
            T* out = y + (size_t)(p0 + pr) * ycs + yco + q * EPG;
            if constexpr (sizeof(T) == 4) {
                const uint4 u = tile[i];
                float o[4] = {__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
                cg_store_acc(out, o, nv, accumulate);
            } else {
                CgH8 o;
                o.u = tile[i];
                cg_store_h8(out, o, nv);
            }
        }
        __syncthreads();
    }
}

template <class T>
inline bool shuffle_lds_launch(const T* x, T* y, int pixels, int C, int group, int xcs, int xco, int ycs, int yco, int accumulate, fcn_stream_t s) {
    constexpr int EPG = 16 / (int)sizeof(T);
    const int cg = (C + EPG - 1) / EPG;
    if (C > SHUFFLE_LDS_MAX_C || cg > SHUFFLE_LDS_GROUPS) return false;
    const int rows = SHUFFLE_LDS_GROUPS / cg;
    long long grid = ((long long)pixels + rows - 1) / rows;
    if (grid > SHUFFLE_MAX_GROUPS) grid = SHUFFLE_MAX_GROUPS;
    hipLaunchKernelGGL(shuffle_lds_kernel<T>, dim3((unsigned)grid), dim3(CG_THREADS), 0, as_stream(s), x, y, pixels, C, group, xcs, xco, ycs, yco, accumulate, rows);
    return true;
}
#endif

// the byte ranges from the first to the last element of the two windows intersect
inline bool shuffle_overlap(const void* x, const void* y, int pixels, int C, int xcs, int xco, int ycs, int yco, int esize) {
    const uintptr_t x0 = (uintptr_t)x + (uintptr_t)xco * esize, x1 = x0 + ((uintptr_t)(pixels - 1) * xcs + C) * esize;
    const uintptr_t y0 = (uintptr_t)y + (uintptr_t)yco * esize, y1 = y0 + ((uintptr_t)(pixels - 1) * ycs + C) * esize;
    return x0 < y1 && y0 < x1;
}

}  // namespace
}  // namespace fcn

using namespace fcn;

int fcn_shuffle_channel_f32(const float* x, float* y, int pixels, int C, int group, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                            int accumulate, fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "shuffle_channel: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "shuffle_channel: non-positive extent");
    FCN_REQUIRE(group >= 1 && C % group == 0, FCN_E_ARG, "shuffle_channel: group %d does not divide %d channels", group, C);
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset), FCN_E_ARG, "shuffle_channel: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 4) && cg_view_ok(y_cstride, y_coffset, 4), FCN_E_ALIGN,
                "shuffle_channel: channel strides and offsets must be multiples of 4 floats");
    FCN_REQUIRE(cg_aligned16(x, y), FCN_E_ALIGN, "shuffle_channel: x and y must be 16-byte aligned");
    FCN_REQUIRE(!shuffle_overlap(x, y, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset, 4), FCN_E_ARG,
                "shuffle_channel: the windows of x and y overlap (the layer cannot run in place)");
#ifdef FCN_SHUFFLE_LDS
    if (shuffle_lds_launch(x, y, pixels, C, group, x_cstride, x_coffset, y_cstride, y_coffset, accumulate ? 1 : 0, s)) {
        FCN_LAUNCH_CHECK("shuffle_lds_kernel");
        return 0;
    }
#endif
    const CgTile t = cg_tile(1, pixels, C, 4, SHUFFLE_MAX_GROUPS);
    hipLaunchKernelGGL(shuffle_f32_kernel, dim3(t.gx, t.gy), dim3(CG_THREADS), 0, as_stream(s), x, y, pixels, C, group, x_cstride, x_coffset, y_cstride,
                       y_coffset, accumulate ? 1 : 0, t.tg);
    FCN_LAUNCH_CHECK("shuffle_f32_kernel");
    return 0;
}

int fcn_shuffle_channel_f16(const void* x, void* y, int pixels, int C, int group, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                            fcn_stream_t s) {
    FCN_REQUIRE(x && y, FCN_E_ARG, "shuffle_channel_f16: null x / y");
    FCN_REQUIRE(pixels > 0 && C > 0, FCN_E_ARG, "shuffle_channel_f16: non-positive extent");
    FCN_REQUIRE(group >= 1 && C % group == 0, FCN_E_ARG, "shuffle_channel_f16: group %d does not divide %d channels", group, C);
    FCN_REQUIRE(cg_view_in(C, x_cstride, x_coffset) && cg_view_in(C, y_cstride, y_coffset), FCN_E_ARG,
                "shuffle_channel_f16: channel slice out of range");
    FCN_REQUIRE(cg_view_ok(x_cstride, x_coffset, 8) && cg_view_ok(y_cstride, y_coffset, 8), FCN_E_ALIGN,
                "shuffle_channel_f16: channel strides and offsets must be multiples of 8 halves");
    FCN_REQUIRE(cg_aligned16(x, y), FCN_E_ALIGN, "shuffle_channel_f16: x and y must be 16-byte aligned");
    FCN_REQUIRE(!shuffle_overlap(x, y, pixels, C, x_cstride, x_coffset, y_cstride, y_coffset, 2), FCN_E_ARG,
                "shuffle_channel_f16: the windows of x and y overlap (the layer cannot run in place)");
#ifdef FCN_SHUFFLE_LDS
    if (shuffle_lds_launch(static_cast<const __half*>(x), static_cast<__half*>(y), pixels, C, group, x_cstride, x_coffset, y_cstride, y_coffset, 0, s)) {
        FCN_LAUNCH_CHECK("shuffle_lds_kernel");
        return 0;
    }
#endif
    const CgTile t = cg_tile(1, pixels, C, 8, SHUFFLE_MAX_GROUPS);
    hipLaunchKernelGGL(shuffle_f16_kernel, dim3(t.gx, t.gy), dim3(CG_THREADS), 0, as_stream(s), static_cast<const __half*>(x), static_cast<__half*>(y), pixels,
                       C, group, x_cstride, x_coffset, y_cstride, y_coffset, t.tg);
    FCN_LAUNCH_CHECK("shuffle_f16_kernel");
    return 0;
}
