// The channel-group work layout of the elementwise and per-channel kernels on NHWC views (act.hip, neuron.hip, gate.hip, batchnorm.hip;
// DESIGN.md 4.27a), once:
//   - a lane owns ONE 16-byte channel group of a pixel (4 floats / 8 halves);
//   - the `tg` lanes next to each other own consecutive groups of the same pixel (tg = 16 where C allows: 256 contiguous bytes per
//     pixel row), the 256 / tg rows of a workgroup own consecutive pixels;
//   - the streaming launches stride over a capped grid (gx, gy[, images]);
//   - a C that is no multiple of the group stores its last group in pieces: channels outside coffset .. coffset + C - 1 are never
//     written; loads of whole groups stay inside the pixel because strides and offsets are multiples of the group;
//   - reductions over pixels use no atomics: a workgroup folds its slab of pixels (rows ascending) through LDS, the slabs' partial sums
//     go to a workspace, and a second launch folds them per channel in a fixed order - lane l of the channel's wave folds slabs l,
//     l + 64, ... ascending, then the lanes fold by halves (32, 16, .. 1).  The same call gives the same bits.
// Nothing here knows a layer: a family supplies its checks and messages, its caps, and either a functor for the two streaming kernel
// templates at the end or kernels of its own on top of the helpers.
#pragma once

#include "common.h"

#include <hip/hip_fp16.h>

namespace fcn {
namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_MAX_GROUPS = 16384;      // workgroups of a streaming launch (a family may ask for fewer)
constexpr int CG_MAX_SLABS = 1024;

// ---------------------------------------------------------------------------------------------------------------- host side
struct CgTile {
    int tg;        // channel groups side by side in a workgroup (power of two, <= 16)
    int rows;      // pixels side by side: CG_THREADS / tg
    int gx;        // workgroups along the channel groups
    int gy;        // workgroups along the pixels of an image (the streaming launches: grid-stride over the rest)
    int slabs;     // slabs of pixels per image (the reductions) ...
    int slab_px;   // ... of this many pixels each (the last one shorter); never below `rows`
};

// epg: elements per group (4 floats, 8 halves).  Both caps are spread over the images, which are the grid's z axis.
inline CgTile cg_tile(int images, int ppi, int C, int epg, int max_groups = CG_MAX_GROUPS) {
    CgTile t;
    const int cg = (C + epg - 1) / epg;
    t.tg = 1;
    while (t.tg < cg && t.tg < 16) t.tg <<= 1;
    t.rows = CG_THREADS / t.tg;
    t.gx = (cg + t.tg - 1) / t.tg;
    const long long per_image = (long long)t.gx * images;
    const long long gy = ((long long)ppi + t.rows - 1) / t.rows;
    long long cap = max_groups / per_image;
    if (cap < 1) cap = 1;
    t.gy = (int)(gy < cap ? gy : cap);
    long long want = 2048 / per_image;
    if (want < 1) want = 1;
    if (want > CG_MAX_SLABS) want = CG_MAX_SLABS;
    t.slab_px = (int)((ppi + want - 1) / want);
    if (t.slab_px < t.rows) t.slab_px = t.rows;      // every row of a workgroup gets a pixel
    t.slabs = (ppi + t.slab_px - 1) / t.slab_px;
    return t;
}

inline bool cg_view_in(int C, int cstride, int coffset) { return coffset >= 0 && cstride >= coffset + C; }
inline bool cg_view_ok(int cstride, int coffset, int epg) { return cstride % epg == 0 && coffset % epg == 0; }
// every pointer 16-byte aligned (a null one is)
template <class... P>
inline bool cg_aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- device side
struct CgLane {
    int gl, row, rows;      // the lane's group column and pixel row in the workgroup; the workgroup's rows
    int c0, nv;             // first channel of the lane's group; its channels inside C (<= 0: the group lies past C)
};

template <int EPG>
__device__ inline CgLane cg_lane(int tg, int C) {
    CgLane l;
    l.gl = threadIdx.x % tg;
    l.row = threadIdx.x / tg;
    l.rows = CG_THREADS / tg;
    l.c0 = EPG * (blockIdx.x * tg + l.gl);
    l.nv = min(EPG, C - l.c0);
    return l;
}

// the lane's pixels of a streaming launch: for (p = cg_first(l); p < pixels; p += cg_step(l))
__device__ inline long long cg_first(const CgLane& l) { return (long long)blockIdx.y * l.rows + l.row; }
__device__ inline long long cg_step(const CgLane& l) { return (long long)gridDim.y * l.rows; }

union CgH8 {
    uint4 u;
    unsigned w[4];
    __half h[8];
};

__device__ inline void cg_load(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__device__ inline CgH8 cg_load_h8(const __half* p) {
    CgH8 v;
    v.u = *reinterpret_cast<const uint4*>(p);
    return v;
}

// Floats: a whole group as 16 bytes, a partial one in a loop of nv trips.  The loop is on purpose: unrolled and predicated, both paths
// store o[0] to p[0], the compiler merges those two stores and the whole group leaves as 12 + 4 bytes (DESIGN.md 4.27a has the
// measurement); the float arrays stay in registers either way.
__device__ inline void cg_store(float* p, const float (&o)[4], int nv) {
    if (nv == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; j < nv; ++j) p[j] = o[j];
    }
}

// p (+)= o
__device__ inline void cg_store_acc(float* p, float (&o)[4], int nv, int accumulate) {
    if (nv == 4) {
        if (accumulate) {
            const float4 old = *reinterpret_cast<const float4*>(p);
            o[0] += old.x; o[1] += old.y; o[2] += old.z; o[3] += old.w;
        }
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; j < nv; ++j) p[j] = accumulate ? p[j] + o[j] : o[j];
    }
}

// Halves, three store forms: a whole group as 16 bytes; of a last, partial group the whole pairs as 32-bit words and an odd last
// channel as one half - the pad half that shares its word is not written.  Unrolled and predicated: here an index that is no
// constant does move the union out of the registers (into 4096 bytes of LDS per workgroup).
__device__ inline void cg_store_h8(__half* p, const CgH8& o, int nv) {
    if (nv == 8) {
        *reinterpret_cast<uint4*>(p) = o.u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (2 * k + 1 < nv) reinterpret_cast<unsigned*>(p)[k] = o.w[k];
            else if (2 * k < nv) p[2 * k] = o.h[2 * k];
        }
    }
}

__device__ inline float4 cg_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// fold of the 256 / tg rows of a workgroup through red[CG_THREADS], rows ascending, by the row-0 thread of each group column: only
// those threads get the sum.  Every thread of the workgroup calls it; a second fold through the same `red` needs a barrier between.
__device__ inline float4 cg_fold_rows(float4 v, float4* red, const CgLane& l, int tg) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (l.row == 0)
        for (int r = 1; r < l.rows; ++r) v = cg_add(v, red[r * tg + l.gl]);
    return v;
}

// the wave fold of one channel's slab sums, K accumulators side by side: a[k] = sum over s of ws[(K * s + k) * C4], ws at the channel.
// Lane 0 holds the result.
template <int K>
__device__ inline void cg_fold_slabs(const float* ws, int slabs, int C4, int lane, float (&a)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.f;
    for (int s = lane; s < slabs; s += 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += ws[(size_t)(K * s + k) * C4];
    }
    for (int off = 32; off >= 1; off >>= 1) {
        float b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) b[k] = __shfl_down(a[k], off, 64);
        if (lane < off) {
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] += b[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- streaming kernels
// A functor F is a small struct passed by value with the family's scalars and pointers:
//   typename F::Op                  what a lane keeps per channel of its group (an empty struct where there is nothing)
//   Op fwd_op(c, live) / bwd_op     the prologue: channel c's operand, read once per lane - never per pixel (live: c lies inside C)
//   float fwd(v, op)                y from x
//   float bwd(d, r, op)             dx from dy and ref; F::BWD_REF says whether ref is read at all
// grid (gx, gy).  y may be x, dx may be dy: a lane reads its group of a pixel before it writes it, and no other lane touches that group.
template <class F>
__global__ __launch_bounds__(CG_THREADS) void cg_map_f32_kernel(const float* x, float* y, float* __restrict__ keep, int pixels, int C, int xcs, int xco,
                                                                 int ycs, int yco, int kcs, int tg, F f) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    typename F::Op op[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) op[j] = f.fwd_op(l.c0 + j, j < l.nv);
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        float v[4], o[4];
        cg_load(x + (size_t)p * xcs + xco + l.c0, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f.fwd(v[j], op[j]);
        if (keep) cg_store(keep + (size_t)p * kcs + l.c0, v, l.nv);
        cg_store(y + (size_t)p * ycs + yco + l.c0, o, l.nv);
    }
}

// halves in, halves out, float32 operands and arithmetic, one rounding to half; a lane owns 8 channels
template <class F>
__global__ __launch_bounds__(CG_THREADS) void cg_map_f16_kernel(const __half* x, __half* y, int pixels, int C, int xcs, int xco, int ycs, int yco, int tg,
                                                                 F f) {
    const CgLane l = cg_lane<8>(tg, C);
    if (l.nv <= 0) return;
    typename F::Op op[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) op[j] = f.fwd_op(l.c0 + j, j < l.nv);
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        const CgH8 in = cg_load_h8(x + (size_t)p * xcs + xco + l.c0);
        CgH8 out;
#pragma unroll
        for (int j = 0; j < 8; ++j) out.h[j] = __float2half_rn(f.fwd(__half2float(in.h[j]), op[j]));
        cg_store_h8(y + (size_t)p * ycs + yco + l.c0, out, l.nv);
    }
}

template <class F>
__global__ __launch_bounds__(CG_THREADS) void cg_bwd_f32_kernel(const float* dy, const float* __restrict__ ref, float* dx, int pixels, int C, int dcs,
                                                                 int dco, int rcs, int rco, int xcs, int xco, int accumulate, int tg, F f) {
    const CgLane l = cg_lane<4>(tg, C);
    if (l.nv <= 0) return;
    typename F::Op op[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) op[j] = f.bwd_op(l.c0 + j, j < l.nv);
    for (long long p = cg_first(l); p < pixels; p += cg_step(l)) {
        float d[4], r[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        cg_load(dy + (size_t)p * dcs + dco + l.c0, d);
        if (F::BWD_REF) cg_load(ref + (size_t)p * rcs + rco + l.c0, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f.bwd(d[j], r[j], op[j]);
        cg_store_acc(dx + (size_t)p * xcs + xco + l.c0, o, l.nv, accumulate);
    }
}

}  // namespace
}  // namespace fcn
