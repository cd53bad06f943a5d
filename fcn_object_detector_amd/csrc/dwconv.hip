// Depthwise convolution for MI355X (gfx950): Caffe ConvolutionLayer with group == channels == num_output (the 3x3 layers of MobileNet
// v1 / v2 and MobileNet-SSD, the separable blocks of Xception / DeepLab-v3+, ERFNet-style blocks) - forward in float32 and in halves,
// data gradient and weight gradient, with per-axis kernel, pad and stride and one dilation for both axes.
//
//   y[n, oy, ox, c] = bias[c] + sum over r, q of w[r][q][c] * x[n, oy*sh - ph + r*dil, ox*sw - pw + q*dil, c]
//
// kh*kw multiply-adds per element moved: the layer is bound by memory and runs on the vector units, NHWC.  The bank is tap-major and
// channel-contiguous, [kh][kw][roundS(C)] float32 (S = the bottom's 16-byte segment: 4 floats, 8 halves), pad channels zero, so a lane
// that owns a channel segment fetches a tap's weights with one 16-byte load (two for 8 halves).
//
// Forward (dw_fwd_plain_kernel, dw_fwd_strip_kernel): a lane owns one 16-byte channel segment of one output pixel (plain: every
// geometry) or of a strip of output pixels along x (strip: stride_w 1 or 2, no dilation, kw 1 / 3 / 5 / 7); consecutive lanes run along
// the channels of a pixel, so every global access is coalesced.  The strip form keeps a filter row's weights in registers and loads
// each input column that neighbouring outputs share once.  No LDS.
//
// Data gradient (dw_dgrad_kernel): a gather over the taps with oy*sh == iy + ph - r*dil, ox*sw == ix + pw - q*dil - the same bank, no
// flip, no atomics, any stride.  No LDS.
//
// Weight gradient (dw_wgrad_kernel): a workgroup takes 16, 32 or 64 channels, a group of up to 9 taps and a split of the N*OH*OW pixels;
// the 64, 32 or 16 lanes of a channel segment walk the split's pixels, accumulate in registers and are added in LDS in lane order
// (4 KiB); the sum of dY (db) rides in the workgroups of the first tap group.  One split writes dw and db directly; otherwise every
// split writes a slab and dw_wgrad_finish_kernel adds the slabs in a fixed order (64 lanes per column, each its slabs in ascending
// order, then a fold by halves).
//
// Deterministic: every output element belongs to exactly one lane, the order of every sum depends only on the descriptor (and the
// split request), there is no atomic.
#include "conv_common.h"

namespace fcn {
namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_MAX_K = 7;
constexpr int DW_CFGS = 2;          // 0: one output pixel per lane, 1: a strip of output pixels per lane
constexpr int DW_STRIP_F32 = 4;     // output pixels of a strip (4 channels per lane)
constexpr int DW_STRIP_F16 = 2;     // ... with 8 channels per lane
constexpr int WG_TAPS = 9;          // weight gradient: taps (accumulators of four floats) per workgroup
constexpr int WG_MAX_SPLITS = 1024;

struct DwP {
    const void* x;
    const float* w;
    const float* bias;
    void* y;
    const float* y2;
    int N, H, W, C, x_cstride, kh, kw, pad_h, pad_w, stride_h, stride_w, dil, OH, OW;
    int y_cstride, y_coffset, y2_cstride, y2_coffset, flags;
    int segs, bank_c, strips, y_vec, y2_vec;      // channel segments per pixel, channels of a bank row, strips per output row
    int items;
};

// ---- a lane's channel segment: S floats, read from 16 bytes of floats or of halves
template <int S> struct Seg { float v[S]; };

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int S = 4;
    static __device__ __forceinline__ Seg<4> load(const float* p) {
        const v4f t = *(const v4f*)p;
        return Seg<4>{{t[0], t[1], t[2], t[3]}};
    }
};
template <> struct Elem<f16_t> {
    static constexpr int S = 8;
    static __device__ __forceinline__ Seg<8> load(const f16_t* p) {
        const v8h t = *(const v8h*)p;
        Seg<8> s;
#pragma unroll
        for (int e = 0; e < 8; ++e) s.v[e] = (float)t[e];
        return s;
    }
};

template <int S>
__device__ __forceinline__ Seg<S> load_bank(const float* p) {
    Seg<S> s;
#pragma unroll
    for (int g = 0; g < S / 4; ++g) {
        const v4f t = *(const v4f*)(p + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) s.v[4 * g + e] = t[e];
    }
    return s;
}

// bias, accumulate, ReLU, mask and the store of one output pixel's segment: channels c0 .. c0 + S - 1, those below C only
template <typename TI, int S>
__device__ __forceinline__ void dw_store(const DwP& p, size_t pix, int c0, Seg<S> a) {
    const bool relu = (p.flags & FCN_CONV_RELU) != 0, accum = (p.flags & FCN_CONV_ACCUM) != 0, mask = (p.flags & FCN_CONV_MASK) != 0;
    const bool out_f32 = sizeof(TI) == 4 || (p.flags & FCN_CONV_OUT_F32) != 0;
    const size_t off = pix * p.y_cstride + p.y_coffset + c0;
    const float* y2 = mask ? p.y2 + pix * p.y2_cstride + p.y2_coffset + c0 : nullptr;
    const bool whole = c0 + S <= p.C;
    if (p.bias) {
#pragma unroll
        for (int e = 0; e < S; ++e)
            if (c0 + e < p.C) a.v[e] += p.bias[c0 + e];
    }
    if (whole && p.y_vec && (!mask || p.y2_vec)) {
        if (out_f32) {
            float* dst = (float*)p.y + off;
#pragma unroll
            for (int g = 0; g < S / 4; ++g) {
                v4f v = {a.v[4 * g], a.v[4 * g + 1], a.v[4 * g + 2], a.v[4 * g + 3]};
                if (accum) v += *(const v4f*)(dst + 4 * g);
                if (relu) for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                if (mask) { const v4f m = *(const v4f*)(y2 + 4 * g); for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f; }
                *(v4f*)(dst + 4 * g) = v;
            }
        } else {
            v8h h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (f16_t)(relu ? fmaxf(a.v[e % S], 0.f) : a.v[e % S]);
            *(v8h*)((f16_t*)p.y + off) = h;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < S; ++e) {
        if (c0 + e >= p.C) break;
        float v = a.v[e];
        if (out_f32) {
            float* dst = (float*)p.y + off + e;
            if (accum) v += *dst;
            if (relu) v = fmaxf(v, 0.f);
            if (mask) v = y2[e] > 0.f ? v : 0.f;
            *dst = v;
        } else {
            ((f16_t*)p.y)[off + e] = (f16_t)(relu ? fmaxf(v, 0.f) : v);
        }
    }
}

// ---- forward, one output pixel per lane: every geometry.  K > 0: kh == kw == K, the taps unrolled - every tap's address is clamped into
// the image and its value dropped by a select where the tap lies outside, so the K*K loads are issued together and not one behind the
// other (the kernel is one dependent chain of loads otherwise: at the sizes of a MobileNet that chain IS its run time).  K == 0: loops.
template <typename TI, int K>
__global__ __launch_bounds__(DW_THREADS) void dw_fwd_plain_kernel(const DwP p) {
    constexpr int S = Elem<TI>::S;
    const int i = blockIdx.x * DW_THREADS + threadIdx.x;
    if (i >= p.items) return;
    const int m = i / p.segs, c0 = (i - m * p.segs) * S;
    const int ox = m % p.OW, t = m / p.OW;
    const int oy = t % p.OH, n = t / p.OH;
    const int iy0 = oy * p.stride_h - p.pad_h, ix0 = ox * p.stride_w - p.pad_w;
    const TI* xn = (const TI*)p.x + (size_t)n * p.H * p.W * p.x_cstride + c0;
    Seg<S> acc;
#pragma unroll
    for (int e = 0; e < S; ++e) acc.v[e] = 0.f;
    if (K > 0) {
        Seg<S> xv[K * K > 0 ? K * K : 1];
        bool ok[K * K > 0 ? K * K : 1];
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const int iy = iy0 + r * p.dil, ix = ix0 + q * p.dil;
                ok[r * K + q] = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
                xv[r * K + q] = Elem<TI>::load(xn + ((size_t)cy * p.W + cx) * p.x_cstride);
            }
#pragma unroll
        for (int tq = 0; tq < K * K; ++tq) {
            const Seg<S> wv = load_bank<S>(p.w + (size_t)tq * p.bank_c + c0);
#pragma unroll
            for (int e = 0; e < S; ++e) acc.v[e] = fmaf(wv.v[e], ok[tq] ? xv[tq].v[e] : 0.f, acc.v[e]);
        }
    } else {
        for (int r = 0; r < p.kh; ++r) {
            const int iy = iy0 + r * p.dil;
            if ((unsigned)iy >= (unsigned)p.H) continue;
            for (int q = 0; q < p.kw; ++q) {
                const int ix = ix0 + q * p.dil;
                if ((unsigned)ix >= (unsigned)p.W) continue;
                const Seg<S> xv = Elem<TI>::load(xn + ((size_t)iy * p.W + ix) * p.x_cstride);
                const Seg<S> wv = load_bank<S>(p.w + (size_t)(r * p.kw + q) * p.bank_c + c0);
#pragma unroll
                for (int e = 0; e < S; ++e) acc.v[e] = fmaf(wv.v[e], xv.v[e], acc.v[e]);
            }
        }
    }
    dw_store<TI, S>(p, (size_t)m, c0, acc);
}

// ---- forward, a strip of T output pixels along x per lane: stride_w SW (1 or 2), no dilation, KW taps per filter row.  The row's
// weights stay in registers for the strip; the (T - 1) SW + KW input columns under it are loaded once.
template <typename TI, int KW, int SW, int T>
__global__ __launch_bounds__(DW_THREADS) void dw_fwd_strip_kernel(const DwP p) {
    constexpr int S = Elem<TI>::S;
    constexpr int SPAN = (T - 1) * SW + KW;
    const int i = blockIdx.x * DW_THREADS + threadIdx.x;
    if (i >= p.items) return;
    const int row = i / p.segs, c0 = (i - row * p.segs) * S;      // row: (n, oy, strip)
    const int st = row % p.strips, t = row / p.strips;
    const int oy = t % p.OH, n = t / p.OH;
    const int ox0 = st * T;
    const int iy0 = oy * p.stride_h - p.pad_h, ix0 = ox0 * SW - p.pad_w;
    const TI* xn = (const TI*)p.x + (size_t)n * p.H * p.W * p.x_cstride + c0;
    Seg<S> acc[T];
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int e = 0; e < S; ++e) acc[j].v[e] = 0.f;
    for (int r = 0; r < p.kh; ++r) {
        const int iy = iy0 + r;
        if ((unsigned)iy >= (unsigned)p.H) continue;
        Seg<S> wv[KW];
#pragma unroll
        for (int q = 0; q < KW; ++q) wv[q] = load_bank<S>(p.w + (size_t)(r * KW + q) * p.bank_c + c0);
        const TI* xr = xn + (size_t)iy * p.W * p.x_cstride;
#pragma unroll
        for (int col = 0; col < SPAN; ++col) {
            const int ix = ix0 + col;
            Seg<S> xv;
            if ((unsigned)ix < (unsigned)p.W) {
                xv = Elem<TI>::load(xr + (size_t)ix * p.x_cstride);
            } else {
#pragma unroll
                for (int e = 0; e < S; ++e) xv.v[e] = 0.f;
            }
            // (a column past the image is a zero; one under no output of the strip's tail is never stored)
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const int q = col - j * SW;
                if (q >= 0 && q < KW) {
#pragma unroll
                    for (int e = 0; e < S; ++e) acc[j].v[e] = fmaf(wv[q].v[e], xv.v[e], acc[j].v[e]);
                }
            }
        }
    }
    const size_t pix0 = ((size_t)n * p.OH + oy) * p.OW + ox0;
#pragma unroll
    for (int j = 0; j < T; ++j)
        if (ox0 + j < p.OW) dw_store<TI, S>(p, pix0 + j, c0, acc[j]);
}

// ty == o * stride with 0 <= o < extent?  (strides 1 and 2 without a division)
__device__ __forceinline__ bool dw_under(int ty, int stride, int extent, int& o) {
    if (stride == 1) o = ty;
    else if (stride == 2) o = ty >> 1;
    else o = ty / stride;
    return ty >= 0 && o * stride == ty && o < extent;
}

// ---- data gradient: a lane owns four channels of one pixel of dX and gathers the taps that reach it.  p describes the FORWARD
// problem: p.y is dY (read), p.x is dX (written), y2 is read at dX's position.  K > 0: kh == kw == K, unrolled as in the forward.
template <int K>
__global__ __launch_bounds__(DW_THREADS) void dw_dgrad_kernel(const DwP p) {
    const int i = blockIdx.x * DW_THREADS + threadIdx.x;
    if (i >= p.items) return;
    const int m = i / p.segs, c0 = (i - m * p.segs) * 4;
    const int ix = m % p.W, t = m / p.W;
    const int iy = t % p.H, n = t / p.H;
    const float* dyn = (const float*)p.y + (size_t)n * p.OH * p.OW * p.y_cstride + p.y_coffset + c0;
    const bool whole = c0 + 4 <= p.C;
    auto load_dy = [&](int oy, int ox) {
        const float* src = dyn + ((size_t)oy * p.OW + ox) * p.y_cstride;
        v4f g = {0.f, 0.f, 0.f, 0.f};
        if (whole && p.y_vec) {
            g = *(const v4f*)src;
        } else {
            g[0] = src[0];
            if (c0 + 1 < p.C) g[1] = src[1];
            if (c0 + 2 < p.C) g[2] = src[2];
            if (c0 + 3 < p.C) g[3] = src[3];
        }
        return g;
    };
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    if (K > 0) {
        v4f g[K * K > 0 ? K * K : 1];
        bool ok[K * K > 0 ? K * K : 1];
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                int oy, ox;
                const bool oky = dw_under(iy + p.pad_h - r * p.dil, p.stride_h, p.OH, oy);
                const bool okx = dw_under(ix + p.pad_w - q * p.dil, p.stride_w, p.OW, ox);
                ok[r * K + q] = oky && okx;
                g[r * K + q] = load_dy(min(max(oy, 0), p.OH - 1), min(max(ox, 0), p.OW - 1));      // (clamped: always inside dY)
            }
#pragma unroll
        for (int tq = 0; tq < K * K; ++tq) {
            const v4f wv = *(const v4f*)(p.w + (size_t)tq * p.bank_c + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], ok[tq] ? g[tq][e] : 0.f, acc[e]);
        }
    } else {
        for (int r = 0; r < p.kh; ++r) {
            int oy;
            if (!dw_under(iy + p.pad_h - r * p.dil, p.stride_h, p.OH, oy)) continue;
            for (int q = 0; q < p.kw; ++q) {
                int ox;
                if (!dw_under(ix + p.pad_w - q * p.dil, p.stride_w, p.OW, ox)) continue;
                const v4f g = load_dy(oy, ox);
                const v4f wv = *(const v4f*)(p.w + (size_t)(r * p.kw + q) * p.bank_c + c0);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], g[e], acc[e]);
            }
        }
    }
    const bool accum = (p.flags & FCN_CONV_ACCUM) != 0, mask = (p.flags & FCN_CONV_MASK) != 0;
    float* dst = (float*)p.x + (size_t)m * p.x_cstride + c0;
    const float* y2 = mask ? p.y2 + (size_t)m * p.y2_cstride + p.y2_coffset + c0 : nullptr;
    if (whole && (!mask || p.y2_vec)) {
        if (accum) acc += *(const v4f*)dst;
        if (mask) { const v4f k = *(const v4f*)y2; for (int e = 0; e < 4; ++e) acc[e] = k[e] > 0.f ? acc[e] : 0.f; }
        *(v4f*)dst = acc;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (c0 + e >= p.C) break;
        float v = acc[e];
        if (accum) v += dst[e];
        if (mask) v = y2[e] > 0.f ? v : 0.f;
        dst[e] = v;
    }
}

// ---- weight gradient
struct DwWgradP {
    const float* x;
    const float* dy;
    float* out;             // dw (one split) or the workspace (a slab of (taps + 1) * C4 floats per split: the taps' rows, then db's)
    float* db;              // NULL: no bias gradient; with one split it is written directly
    int N, H, W, C, x_cstride, kh, kw, pad_h, pad_w, stride_h, stride_w, dil, OH, OW;
    int dy_cstride, dy_coffset, dy_vec;
    int C4, M, pix_per_split, direct;
    unsigned long long slab;
};

// CH channels per workgroup (16, 32 or 64: the smallest that holds round4(C), so narrow layers keep every lane busy), 256 / (CH / 4) lanes
// per channel segment.  Every tap's address is clamped into the image and its value dropped by a select where the tap lies outside: the
// loads of a pixel are issued together.
template <int CH>
__global__ __launch_bounds__(DW_THREADS) void dw_wgrad_kernel(const DwWgradP p) {
    constexpr int SEGS = CH / 4, LANES = DW_THREADS / SEGS;
    __shared__ __attribute__((aligned(16))) float red[LANES * CH];      // 4 KiB
    const int tid = threadIdx.x;
    const int seg = tid % SEGS, pl = tid / SEGS;
    const int c0 = blockIdx.x * CH + seg * 4;
    const int taps = p.kh * p.kw, tap0 = blockIdx.y * WG_TAPS;
    const int split = blockIdx.z;
    const int m0 = split * p.pix_per_split, m1 = min(m0 + p.pix_per_split, p.M);
    const bool live = c0 < p.C4, whole = c0 + 4 <= p.C;

    int dr[WG_TAPS], dq[WG_TAPS];      // (uniform over the workgroup: the taps' row and column offsets)
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t) {
        const int tap = min(tap0 + t, taps - 1);
        dr[t] = (tap / p.kw) * p.dil - p.pad_h;
        dq[t] = (tap % p.kw) * p.dil - p.pad_w;
    }
    v4f acc[WG_TAPS];
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    v4f acc_db = {0.f, 0.f, 0.f, 0.f};      // sum of dY: the first tap group's workgroups own db

    if (live) {
        for (int m = m0 + pl; m < m1; m += LANES) {
            const int ox = m % p.OW, tt = m / p.OW;
            const int oy = tt % p.OH, n = tt / p.OH;
            const float* src = p.dy + (size_t)m * p.dy_cstride + p.dy_coffset + c0;
            v4f g = {0.f, 0.f, 0.f, 0.f};
            if (whole && p.dy_vec) {
                g = *(const v4f*)src;
            } else {
                g[0] = src[0];
                if (c0 + 1 < p.C) g[1] = src[1];
                if (c0 + 2 < p.C) g[2] = src[2];
                if (c0 + 3 < p.C) g[3] = src[3];
            }
            acc_db += g;
            const float* xn = p.x + (size_t)n * p.H * p.W * p.x_cstride + c0;
            const int by = oy * p.stride_h, bx = ox * p.stride_w;
            v4f xv[WG_TAPS];
            bool ok[WG_TAPS];
#pragma unroll
            for (int t = 0; t < WG_TAPS; ++t) {
                const int iy = by + dr[t], ix = bx + dq[t];
                ok[t] = tap0 + t < taps && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const int cy = min(max(iy, 0), p.H - 1), cx = min(max(ix, 0), p.W - 1);
                xv[t] = *(const v4f*)(xn + ((size_t)cy * p.W + cx) * p.x_cstride);
            }
#pragma unroll
            for (int t = 0; t < WG_TAPS; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][e] = fmaf(g[e], ok[t] ? xv[t][e] : 0.f, acc[t][e]);
        }
    }
    // the lanes of a channel segment, added in lane order by the thread that owns the channel
    float* out = p.out + (size_t)split * p.slab;
    const int c = blockIdx.x * CH + tid;
#pragma unroll
    for (int t = 0; t < WG_TAPS; ++t) {
        if (tap0 + t >= taps) break;      // (uniform)
        *(v4f*)&red[pl * CH + seg * 4] = acc[t];
        __syncthreads();
        if (tid < CH && c < p.C4) {
            float s = red[tid];
            for (int k = 1; k < LANES; ++k) s += red[k * CH + tid];
            out[(size_t)(tap0 + t) * p.C4 + c] = c < p.C ? s : 0.f;      // pad channels: exact zeros
        }
        __syncthreads();
    }
    if (p.db && blockIdx.y == 0) {      // (uniform)
        *(v4f*)&red[pl * CH + seg * 4] = acc_db;
        __syncthreads();
        if (tid < CH && c < p.C4) {
            float s = red[tid];
            for (int k = 1; k < LANES; ++k) s += red[k * CH + tid];
            if (!p.direct) out[(size_t)taps * p.C4 + c] = c < p.C ? s : 0.f;
            else if (c < p.C) p.db[c] = s;
        }
    }
}

// Four float4 columns of a slab per workgroup: of a column's 64 lanes, lane l adds slabs l, l + 64, ... in ascending order, then the lanes
// fold by halves - the same order on every run.  Columns 0 .. dw4-1 are dw's; the C4 / 4 behind them (db != NULL) are db's channels.
__global__ __launch_bounds__(256) void dw_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw, long long dw4, long long total4,
                                                               int splits, unsigned long long slab, float* __restrict__ db, int C) {
    __shared__ v4f part4[256];
    const int l = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    v4f s = {0.f, 0.f, 0.f, 0.f};
    if (j < total4)
        for (int k = l; k < splits; k += 64) s += *(const v4f*)(ws + (size_t)k * slab + 4 * j);
    part4[threadIdx.x] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (l < h) part4[threadIdx.x] += part4[threadIdx.x + h];
        __syncthreads();
    }
    if (l != 0 || j >= total4) return;
    const v4f r = part4[threadIdx.x];
    if (j < dw4) {
        *(v4f*)(dw + 4 * j) = r;
    } else {
        const int c = (int)(4 * (j - dw4));
        for (int e = 0; e < 4; ++e)
            if (c + e < C) db[c + e] = r[e];
    }
}

// ---- host side
enum Pass { FWD_F32, FWD_F16, DGRAD, WGRAD };

// (w, bias, y2 and flags are not looked at for WGRAD; y names dY for DGRAD and WGRAD, x names dX for DGRAD)
int validate(const fcn_dwconv_desc& d, Pass pass) {
    const int S = pass == FWD_F16 ? 8 : 4;
    const int ysz = pass == FWD_F16 && !(d.flags & FCN_CONV_OUT_F32) ? 2 : 4;
    FCN_REQUIRE(d.x && d.y && (pass == WGRAD || d.w), FCN_E_ARG, "dwconv: null x/w/y");
    FCN_REQUIRE(d.N > 0 && d.H > 0 && d.W > 0 && d.C > 0 && d.kh > 0 && d.kw > 0 && d.stride_h > 0 && d.stride_w > 0 && d.pad_h >= 0 && d.pad_w >= 0,
                FCN_E_ARG, "dwconv: non-positive extent");
    FCN_REQUIRE(d.dilation >= 1, FCN_E_UNSUPPORTED, "dwconv: dilation %d below 1", d.dilation);
    FCN_REQUIRE(d.kh <= DW_MAX_K && d.kw <= DW_MAX_K, FCN_E_UNSUPPORTED, "dwconv: kernel window %dx%d above %dx%d", d.kh, d.kw, DW_MAX_K, DW_MAX_K);
    const int cs = (d.C + S - 1) / S * S;
    FCN_REQUIRE(d.x_cstride % S == 0 && d.x_cstride >= cs, FCN_E_ALIGN, "dwconv: x_cstride (%d) must be a multiple of %d holding C (%d) padded to %d",
                d.x_cstride, S, d.C, S);
    FCN_REQUIRE(((uintptr_t)d.x & 15) == 0 && (pass == WGRAD || ((uintptr_t)d.w & 15) == 0), FCN_E_ALIGN, "dwconv: x / w must be 16-byte aligned");
    FCN_REQUIRE(((uintptr_t)d.y & (ysz - 1)) == 0 && (pass == WGRAD || !d.bias || ((uintptr_t)d.bias & 3) == 0), FCN_E_ALIGN,
                "dwconv: y / bias must be aligned to their elements");
    const long long eh = (long long)d.dilation * (d.kh - 1) + 1, ew = (long long)d.dilation * (d.kw - 1) + 1;
    const long long nh = (long long)d.H + 2ll * d.pad_h - eh, nw = (long long)d.W + 2ll * d.pad_w - ew;
    FCN_REQUIRE(nh >= 0 && nw >= 0, FCN_E_ARG, "dwconv: the window (%lldx%lld) exceeds the padded image", eh, ew);
    FCN_REQUIRE(d.OH == nh / d.stride_h + 1 && d.OW == nw / d.stride_w + 1, FCN_E_ARG,
                "dwconv: OH/OW (%d,%d) is not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 per axis = (%lld,%lld)", d.OH, d.OW, nh / d.stride_h + 1,
                nw / d.stride_w + 1);
    FCN_REQUIRE(d.y_coffset >= 0 && d.y_cstride >= d.y_coffset + d.C, FCN_E_ARG, "dwconv: output slice exceeds y_cstride");
    if (pass != WGRAD) {
        const int allowed = pass == FWD_F32 ? (FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK)
                            : pass == DGRAD ? (FCN_CONV_ACCUM | FCN_CONV_MASK)
                                            : (FCN_CONV_RELU | FCN_CONV_OUT_F32);
        FCN_REQUIRE((d.flags & ~allowed) == 0, FCN_E_UNSUPPORTED, "dwconv: flags 0x%x outside 0x%x for this pass", d.flags, allowed);
        if (d.flags & FCN_CONV_MASK)
            FCN_REQUIRE(d.y2 && ((uintptr_t)d.y2 & 3) == 0 && d.y2_coffset >= 0 && d.y2_cstride >= d.y2_coffset + d.C, FCN_E_ARG,
                        "dwconv: FCN_CONV_MASK needs y2 with a slice of C channels");
    }
    const long long y2_pix = pass == DGRAD ? (long long)d.N * d.H * d.W : (long long)d.N * d.OH * d.OW;
    FCN_REQUIRE((long long)d.N * d.H * d.W * d.x_cstride < (1ll << 31) && (long long)d.N * d.OH * d.OW * d.y_cstride < (1ll << 31) &&
                    (pass == WGRAD || !(d.flags & FCN_CONV_MASK) || y2_pix * d.y2_cstride < (1ll << 31)),
                FCN_E_UNSUPPORTED, "dwconv: tensor too large for 32-bit element offsets");
    return 0;
}

bool strip_takes(const fcn_dwconv_desc& d) {
    return d.dilation == 1 && (d.stride_w == 1 || d.stride_w == 2) && (d.kw == 1 || d.kw == 3 || d.kw == 5 || d.kw == 7);
}

void fill(DwP& p, const fcn_dwconv_desc& d, int S, int ysz) {
    p.x = d.x; p.w = d.w; p.bias = d.bias; p.y = d.y; p.y2 = (d.flags & FCN_CONV_MASK) ? d.y2 : nullptr;
    p.N = d.N; p.H = d.H; p.W = d.W; p.C = d.C; p.x_cstride = d.x_cstride; p.kh = d.kh; p.kw = d.kw;
    p.pad_h = d.pad_h; p.pad_w = d.pad_w; p.stride_h = d.stride_h; p.stride_w = d.stride_w; p.dil = d.dilation; p.OH = d.OH; p.OW = d.OW;
    p.y_cstride = d.y_cstride; p.y_coffset = d.y_coffset; p.y2_cstride = d.y2_cstride; p.y2_coffset = d.y2_coffset; p.flags = d.flags;
    p.segs = (d.C + S - 1) / S;
    p.bank_c = p.segs * S;
    p.strips = 0;
    // whole-segment stores / loads: the view starts on 16 bytes and its stride and offset are whole 16-byte runs of its elements
    const int ya = 16 / ysz;
    p.y_vec = (((uintptr_t)d.y & 15) == 0 && d.y_cstride % ya == 0 && d.y_coffset % ya == 0) ? 1 : 0;
    p.y2_vec = (p.y2 && ((uintptr_t)d.y2 & 15) == 0 && d.y2_cstride % 4 == 0 && d.y2_coffset % 4 == 0) ? 1 : 0;
    p.items = 0;
}

template <typename TI, int T, int SW>
void launch_strip_kw(const DwP& p, int kw, unsigned grid, hipStream_t st) {
    switch (kw) {
        case 1: hipLaunchKernelGGL((dw_fwd_strip_kernel<TI, 1, SW, T>), dim3(grid), dim3(DW_THREADS), 0, st, p); break;
        case 3: hipLaunchKernelGGL((dw_fwd_strip_kernel<TI, 3, SW, T>), dim3(grid), dim3(DW_THREADS), 0, st, p); break;
        case 5: hipLaunchKernelGGL((dw_fwd_strip_kernel<TI, 5, SW, T>), dim3(grid), dim3(DW_THREADS), 0, st, p); break;
        default: hipLaunchKernelGGL((dw_fwd_strip_kernel<TI, 7, SW, T>), dim3(grid), dim3(DW_THREADS), 0, st, p); break;
    }
}

template <typename TI, int T>
int forward(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s, Pass pass) {
    FCN_REQUIRE(h_d, FCN_E_ARG, "dwconv: null descriptor");
    const fcn_dwconv_desc& d = *h_d;
    const int rc = validate(d, pass);
    if (rc) return rc;
    FCN_REQUIRE(cfg_request >= -1 && cfg_request < DW_CFGS, FCN_E_ARG, "dwconv: unknown configuration %d", cfg_request);
    FCN_REQUIRE(cfg_request != 1 || strip_takes(d), FCN_E_UNSUPPORTED,
                "dwconv: the strip form takes stride_w 1 or 2, no dilation and kw 1 / 3 / 5 / 7 (stride_w %d, dilation %d, kw %d)", d.stride_w,
                d.dilation, d.kw);
    constexpr int S = Elem<TI>::S;
    const int ysz = pass == FWD_F16 && !(d.flags & FCN_CONV_OUT_F32) ? 2 : 4;
    // built-in choice: the strip form for stride_w 1 (neighbouring outputs share kw - 1 of kw columns; at stride 2 they share one and the
    // form only costs lanes) where the problem has lanes to spare - a quarter of them must still fill the chip
    const long long lanes1 = (long long)d.N * d.OH * d.OW * ((d.C + S - 1) / S);
    const int cfg = cfg_request >= 0 ? cfg_request : (strip_takes(d) && d.stride_w == 1 && d.kw > 1 && d.OW >= T && lanes1 >= (1 << 17)) ? 1 : 0;
    DwP p;
    fill(p, d, S, ysz);
    p.strips = (d.OW + T - 1) / T;
    const long long rows = (long long)d.N * d.OH * (cfg == 1 ? p.strips : d.OW);
    const long long items = rows * p.segs;
    FCN_REQUIRE(items < (1ll << 31), FCN_E_UNSUPPORTED, "dwconv: too many work items for one launch");
    p.items = (int)items;
    const unsigned grid = (unsigned)((items + DW_THREADS - 1) / DW_THREADS);
    if (cfg == 0) {
        if (d.kh == 3 && d.kw == 3) hipLaunchKernelGGL((dw_fwd_plain_kernel<TI, 3>), dim3(grid), dim3(DW_THREADS), 0, as_stream(s), p);
        else hipLaunchKernelGGL((dw_fwd_plain_kernel<TI, 0>), dim3(grid), dim3(DW_THREADS), 0, as_stream(s), p);
        FCN_LAUNCH_CHECK("dw_fwd_plain_kernel");
    } else {
        if (d.stride_w == 1) launch_strip_kw<TI, T, 1>(p, d.kw, grid, as_stream(s));
        else launch_strip_kw<TI, T, 2>(p, d.kw, grid, as_stream(s));
        FCN_LAUNCH_CHECK("dw_fwd_strip_kernel");
    }
    return 0;
}

// pixel splits of the weight gradient: enough workgroups to fill the chip, at least 64 pixels each
struct WgradPlan { int splits, pix_per_split, nblk_c, ngrp, ch; };
int wgrad_plan(const fcn_dwconv_desc& d, int split_request, WgradPlan* wp) {
    const long long M = (long long)d.N * d.OH * d.OW;
    FCN_REQUIRE(split_request >= 0 && split_request <= WG_MAX_SPLITS && split_request <= M, FCN_E_ARG,
                "dwconv wgrad: split request %d outside 0 .. min(%d, pixels)", split_request, WG_MAX_SPLITS);
    const int c4 = (d.C + 3) & ~3;
    wp->ch = c4 <= 16 ? 16 : c4 <= 32 ? 32 : 64;
    wp->nblk_c = (c4 + wp->ch - 1) / wp->ch;
    wp->ngrp = (d.kh * d.kw + WG_TAPS - 1) / WG_TAPS;
    long long want = split_request;
    if (want == 0) {
        const long long tiles = (long long)wp->nblk_c * wp->ngrp;
        want = (2048 + tiles - 1) / tiles;
        const long long most = (M + 63) / 64;
        if (want > most) want = most;
        if (want > WG_MAX_SPLITS) want = WG_MAX_SPLITS;
        if (want < 1) want = 1;
    }
    const long long pps = (M + want - 1) / want;
    wp->pix_per_split = (int)pps;
    wp->splits = (int)((M + pps - 1) / pps);      // (no empty split)
    return 0;
}

}  // namespace
}  // namespace fcn

using namespace fcn;

extern "C" {

int fcn_dwconv2d_num_configs(void) { return DW_CFGS; }

int fcn_dwconv2d_fwd_f32(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s) {
    return forward<float, DW_STRIP_F32>(h_d, cfg_request, s, FWD_F32);
}

int fcn_dwconv2d_fwd_f16(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s) {
    return forward<f16_t, DW_STRIP_F16>(h_d, cfg_request, s, FWD_F16);
}

int fcn_dwconv2d_dgrad_f32(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s) {
    FCN_REQUIRE(h_d, FCN_E_ARG, "dwconv dgrad: null descriptor");
    const fcn_dwconv_desc& d = *h_d;
    const int rc = validate(d, DGRAD);
    if (rc) return rc;
    FCN_REQUIRE(cfg_request >= -1 && cfg_request < DW_CFGS, FCN_E_ARG, "dwconv dgrad: unknown configuration %d", cfg_request);
    FCN_REQUIRE(cfg_request != 1, FCN_E_UNSUPPORTED, "dwconv dgrad: the strip form is forward only");
    DwP p;
    fill(p, d, 4, 4);
    const long long items = (long long)d.N * d.H * d.W * p.segs;
    FCN_REQUIRE(items < (1ll << 31), FCN_E_UNSUPPORTED, "dwconv dgrad: too many work items for one launch");
    p.items = (int)items;
    const dim3 grid((unsigned)((items + DW_THREADS - 1) / DW_THREADS));
    if (d.kh == 3 && d.kw == 3) hipLaunchKernelGGL(dw_dgrad_kernel<3>, grid, dim3(DW_THREADS), 0, as_stream(s), p);
    else hipLaunchKernelGGL(dw_dgrad_kernel<0>, grid, dim3(DW_THREADS), 0, as_stream(s), p);
    FCN_LAUNCH_CHECK("dw_dgrad_kernel");
    return 0;
}

size_t fcn_dwconv2d_wgrad_workspace_floats(const fcn_dwconv_desc* h_d, int split_request) {
    WgradPlan wp;
    if (!h_d || validate(*h_d, WGRAD) || wgrad_plan(*h_d, split_request, &wp)) return 0;
    if (wp.splits <= 1) return 0;
    return (size_t)wp.splits * (h_d->kh * h_d->kw + 1) * ((h_d->C + 3) & ~3);
}

int fcn_dwconv2d_wgrad_f32(const fcn_dwconv_desc* h_d, float* dw, float* db, float* d_workspace, int split_request, fcn_stream_t s) {
    FCN_REQUIRE(h_d && dw, FCN_E_ARG, "dwconv wgrad: null descriptor / dw");
    const fcn_dwconv_desc& d = *h_d;
    int rc = validate(d, WGRAD);
    if (rc) return rc;
    FCN_REQUIRE(((uintptr_t)dw & 15) == 0 && (!db || ((uintptr_t)db & 3) == 0), FCN_E_ALIGN, "dwconv wgrad: dw must be 16-byte, db 4-byte aligned");
    WgradPlan wp;
    rc = wgrad_plan(d, split_request, &wp);
    if (rc) return rc;
    const int c4 = (d.C + 3) & ~3, taps = d.kh * d.kw;
    const unsigned long long slab = (unsigned long long)(taps + 1) * c4;      // (the taps' rows, then db's)
    FCN_REQUIRE(wp.splits == 1 || d_workspace, FCN_E_ARG, "dwconv wgrad: %d pixel splits need a workspace", wp.splits);
    FCN_REQUIRE(wp.splits == 1 || ((uintptr_t)d_workspace & 15) == 0, FCN_E_ALIGN, "dwconv wgrad: the workspace must be 16-byte aligned");
    DwWgradP p;
    p.x = (const float*)d.x; p.dy = (const float*)d.y; p.out = wp.splits == 1 ? dw : d_workspace;
    p.db = db; p.direct = wp.splits == 1 ? 1 : 0;
    p.N = d.N; p.H = d.H; p.W = d.W; p.C = d.C; p.x_cstride = d.x_cstride; p.kh = d.kh; p.kw = d.kw;
    p.pad_h = d.pad_h; p.pad_w = d.pad_w; p.stride_h = d.stride_h; p.stride_w = d.stride_w; p.dil = d.dilation; p.OH = d.OH; p.OW = d.OW;
    p.dy_cstride = d.y_cstride; p.dy_coffset = d.y_coffset;
    p.dy_vec = (((uintptr_t)d.y & 15) == 0 && ((d.y_cstride | d.y_coffset) & 3) == 0) ? 1 : 0;
    p.C4 = c4; p.M = d.N * d.OH * d.OW; p.pix_per_split = wp.pix_per_split;
    p.slab = slab;
    const dim3 grid((unsigned)wp.nblk_c, (unsigned)wp.ngrp, (unsigned)wp.splits);
    if (wp.ch == 16) hipLaunchKernelGGL(dw_wgrad_kernel<16>, grid, dim3(DW_THREADS), 0, as_stream(s), p);
    else if (wp.ch == 32) hipLaunchKernelGGL(dw_wgrad_kernel<32>, grid, dim3(DW_THREADS), 0, as_stream(s), p);
    else hipLaunchKernelGGL(dw_wgrad_kernel<64>, grid, dim3(DW_THREADS), 0, as_stream(s), p);
    FCN_LAUNCH_CHECK("dw_wgrad_kernel");
    if (wp.splits > 1) {
        const long long dw4 = (long long)taps * c4 / 4, total4 = dw4 + (db ? c4 / 4 : 0);
        hipLaunchKernelGGL(dw_wgrad_finish_kernel, dim3((unsigned)((total4 + 3) / 4)), dim3(256), 0, as_stream(s), (const float*)d_workspace, dw, dw4,
                           total4, wp.splits, slab, db, d.C);
        FCN_LAUNCH_CHECK("dw_wgrad_finish_kernel");
    }
    return 0;
}

}  // extern "C"
