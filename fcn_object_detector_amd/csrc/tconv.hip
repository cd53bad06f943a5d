// Transposed (fractionally-strided) convolution for MI355X (gfx950): Caffe DeconvolutionLayer::Forward_gpu with group 1 and
// the data gradient of a strided ConvolutionLayer (Backward_gpu, bottom diff).
//
//   b[n, oy, ox, cb] = bias[cb] + sum over ca, r, q, iy, ix with oy + p - r == s*iy, ox + p - q == s*ix of w[ca][cb][r][q] * a[n, iy, ix, ca]
//
// No structural zero is multiplied: the outputs with ((oy + p) mod s, (ox + p) mod s) = (fy, fx) form a lattice ("phase"), and on
// it the operation is a stride-1 correlation of `a` with the taps r = fy, fy + s, ..., q = fx, fx + s, ... of the bank.  One launch
// covers every phase of every problem: grid = (pixel blocks x Cb blocks of the largest phase, phases, problems); the phases of one
// problem differ by at most one lattice row / column, so the workgroups past a smaller phase's end (they return at once) are few.
//
// A workgroup (256 threads, four waves as 2 x 2) computes 64 lattice pixels x 64 output channels as out^T = W . act^T with
// v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fma chain): A = 32 filters x 2 k, B = 2 k x 32 pixels, so a lane ends up with
// one pixel and four runs of four consecutive channels - 16-byte stores into the NHWC result.  The contraction runs over the
// phase's taps (outer) and Ca in chunks of 16 (inner); both operands are staged through LDS (64 rows x 64 bytes each, the 16-byte
// slots XOR-swizzled so the ds_read_b128 fragment reads are conflict-free) in two buffers, one barrier per chunk, the next
// chunk's global loads in flight behind the current chunk's MFMAs.  16 KiB of LDS and < 64 VGPRs per workgroup: several
// workgroups share a CU and hide each other's staging.
//
// In halves (tconv_f16_kernel, fcn_tconv2d_prepare_f16 / fcn_tconv2d_f16): the same phases, launch, loader roles and LDS
// rows over NHWC halves and the bank [kh][kw][Cb][round8(Ca)]; a 64-byte LDS row holds 32 input channels, a lane's 16-byte fragment
// is the 8 consecutive k that v_mfma_f32_32x32x16_f16 takes: two MFMAs per chunk and wave.  Float32 sums, one rounding to half (or a
// float32 result), bias and ReLU only: inference.  Two tiles: 64 lattice pixels x 64 channels (waves 2 x 2) and 128 x 32 (four waves
// of 32 x 32) for the narrow score layers.
//
// Deterministic: every output element belongs to exactly one lane of one workgroup, the contraction is never split across
// workgroups, there is no atomic.  The order of the sum depends only on the descriptor.
#include "conv_common.h"

#include <vector>

namespace fcn {
namespace {

constexpr int TC_BM = 64;       // lattice pixels per workgroup
constexpr int TC_BN = 64;       // output channels per workgroup
constexpr int TC_BK = 16;       // input channels per staged chunk
constexpr int TC_THREADS = 256;
constexpr int TC_MAX_STRIDE = 64;
constexpr int TH_BK = 32;       // halves: input channels per staged chunk (the same 64-byte LDS row)
constexpr int TH_CONFIGS = 2;   // halves: 0 = 64 lattice pixels x 64 channels, 1 = 128 lattice pixels x 32 channels
constexpr int TH_CFG_BASE = FCN_TCONV_CFG_F16;      // fcn_tconv_plan.cfg of a half plan counts from here: a plan names its element type

typedef _Float16 v4h __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

struct TConvP {
    const float* a;
    const float* w;       // packed bank [kh][kw][Cb][Ca4]
    const float* bias;
    float* b;
    const float* y2;
    int N, H, W, Ca, a_cstride, Cb, kh, kw, pad, stride, OH, OW;
    int b_cstride, b_coffset, y2_cstride, y2_coffset, flags;
    int Ca4, nblk_n, pad_;
};

// one axis of a phase: first output coordinate of the lattice, its length, the input coordinate under tap 0 at lattice index 0
// and the number of taps
struct Axis { int o0, len, t0, taps; };
__host__ __device__ inline Axis phase_axis(int f, int s, int pad, int k, int out) {
    Axis ax;
    int o0 = (f - pad) % s;
    if (o0 < 0) o0 += s;
    ax.o0 = o0;
    ax.len = o0 < out ? (out - 1 - o0) / s + 1 : 0;
    ax.t0 = (o0 + pad - f) / s;      // exact: o0 + pad == f (mod s)
    ax.taps = f < k ? (k - f + s - 1) / s : 0;
    return ax;
}

__global__ __launch_bounds__(TC_THREADS) void tconv_f32_kernel(const TConvP* __restrict__ probs) {
    const TConvP& p = probs[blockIdx.z];
    const int s = p.stride;
    const int ph = blockIdx.y;
    if (ph >= s * s) return;
    const int fy = ph / s, fx = ph - fy * s;
    const Axis ay = phase_axis(fy, s, p.pad, p.kh, p.OH), ax = phase_axis(fx, s, p.pad, p.kw, p.OW);
    const int M = p.N * ay.len * ax.len;
    const int mblk = blockIdx.x / p.nblk_n, nblk = blockIdx.x - mblk * p.nblk_n;
    if (mblk * TC_BM >= M || nblk * TC_BN >= p.Cb) return;

    __shared__ __attribute__((aligned(16))) float sW[2][TC_BN * TC_BK];
    __shared__ __attribute__((aligned(16))) float sA[2][TC_BM * TC_BK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- loader roles: row (a filter of the bank tile / a pixel of the activation tile) and 16-byte segment of the chunk
    const int lrow = tid >> 2, lseg = tid & 3;
    const int l_cb = nblk * TC_BN + lrow;
    const int l_m = mblk * TC_BM + lrow;
    int l_n = 0, l_jy = 0, l_jx = 0;
    const bool l_mok = l_m < M;
    if (l_mok) {
        l_jx = l_m % ax.len;
        const int t = l_m / ax.len;
        l_jy = t % ay.len;
        l_n = t / ay.len;
    }
    const int lds_slot = lrow * TC_BK + ((lseg ^ swz<4>(lrow)) << 2);
    const int nchunk = (p.Ca4 + TC_BK - 1) / TC_BK;
    const int total = ay.taps * ax.taps * nchunk;

    v4f regW = {0.f, 0.f, 0.f, 0.f}, regA = {0.f, 0.f, 0.f, 0.f};
    int it_mr = 0, it_mq = 0, it_c = 0;      // the chunk the NEXT fetch() loads
    auto fetch = [&]() {
        const int ca = it_c * TC_BK + lseg * 4;
        const int r = fy + s * it_mr, q = fx + s * it_mq;
        const int iy = ay.t0 + l_jy - it_mr, ix = ax.t0 + l_jx - it_mq;
        regW = v4f{0.f, 0.f, 0.f, 0.f};
        regA = v4f{0.f, 0.f, 0.f, 0.f};
        if (ca < p.Ca4) {
            if (l_cb < p.Cb) regW = *(const v4f*)(p.w + ((size_t)(r * p.kw + q) * p.Cb + l_cb) * p.Ca4 + ca);
            if (l_mok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                regA = *(const v4f*)(p.a + ((size_t)(l_n * p.H + iy) * p.W + ix) * p.a_cstride + ca);
                // channels Ca .. Ca4-1 of a pixel are padding: never multiplied, whatever they hold
                if (ca + 1 >= p.Ca) regA[1] = 0.f;
                if (ca + 2 >= p.Ca) regA[2] = 0.f;
                if (ca + 3 >= p.Ca) regA[3] = 0.f;
            }
        }
        if (++it_c == nchunk) {
            it_c = 0;
            if (++it_mq == ax.taps) { it_mq = 0; ++it_mr; }
        }
    };

    // ---- MFMA roles
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int rowW = wm * 32 + fr, rowA = wn * 32 + fr;
    int offW[2], offA[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        offW[j] = rowW * TC_BK + (((2 * j + fh) ^ swz<4>(rowW)) << 2);
        offA[j] = rowA * TC_BK + (((2 * j + fh) ^ swz<4>(rowA)) << 2);
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    if (total > 0) fetch();
#pragma unroll 1
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        *(v4f*)&sW[buf][lds_slot] = regW;
        *(v4f*)&sA[buf][lds_slot] = regA;
        if (it + 1 < total) fetch();
        __syncthreads();
        // (the buffer written in iteration it + 1 was last read in iteration it - 1, and every wave has passed this barrier
        //  only after those reads: one barrier per chunk is enough with two buffers)
        v4f wf[2], af[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wf[j] = *(const v4f*)&sW[buf][offW[j]];
            af[j] = *(const v4f*)&sA[buf][offA[j]];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j][e], af[j][e], acc, 0, 0, 0);
    }

    // ---- epilogue: lane = pixel (column of the MFMA result), registers 4g .. 4g+3 = channels 8g + 4 fh .. +3 of the wave's 32
    const int m = mblk * TC_BM + wn * 32 + fr;
    if (m >= M) return;
    const int jx = m % ax.len;
    const int t = m / ax.len;
    const int jy = t % ay.len, n = t / ay.len;
    const size_t pix = (size_t)(n * p.OH + ay.o0 + s * jy) * p.OW + ax.o0 + s * jx;
    const bool do_relu = (p.flags & FCN_CONV_RELU) != 0, do_accum = (p.flags & FCN_CONV_ACCUM) != 0;
    const bool do_mask = (p.flags & FCN_CONV_MASK) != 0;
    float* dst_px = p.b + pix * p.b_cstride + p.b_coffset;
    const float* y2_px = do_mask ? p.y2 + pix * p.y2_cstride + p.y2_coffset : nullptr;
    const bool vec_ok = ((p.b_cstride | p.b_coffset) & 3) == 0 && ((unsigned)(size_t)p.b & 15) == 0 &&
                        (!do_mask || (((p.y2_cstride | p.y2_coffset) & 3) == 0 && ((unsigned)(size_t)p.y2 & 15) == 0));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int cb = nblk * TC_BN + wm * 32 + 8 * g + 4 * fh;
        if (cb >= p.Cb) continue;
        v4f v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (vec_ok && cb + 3 < p.Cb) {
            if (p.bias) for (int e = 0; e < 4; ++e) v[e] += p.bias[cb + e];      // (the bias vector is only 4-byte aligned in general)
            if (do_accum) v += *(const v4f*)(dst_px + cb);
            if (do_relu) for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            if (do_mask) { const v4f y = *(const v4f*)(y2_px + cb); for (int e = 0; e < 4; ++e) v[e] = y[e] > 0.f ? v[e] : 0.f; }
            *(v4f*)(dst_px + cb) = v;
        } else {
            for (int e = 0; e < 4; ++e) {
                if (cb + e >= p.Cb) break;
                float x = v[e];
                if (p.bias) x += p.bias[cb + e];
                if (do_accum) x += dst_px[cb + e];
                if (do_relu) x = fmaxf(x, 0.f);
                if (do_mask) x = y2_px[cb + e] > 0.f ? x : 0.f;
                dst_px[cb + e] = x;
            }
        }
    }
}

// packed[(r * kw + q) * Cb + cb][ca] = w[ca][r][q][cb] for ca < Ca, 0 for Ca <= ca < Ca4
__global__ __launch_bounds__(256) void tconv_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int Ca, int Cb, int w_cstride,
                                                         int taps, int Ca4) {
    const long long total = (long long)taps * Cb * Ca4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ca = (int)(i % Ca4);
        const long long t = i / Ca4;
        const int cb = (int)(t % Cb);
        const int tap = (int)(t / Cb);
        packed[i] = ca < Ca ? w[((size_t)ca * taps + tap) * w_cstride + cb] : 0.f;
    }
}

// The transposed convolution in halves (fcn_tconv2d_f16): the phases, the launch, the loader roles, the swizzled 64-byte LDS rows and
// the one barrier per chunk of tconv_f32_kernel.  A row now holds 32 input channels, a thread's 16-byte load is 8 halves, and a lane's
// 16-byte fragment is the 8 consecutive k of its row that v_mfma_f32_32x32x16_f16 takes (lane half fh: k 8 fh .. 8 fh + 7 of the
// instruction's 16): two MFMAs per chunk and wave.  TConvP's a / w / b point to halves here (b to floats under FCN_CONV_OUT_F32) and
// Ca4 holds round8(Ca).  BM x BN = 64 x 64: the waves 2 x 2, a thread stages one bank row segment and one pixel segment per chunk;
// 128 x 32: four waves of 32 pixels x 32 channels, threads 0 .. 127 stage the bank, every thread two pixel segments.
template <int BM, int BN>
__global__ __launch_bounds__(TC_THREADS) void tconv_f16_kernel(const TConvP* __restrict__ probs) {
    constexpr int NA = BM / 64;       // activation rows a thread stages per chunk
    constexpr int WM = BN / 32;       // waves along the channels
    const TConvP& p = probs[blockIdx.z];
    const int s = p.stride;
    const int ph = blockIdx.y;
    if (ph >= s * s) return;
    const int fy = ph / s, fx = ph - fy * s;
    const Axis ay = phase_axis(fy, s, p.pad, p.kh, p.OH), ax = phase_axis(fx, s, p.pad, p.kw, p.OW);
    const int M = p.N * ay.len * ax.len;
    const int mblk = blockIdx.x / p.nblk_n, nblk = blockIdx.x - mblk * p.nblk_n;
    if (mblk * BM >= M || nblk * BN >= p.Cb) return;

    __shared__ __attribute__((aligned(16))) f16_t sW[2][BN * TH_BK];
    __shared__ __attribute__((aligned(16))) f16_t sA[2][BM * TH_BK];

    const f16_t* ah = reinterpret_cast<const f16_t*>(p.a);
    const f16_t* wh = reinterpret_cast<const f16_t*>(p.w);
    const int Ca8 = p.Ca4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- loader roles: row (a filter of the bank tile / a pixel of the activation tile) and 16-byte segment of the chunk
    const int lrow = tid >> 2, lseg = tid & 3;
    const bool l_wok = lrow < BN && nblk * BN + lrow < p.Cb;
    const int l_cb = nblk * BN + lrow;
    int l_n[NA], l_jy[NA], l_jx[NA];
    bool l_mok[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int l_m = mblk * BM + lrow + 64 * i;
        l_mok[i] = l_m < M;
        l_n[i] = l_jy[i] = l_jx[i] = 0;
        if (l_mok[i]) {
            l_jx[i] = l_m % ax.len;
            const int t = l_m / ax.len;
            l_jy[i] = t % ay.len;
            l_n[i] = t / ay.len;
        }
    }
    const int lds_slot = lrow * TH_BK + ((lseg ^ swz<4>(lrow)) << 3);      // (row + 64 has the same swizzle)
    const int nchunk = (Ca8 + TH_BK - 1) / TH_BK;
    const int total = ay.taps * ax.taps * nchunk;

    const v8h zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    v8h regW = zero8, regA[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) regA[i] = zero8;
    int it_mr = 0, it_mq = 0, it_c = 0;      // the chunk the NEXT fetch() loads
    auto fetch = [&]() {
        const int ca = it_c * TH_BK + lseg * 8;
        const int r = fy + s * it_mr, q = fx + s * it_mq;
        regW = zero8;
#pragma unroll
        for (int i = 0; i < NA; ++i) regA[i] = zero8;
        if (ca < Ca8) {
            if (l_wok) regW = *(const v8h*)(wh + ((size_t)(r * p.kw + q) * p.Cb + l_cb) * Ca8 + ca);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int iy = ay.t0 + l_jy[i] - it_mr, ix = ax.t0 + l_jx[i] - it_mq;
                if (l_mok[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                    regA[i] = *(const v8h*)(ah + ((size_t)(l_n[i] * p.H + iy) * p.W + ix) * p.a_cstride + ca);
                    // channels Ca .. Ca8-1 of a pixel are padding: never multiplied, whatever they hold
#pragma unroll
                    for (int e = 1; e < 8; ++e)
                        if (ca + e >= p.Ca) regA[i][e] = (f16_t)0.f;
                }
            }
        }
        if (++it_c == nchunk) {
            it_c = 0;
            if (++it_mq == ax.taps) { it_mq = 0; ++it_mr; }
        }
    };

    // ---- MFMA roles
    const int wm = wave % WM, wn = wave / WM;
    const int fr = lane & 31, fh = lane >> 5;
    const int rowW = wm * 32 + fr, rowA = wn * 32 + fr;
    int offW[2], offA[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {      // MFMA j contracts k 16 j .. 16 j + 15 of the chunk: slots 2 j and 2 j + 1, one per lane half
        offW[j] = rowW * TH_BK + (((2 * j + fh) ^ swz<4>(rowW)) << 3);
        offA[j] = rowA * TH_BK + (((2 * j + fh) ^ swz<4>(rowA)) << 3);
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    if (total > 0) fetch();
#pragma unroll 1
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        if (lrow < BN) *(v8h*)&sW[buf][lds_slot] = regW;
#pragma unroll
        for (int i = 0; i < NA; ++i) *(v8h*)&sA[buf][lds_slot + 64 * i * TH_BK] = regA[i];
        if (it + 1 < total) fetch();
        __syncthreads();      // (two buffers, one barrier per chunk: as in tconv_f32_kernel)
        v8h wf[2], af[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wf[j] = *(const v8h*)&sW[buf][offW[j]];
            af[j] = *(const v8h*)&sA[buf][offA[j]];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], af[j], acc, 0, 0, 0);
    }

    // ---- epilogue: the result layout of tconv_f32_kernel - lane = pixel, registers 4g .. 4g+3 = channels 8g + 4 fh .. +3 of the wave's 32
    const int m = mblk * BM + wn * 32 + fr;
    if (m >= M) return;
    const int jx = m % ax.len;
    const int t = m / ax.len;
    const int jy = t % ay.len, n = t / ay.len;
    const size_t pix = (size_t)(n * p.OH + ay.o0 + s * jy) * p.OW + ax.o0 + s * jx;
    const bool do_relu = (p.flags & FCN_CONV_RELU) != 0, out32 = (p.flags & FCN_CONV_OUT_F32) != 0;
    float* dst32 = reinterpret_cast<float*>(p.b) + pix * p.b_cstride + p.b_coffset;
    f16_t* dst16 = reinterpret_cast<f16_t*>(p.b) + pix * p.b_cstride + p.b_coffset;
    // bias and ReLU on the lane's own four runs of four channels
    const int cbase = nblk * BN + wm * 32;
    v4f v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int cb = cbase + 8 * g + 4 * fh;
        v[g] = v4f{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p.bias && cb + e < p.Cb) v[g][e] += p.bias[cb + e];
            if (do_relu) v[g][e] = fmaxf(v[g][e], 0.f);
        }
    }
    if (!out32 && ((p.b_cstride | p.b_coffset) & 7) == 0 && ((unsigned)(size_t)p.b & 15) == 0) {
        // 16-byte stores of halves: the two lanes of a pixel (fh = 0, 1; the same m, so both are here) trade runs - of the 16 channels
        // of runs 2 gp and 2 gp + 1, lane fh = 0 ends up with the first eight and lane fh = 1 with the last eight
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            const v4f a = v[2 * gp], b = v[2 * gp + 1];
            const v4h own0 = {(f16_t)a[0], (f16_t)a[1], (f16_t)a[2], (f16_t)a[3]};      // round to nearest even, once
            const v4h own1 = {(f16_t)b[0], (f16_t)b[1], (f16_t)b[2], (f16_t)b[3]};
            const v2i send = __builtin_bit_cast(v2i, fh ? own0 : own1);
            const v2i got = {__shfl_xor(send[0], 32), __shfl_xor(send[1], 32)};
            const v4h recv = __builtin_bit_cast(v4h, got);
            const v4h lo = fh ? recv : own0, hi = fh ? own1 : recv;
            const v8h out = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            const int cb8 = cbase + 16 * gp + 8 * fh;
            if (cb8 + 7 < p.Cb) {
                *(v8h*)(dst16 + cb8) = out;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (cb8 + e < p.Cb) dst16[cb8 + e] = out[e];
            }
        }
        return;
    }
    // otherwise a run of four channels is one store where it is aligned as a whole: 16 bytes of floats, 8 bytes of halves
    const bool vec_ok = ((p.b_cstride | p.b_coffset) & 3) == 0 && ((unsigned)(size_t)p.b & (out32 ? 15 : 7)) == 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int cb = cbase + 8 * g + 4 * fh;
        if (cb >= p.Cb) continue;
        const int run = min(4, p.Cb - cb);
        if (vec_ok && run == 4) {
            if (out32) {
                *(v4f*)(dst32 + cb) = v[g];
            } else {
                const v4h h = {(f16_t)v[g][0], (f16_t)v[g][1], (f16_t)v[g][2], (f16_t)v[g][3]};      // round to nearest even, once
                *(v4h*)(dst16 + cb) = h;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= run) break;
                if (out32) dst32[cb + e] = v[g][e];
                else dst16[cb + e] = (f16_t)v[g][e];      // a 2-byte store: the half that shares the word is not touched
            }
        }
    }
}

// the bank in halves: packed[(r * kw + q) * Cb + cb][ca] = w[ca][r][q][cb] for ca < Ca, 0 for Ca <= ca < Ca8
__global__ __launch_bounds__(256) void tconv_pack_f16_kernel(const f16_t* __restrict__ w, f16_t* __restrict__ packed, int Ca, int Cb, int w_cstride,
                                                             int taps, int Ca8) {
    const long long total = (long long)taps * Cb * Ca8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ca = (int)(i % Ca8);
        const long long t = i / Ca8;
        const int cb = (int)(t % Cb);
        const int tap = (int)(t / Cb);
        packed[i] = ca < Ca ? w[((size_t)ca * taps + tap) * w_cstride + cb] : (f16_t)0.f;
    }
}

// db[c] = sum over pixels of dy[pixel][c]: one workgroup per channel, every thread a strided run of pixels in ascending order,
// then a binary tree over the 256 partial sums - the same order on every run
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ dy, float* __restrict__ db, int pixels, int cstride, int coffset) {
    __shared__ float part[256];
    const int c = blockIdx.x;
    float sum = 0.f;
    for (int i = threadIdx.x; i < pixels; i += 256) sum += dy[(size_t)i * cstride + coffset + c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) db[c] = part[0];
}

// half = true: the descriptor of fcn_tconv2d_prepare_f16 (a, w and b point to halves, b to floats under FCN_CONV_OUT_F32)
int validate(const fcn_tconv_desc& d, bool half = false) {
    FCN_REQUIRE(d.a && d.w && d.b, FCN_E_ARG, "tconv: null a/w/b");
    FCN_REQUIRE(d.N > 0 && d.H > 0 && d.W > 0 && d.Ca > 0 && d.Cb > 0 && d.kh > 0 && d.kw > 0 && d.stride > 0 && d.pad >= 0, FCN_E_ARG,
                "tconv: non-positive extent");
    FCN_REQUIRE(d.stride <= TC_MAX_STRIDE, FCN_E_UNSUPPORTED, "tconv: stride %d above %d", d.stride, TC_MAX_STRIDE);
    FCN_REQUIRE(d.pad < d.kh && d.pad < d.kw, FCN_E_UNSUPPORTED, "tconv: pad %d must stay below the kernel extent %dx%d", d.pad, d.kh, d.kw);
    FCN_REQUIRE(d.kh * d.kw <= 4096, FCN_E_UNSUPPORTED, "tconv: kernel window %dx%d too large", d.kh, d.kw);      // (64 x 64: the x32 upsampling of FCN-32s)
    const int vec = half ? 8 : 4;      // elements of a 16-byte load
    const int ca4 = (d.Ca + vec - 1) & ~(vec - 1);
    FCN_REQUIRE(d.a_cstride % vec == 0 && d.a_cstride >= ca4, FCN_E_ALIGN, "tconv: a_cstride (%d) must be a multiple of %d holding Ca (%d) padded to %d",
                d.a_cstride, vec, d.Ca, vec);
    FCN_REQUIRE(((uintptr_t)d.a & 15) == 0 && ((uintptr_t)d.w & 15) == 0, FCN_E_ALIGN, "tconv: a / w must be 16-byte aligned");
    if (half && !(d.flags & FCN_CONV_OUT_F32))
        FCN_REQUIRE(((uintptr_t)d.b & 1) == 0 && (!d.bias || ((uintptr_t)d.bias & 3) == 0), FCN_E_ALIGN, "tconv: b must be 2-byte, bias 4-byte aligned");
    else
        FCN_REQUIRE(((uintptr_t)d.b & 3) == 0 && (!d.bias || ((uintptr_t)d.bias & 3) == 0), FCN_E_ALIGN, "tconv: b / bias must be 4-byte aligned");
    const long long oh0 = (long long)d.stride * (d.H - 1) + d.kh - 2 * d.pad, ow0 = (long long)d.stride * (d.W - 1) + d.kw - 2 * d.pad;
    FCN_REQUIRE(oh0 > 0 && ow0 > 0, FCN_E_ARG, "tconv: empty output");
    FCN_REQUIRE(d.OH >= oh0 && d.OH < oh0 + d.stride && d.OW >= ow0 && d.OW < ow0 + d.stride, FCN_E_ARG,
                "tconv: OH/OW (%d,%d) outside [s(H-1)+k-2p, s(H-1)+k-2p+s-1] = [%lld..%lld, %lld..%lld]", d.OH, d.OW, oh0, oh0 + d.stride - 1, ow0,
                ow0 + d.stride - 1);
    FCN_REQUIRE(d.b_coffset >= 0 && d.b_cstride >= d.b_coffset + d.Cb, FCN_E_ARG, "tconv: output slice exceeds b_cstride");
    if (half) {      // the training epilogues stay float32
        FCN_REQUIRE((d.flags & ~(FCN_CONV_RELU | FCN_CONV_OUT_F32)) == 0 && !d.y2, FCN_E_UNSUPPORTED,
                    "tconv: flags 0x%x outside FCN_CONV_RELU | FCN_CONV_OUT_F32, or y2 set (half floats: forward only)", d.flags);
    } else {
        FCN_REQUIRE((d.flags & ~(FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK)) == 0, FCN_E_UNSUPPORTED,
                    "tconv: flags 0x%x outside FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK (float32 only)", d.flags);
        if (d.flags & FCN_CONV_MASK)
            FCN_REQUIRE(d.y2 && ((uintptr_t)d.y2 & 3) == 0 && d.y2_coffset >= 0 && d.y2_cstride >= d.y2_coffset + d.Cb, FCN_E_ARG,
                        "tconv: FCN_CONV_MASK needs y2 with a slice of Cb channels");
    }
    FCN_REQUIRE((long long)d.N * d.H * d.W * d.a_cstride < (1ll << 31) && (long long)d.N * d.OH * d.OW * d.b_cstride < (1ll << 31) &&
                    (long long)d.kh * d.kw * d.Cb * ca4 < (1ll << 31) &&
                    (half || !(d.flags & FCN_CONV_MASK) || (long long)d.N * d.OH * d.OW * d.y2_cstride < (1ll << 31)),
                FCN_E_UNSUPPORTED, "tconv: tensor too large for 32-bit element offsets");
    return 0;
}

// grid.x of one problem: the largest phase's pixel blocks x channel blocks
long long tiles_x(const fcn_tconv_desc& d, int bm = TC_BM, int bn = TC_BN) {
    const long long ph = (d.OH + d.stride - 1) / d.stride, pw = (d.OW + d.stride - 1) / d.stride;
    return ((long long)d.N * ph * pw + bm - 1) / bm * ((d.Cb + bn - 1) / bn);
}

// the tile of a half configuration
inline int th_bm(int cfg) { return cfg == 1 ? 128 : 64; }
inline int th_bn(int cfg) { return cfg == 1 ? 32 : 64; }

}  // namespace
}  // namespace fcn

using namespace fcn;

extern "C" {

int fcn_tconv2d_num_configs(void) { return 1; }
int fcn_tconv2d_num_configs_f16(void) { return TH_CONFIGS; }

size_t fcn_tconv2d_workspace_bytes(const fcn_tconv_desc* h_descs, int n) {
    (void)h_descs;
    return n > 0 ? (size_t)n * sizeof(TConvP) : 0;
}

size_t fcn_tconv_bank_floats(int Ca, int Cb, int kh, int kw) {
    if (Ca <= 0 || Cb <= 0 || kh <= 0 || kw <= 0) return 0;
    return (size_t)kh * kw * Cb * ((Ca + 3) & ~3);
}

size_t fcn_tconv_bank_halves(int Ca, int Cb, int kh, int kw) {
    if (Ca <= 0 || Cb <= 0 || kh <= 0 || kw <= 0) return 0;
    return (size_t)kh * kw * Cb * ((Ca + 7) & ~7);
}

// half: the configuration holds for the whole plan (one launch); -1 takes the narrow tile when no problem has more than 32 output
// channels - the score layers of the FCN nets - and the square one otherwise
static int tconv_prepare(const fcn_tconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_tconv_plan* h_out, bool half) {
    FCN_REQUIRE(h_descs && h_out && n > 0, FCN_E_ARG, "tconv prepare: null descriptors / plan or n <= 0");
    FCN_REQUIRE(n <= 65535, FCN_E_UNSUPPORTED, "tconv prepare: more than 65535 problems");
    FCN_REQUIRE(cfg_request >= -1 && cfg_request < (half ? TH_CONFIGS : fcn_tconv2d_num_configs()), FCN_E_ARG, "tconv prepare: unknown configuration %d",
                cfg_request);
    for (int i = 0; i < n; ++i) {
        const int rc = validate(h_descs[i], half);
        if (rc) return rc;
    }
    int cfg = 0;
    if (half) {
        cfg = cfg_request;
        if (cfg < 0) {
            cfg = 1;
            for (int i = 0; i < n; ++i)
                if (h_descs[i].Cb > 32) cfg = 0;
        }
    }
    const int bm = half ? th_bm(cfg) : TC_BM, bn = half ? th_bn(cfg) : TC_BN;
    long long gx = 0, total = 0;
    int gy = 0;
    for (int i = 0; i < n; ++i) {
        const long long tx = tiles_x(h_descs[i], bm, bn);
        const int phases = h_descs[i].stride * h_descs[i].stride;
        gx = tx > gx ? tx : gx;
        gy = phases > gy ? phases : gy;
        total += tx * phases;
    }
    FCN_REQUIRE(gx < (1ll << 31) && total < (1ll << 31), FCN_E_UNSUPPORTED, "tconv prepare: too many tiles for one launch");
    FCN_REQUIRE(d_workspace, FCN_E_ARG, "tconv prepare: null workspace");
    std::vector<TConvP> ps((size_t)n);
    for (int i = 0; i < n; ++i) {
        const fcn_tconv_desc& d = h_descs[i];
        TConvP& p = ps[(size_t)i];
        p.a = d.a; p.w = d.w; p.bias = d.bias; p.b = d.b; p.y2 = (d.flags & FCN_CONV_MASK) ? d.y2 : nullptr;
        p.N = d.N; p.H = d.H; p.W = d.W; p.Ca = d.Ca; p.a_cstride = d.a_cstride; p.Cb = d.Cb; p.kh = d.kh; p.kw = d.kw;
        p.pad = d.pad; p.stride = d.stride; p.OH = d.OH; p.OW = d.OW;
        p.b_cstride = d.b_cstride; p.b_coffset = d.b_coffset; p.y2_cstride = d.y2_cstride; p.y2_coffset = d.y2_coffset; p.flags = d.flags;
        p.Ca4 = half ? (d.Ca + 7) & ~7 : (d.Ca + 3) & ~3;
        p.nblk_n = (d.Cb + bn - 1) / bn;
        p.pad_ = 0;
    }
    FCN_HIP(hipMemcpy(d_workspace, ps.data(), ps.size() * sizeof(TConvP), hipMemcpyHostToDevice));
    h_out->d_probs = d_workspace;
    h_out->n = n;
    h_out->cfg = half ? TH_CFG_BASE + cfg : 0;
    h_out->grid_x = (int32_t)gx;
    h_out->grid_y = gy;
    h_out->total_tiles = (int32_t)total;
    return 0;
}

int fcn_tconv2d_prepare(const fcn_tconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_tconv_plan* h_out) {
    return tconv_prepare(h_descs, n, d_workspace, cfg_request, h_out, false);
}

int fcn_tconv2d_prepare_f16(const fcn_tconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_tconv_plan* h_out) {
    return tconv_prepare(h_descs, n, d_workspace, cfg_request, h_out, true);
}

int fcn_tconv2d_f32(const fcn_tconv_plan* h_plan, fcn_stream_t s) {
    FCN_REQUIRE(h_plan && h_plan->d_probs && h_plan->n > 0 && h_plan->grid_x > 0 && h_plan->grid_y > 0 && h_plan->grid_y <= TC_MAX_STRIDE * TC_MAX_STRIDE &&
                    h_plan->n <= 65535 && h_plan->cfg == 0,
                FCN_E_ARG, "tconv: the plan was not filled by fcn_tconv2d_prepare");
    hipLaunchKernelGGL(tconv_f32_kernel, dim3((unsigned)h_plan->grid_x, (unsigned)h_plan->grid_y, (unsigned)h_plan->n), dim3(TC_THREADS), 0, as_stream(s),
                       (const TConvP*)h_plan->d_probs);
    FCN_LAUNCH_CHECK("tconv_f32_kernel");
    return 0;
}

int fcn_tconv2d_f16(const fcn_tconv_plan* h_plan, fcn_stream_t s) {
    FCN_REQUIRE(h_plan && h_plan->d_probs && h_plan->n > 0 && h_plan->grid_x > 0 && h_plan->grid_y > 0 && h_plan->grid_y <= TC_MAX_STRIDE * TC_MAX_STRIDE &&
                    h_plan->n <= 65535 && h_plan->cfg >= TH_CFG_BASE && h_plan->cfg < TH_CFG_BASE + TH_CONFIGS,
                FCN_E_ARG, "tconv: the plan was not filled by fcn_tconv2d_prepare_f16");
    const dim3 grid((unsigned)h_plan->grid_x, (unsigned)h_plan->grid_y, (unsigned)h_plan->n);
    if (h_plan->cfg - TH_CFG_BASE == 1)
        hipLaunchKernelGGL((tconv_f16_kernel<128, 32>), grid, dim3(TC_THREADS), 0, as_stream(s), (const TConvP*)h_plan->d_probs);
    else
        hipLaunchKernelGGL((tconv_f16_kernel<64, 64>), grid, dim3(TC_THREADS), 0, as_stream(s), (const TConvP*)h_plan->d_probs);
    FCN_LAUNCH_CHECK("tconv_f16_kernel");
    return 0;
}

int fcn_tconv_bank_pack_f16(const void* w, void* packed, int Ca, int Cb, int w_cstride, int kh, int kw, fcn_stream_t s) {
    FCN_REQUIRE(w && packed, FCN_E_ARG, "tconv pack: null w / packed");
    FCN_REQUIRE(Ca > 0 && Cb > 0 && kh > 0 && kw > 0, FCN_E_ARG, "tconv pack: non-positive extent");
    FCN_REQUIRE(w_cstride >= Cb, FCN_E_ARG, "tconv pack: w_cstride (%d) below Cb (%d)", w_cstride, Cb);
    FCN_REQUIRE(((uintptr_t)w & 1) == 0 && ((uintptr_t)packed & 15) == 0, FCN_E_ALIGN, "tconv pack: w must be 2-byte, packed 16-byte aligned");
    const int ca8 = (Ca + 7) & ~7;
    FCN_REQUIRE((long long)kh * kw * Cb * ca8 < (1ll << 31) && (long long)Ca * kh * kw * w_cstride < (1ll << 31), FCN_E_UNSUPPORTED,
                "tconv pack: bank too large for 32-bit element offsets");
    const long long total = (long long)kh * kw * Cb * ca8;
    hipLaunchKernelGGL(tconv_pack_f16_kernel, dim3((unsigned)stream_grid(total, 256)), dim3(256), 0, as_stream(s), (const f16_t*)w, (f16_t*)packed, Ca, Cb,
                       w_cstride, kh * kw, ca8);
    FCN_LAUNCH_CHECK("tconv_pack_f16_kernel");
    return 0;
}

int fcn_tconv_bank_pack_f32(const float* w, float* packed, int Ca, int Cb, int w_cstride, int kh, int kw, fcn_stream_t s) {
    FCN_REQUIRE(w && packed, FCN_E_ARG, "tconv pack: null w / packed");
    FCN_REQUIRE(Ca > 0 && Cb > 0 && kh > 0 && kw > 0, FCN_E_ARG, "tconv pack: non-positive extent");
    FCN_REQUIRE(w_cstride >= Cb, FCN_E_ARG, "tconv pack: w_cstride (%d) below Cb (%d)", w_cstride, Cb);
    FCN_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)packed & 15) == 0, FCN_E_ALIGN, "tconv pack: w must be 4-byte, packed 16-byte aligned");
    const int ca4 = (Ca + 3) & ~3;
    FCN_REQUIRE((long long)kh * kw * Cb * ca4 < (1ll << 31) && (long long)Ca * kh * kw * w_cstride < (1ll << 31), FCN_E_UNSUPPORTED,
                "tconv pack: bank too large for 32-bit element offsets");
    const long long total = (long long)kh * kw * Cb * ca4;
    hipLaunchKernelGGL(tconv_pack_kernel, dim3((unsigned)stream_grid(total, 256)), dim3(256), 0, as_stream(s), w, packed, Ca, Cb, w_cstride, kh * kw, ca4);
    FCN_LAUNCH_CHECK("tconv_pack_kernel");
    return 0;
}

int fcn_channel_sum_f32(const float* dy, float* db, int pixels, int C, int cstride, int coffset, fcn_stream_t s) {
    FCN_REQUIRE(dy && db, FCN_E_ARG, "channel sum: null dy / db");
    FCN_REQUIRE(pixels > 0 && C > 0 && C <= 65535 * 16 && coffset >= 0 && cstride >= coffset + C, FCN_E_ARG, "channel sum: bad extent / slice");
    FCN_REQUIRE(((uintptr_t)dy & 3) == 0 && ((uintptr_t)db & 3) == 0, FCN_E_ALIGN, "channel sum: pointers must be 4-byte aligned");
    FCN_REQUIRE((long long)pixels * cstride < (1ll << 31), FCN_E_UNSUPPORTED, "channel sum: tensor too large for 32-bit element offsets");
    hipLaunchKernelGGL(channel_sum_kernel, dim3((unsigned)C), dim3(256), 0, as_stream(s), dy, db, pixels, cstride, coffset);
    FCN_LAUNCH_CHECK("channel_sum_kernel");
    return 0;
}

}  // extern "C"
