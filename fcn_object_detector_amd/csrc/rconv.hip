// Dilated and rectangular convolution for MI355X (gfx950): Caffe ConvolutionLayer with convolution_param { dilation: d } - the conv5 /
// fc6 layers of DeepLab-LargeFOV, the four branches of the DeepLab-v2 ASPP head - and Caffe ConvolutionLayer whose two spatial axes
// differ in kernel extent, pad or stride - the 1x7 / 7x1 and 1x3 / 3x1 pairs of Inception-v3 / v4, the k x 1 + 1 x k pairs of ENet /
// ERFNet and of large-kernel segmentation heads - forward, data gradient and weight gradient, with one dilation for both axes.
//
//   y[n, oy, ox, co] = bias[co] + sum over ci, r, q of w[co][r][q][ci] * x[n, oy*sh - ph + r*dil, ox*sw - pw + q*dil, ci]
//
// One kernel family behind one ABI: fcn_rconv2d_* keeps the geometry per axis, and a square dilated layer is
// its case with equal axes.
//
// Forward / data gradient (rconv_f32_kernel): a workgroup (256 threads, four waves as 2 x 2) computes 64 output pixels x 64 output
// channels as out^T = W . act^T with v_mfma_f32_32x32x2_f32 (exact f32, a k-ordered fma chain): A = 32 filters x 2 k, B = 2 k x 32
// pixels, so a lane ends up with one pixel and four runs of four consecutive channels - 16-byte stores into the NHWC result.  The
// contraction runs over the taps (outer, rows then columns) and Cin in chunks of 16 (inner); the bank is read where the Convolution's
// parameter blob lies ([Cout][kh][kw][round4(Cin)]: a filter tap is a contiguous row), both operands are staged through LDS (64 rows
// x 64 bytes each, 16-byte slots XOR-swizzled) in two buffers, one barrier per chunk, the next chunk's global loads in flight behind
// the current chunk's MFMAs.  A tap that falls outside the image contributes staged zeros.  16 KiB of LDS.  One launch covers every
// problem of a plan: grid = (pixel blocks x Cout blocks of the largest problem, 1, problems).
//
// Forward in halves (rconv_f16_kernel, fcn_rconv2d_prepare_f16 / fcn_rconv2d_f16): the same tile, loader roles and LDS
// layout over NHWC halves and the bank [Cout][kh][kw][round8(Cin)]; a 64-byte LDS row holds 32 input channels, a lane's 16-byte
// fragment is the 8 consecutive k that v_mfma_f32_32x32x16_f16 takes: two MFMAs per chunk and wave.  Float32 sums, one rounding to
// half (or a float32 result), bias and ReLU only: inference.
//
// Weight gradient (rconv_wgrad_kernel): per tap, dw[co][tap][ci] = sum over pixels of dy[pixel][co] * x[pixel under the tap][ci]: a
// workgroup computes 64 Cout x 64 Cin of one tap over one split of the pixels, 16 pixels per staged chunk.  16 KiB of LDS.  With one
// split the result goes straight to dw; otherwise every split writes its own slab of the workspace and rconv_wgrad_finish_kernel adds
// the slabs in ascending order.  That second launch also sums db, one workgroup per channel.
//
// Deterministic: every output element belongs to exactly one lane of one workgroup, the order of every sum depends only on the
// descriptor, there is no atomic.
#include "conv_common.h"

#include <vector>

namespace fcn {
namespace {

constexpr int RC_BM = 64;       // output pixels per workgroup
constexpr int RC_BN = 64;       // output channels per workgroup
constexpr int RC_BK = 16;       // input channels per staged chunk
constexpr int RC_THREADS = 256;
constexpr int RW_BP = 16;       // weight gradient: pixels per staged chunk
constexpr int RW_MAX_SPLITS = 64;
constexpr int RC_CONFIGS = 1;   // tile configurations: 64 pixels x 64 channels x 16 k
constexpr int RH_BK = 32;       // halves: input channels per staged chunk (the same 64-byte LDS row)
constexpr int RH_CONFIGS = 1;   // halves: 64 pixels x 64 channels x 32 k
constexpr int RH_CFG_BASE = FCN_RCONV_CFG_F16;      // fcn_rconv_plan.cfg of a half plan counts from here: a plan names its element type

typedef _Float16 v4h __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

struct RConvP {
    const float* x;
    const float* w;       // [Cout][kh][kw][Cin4]
    const float* bias;
    float* y;
    const float* y2;
    int N, H, W, Cin, x_cstride, Cout, kh, kw, pad_h, pad_w, stride_h, stride_w, dil, OH, OW;
    int y_cstride, y_coffset, y2_cstride, y2_coffset, flags;
    int Cin4, nblk_n, M;
};

__global__ __launch_bounds__(RC_THREADS) void rconv_f32_kernel(const RConvP* __restrict__ probs) {
    const RConvP& p = probs[blockIdx.z];
    const int M = p.M;
    const int mblk = blockIdx.x / p.nblk_n, nblk = blockIdx.x - mblk * p.nblk_n;
    if (mblk * RC_BM >= M) return;

    __shared__ __attribute__((aligned(16))) float sW[2][RC_BN * RC_BK];
    __shared__ __attribute__((aligned(16))) float sA[2][RC_BM * RC_BK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- loader roles: row (a filter of the bank tile / a pixel of the activation tile) and 16-byte segment of the chunk
    const int lrow = tid >> 2, lseg = tid & 3;
    const int l_co = nblk * RC_BN + lrow;
    const int l_m = mblk * RC_BM + lrow;
    int l_n = 0, l_y0 = 0, l_x0 = 0;      // image, input row / column under tap (0, 0)
    const bool l_mok = l_m < M;
    if (l_mok) {
        const int ox = l_m % p.OW;
        const int t = l_m / p.OW;
        l_y0 = (t % p.OH) * p.stride_h - p.pad_h;
        l_x0 = ox * p.stride_w - p.pad_w;
        l_n = t / p.OH;
    }
    const int lds_slot = lrow * RC_BK + ((lseg ^ swz<4>(lrow)) << 2);
    const int nchunk = (p.Cin4 + RC_BK - 1) / RC_BK;
    const int total = p.kh * p.kw * nchunk;

    v4f regW = {0.f, 0.f, 0.f, 0.f}, regA = {0.f, 0.f, 0.f, 0.f};
    int it_r = 0, it_q = 0, it_c = 0;      // the chunk the NEXT fetch() loads
    auto fetch = [&]() {
        const int ci = it_c * RC_BK + lseg * 4;
        const int iy = l_y0 + it_r * p.dil, ix = l_x0 + it_q * p.dil;
        regW = v4f{0.f, 0.f, 0.f, 0.f};
        regA = v4f{0.f, 0.f, 0.f, 0.f};
        if (ci < p.Cin4) {
            if (l_co < p.Cout) regW = *(const v4f*)(p.w + ((size_t)(l_co * p.kh + it_r) * p.kw + it_q) * p.Cin4 + ci);
            if (l_mok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                regA = *(const v4f*)(p.x + ((size_t)(l_n * p.H + iy) * p.W + ix) * p.x_cstride + ci);
                // channels Cin .. Cin4-1 of a pixel are padding: never multiplied, whatever they hold
                if (ci + 1 >= p.Cin) regA[1] = 0.f;
                if (ci + 2 >= p.Cin) regA[2] = 0.f;
                if (ci + 3 >= p.Cin) regA[3] = 0.f;
            }
        }
        if (++it_c == nchunk) {
            it_c = 0;
            if (++it_q == p.kw) { it_q = 0; ++it_r; }
        }
    };

    // ---- MFMA roles
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int rowW = wm * 32 + fr, rowA = wn * 32 + fr;
    int offW[2], offA[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        offW[j] = rowW * RC_BK + (((2 * j + fh) ^ swz<4>(rowW)) << 2);
        offA[j] = rowA * RC_BK + (((2 * j + fh) ^ swz<4>(rowA)) << 2);
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    fetch();
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
    const int m = mblk * RC_BM + wn * 32 + fr;
    if (m >= M) return;
    const size_t pix = (size_t)m;      // m enumerates (n, oy, ox) in memory order
    const bool do_relu = (p.flags & FCN_CONV_RELU) != 0, do_accum = (p.flags & FCN_CONV_ACCUM) != 0;
    const bool do_mask = (p.flags & FCN_CONV_MASK) != 0;
    float* dst_px = p.y + pix * p.y_cstride + p.y_coffset;
    const float* y2_px = do_mask ? p.y2 + pix * p.y2_cstride + p.y2_coffset : nullptr;
    const bool vec_ok = ((p.y_cstride | p.y_coffset) & 3) == 0 && ((unsigned)(size_t)p.y & 15) == 0 &&
                        (!do_mask || (((p.y2_cstride | p.y2_coffset) & 3) == 0 && ((unsigned)(size_t)p.y2 & 15) == 0));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = nblk * RC_BN + wm * 32 + 8 * g + 4 * fh;
        if (co >= p.Cout) continue;
        v4f v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        if (vec_ok && co + 3 < p.Cout) {
            if (p.bias) for (int e = 0; e < 4; ++e) v[e] += p.bias[co + e];      // (the bias vector is only 4-byte aligned in general)
            if (do_accum) v += *(const v4f*)(dst_px + co);
            if (do_relu) for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            if (do_mask) { const v4f y = *(const v4f*)(y2_px + co); for (int e = 0; e < 4; ++e) v[e] = y[e] > 0.f ? v[e] : 0.f; }
            *(v4f*)(dst_px + co) = v;
        } else {
            for (int e = 0; e < 4; ++e) {
                if (co + e >= p.Cout) break;
                float x = v[e];
                if (p.bias) x += p.bias[co + e];
                if (do_accum) x += dst_px[co + e];
                if (do_relu) x = fmaxf(x, 0.f);
                if (do_mask) x = y2_px[co + e] > 0.f ? x : 0.f;
                dst_px[co + e] = x;
            }
        }
    }
}

// The forward in halves (fcn_rconv2d_f16): the tile, the loader roles, the swizzled 64-byte LDS rows and the one barrier per chunk of
// rconv_f32_kernel.  A row now holds 32 input channels, a thread's 16-byte load is 8 halves, and a lane's 16-byte fragment is the 8
// consecutive k of its row that v_mfma_f32_32x32x16_f16 takes (lane half fh: k 8 fh .. 8 fh + 7 of the instruction's 16): two MFMAs
// per chunk and wave.  RConvP's x / w / y point to halves here (y to floats under FCN_CONV_OUT_F32) and Cin4 holds round8(Cin).
__global__ __launch_bounds__(RC_THREADS) void rconv_f16_kernel(const RConvP* __restrict__ probs) {
    const RConvP& p = probs[blockIdx.z];
    const int M = p.M;
    const int mblk = blockIdx.x / p.nblk_n, nblk = blockIdx.x - mblk * p.nblk_n;
    if (mblk * RC_BM >= M) return;

    __shared__ __attribute__((aligned(16))) f16_t sW[2][RC_BN * RH_BK];
    __shared__ __attribute__((aligned(16))) f16_t sA[2][RC_BM * RH_BK];

    const f16_t* xh = reinterpret_cast<const f16_t*>(p.x);
    const f16_t* wh = reinterpret_cast<const f16_t*>(p.w);
    const int Cin8 = p.Cin4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- loader roles: row (a filter of the bank tile / a pixel of the activation tile) and 16-byte segment of the chunk
    const int lrow = tid >> 2, lseg = tid & 3;
    const int l_co = nblk * RC_BN + lrow;
    const int l_m = mblk * RC_BM + lrow;
    int l_n = 0, l_y0 = 0, l_x0 = 0;      // image, input row / column under tap (0, 0)
    const bool l_mok = l_m < M;
    if (l_mok) {
        const int ox = l_m % p.OW;
        const int t = l_m / p.OW;
        l_y0 = (t % p.OH) * p.stride_h - p.pad_h;
        l_x0 = ox * p.stride_w - p.pad_w;
        l_n = t / p.OH;
    }
    const int lds_slot = lrow * RH_BK + ((lseg ^ swz<4>(lrow)) << 3);
    const int nchunk = (Cin8 + RH_BK - 1) / RH_BK;
    const int total = p.kh * p.kw * nchunk;

    const v8h zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    v8h regW = zero8, regA = zero8;
    int it_r = 0, it_q = 0, it_c = 0;      // the chunk the NEXT fetch() loads
    auto fetch = [&]() {
        const int ci = it_c * RH_BK + lseg * 8;
        const int iy = l_y0 + it_r * p.dil, ix = l_x0 + it_q * p.dil;
        regW = zero8;
        regA = zero8;
        if (ci < Cin8) {
            if (l_co < p.Cout) regW = *(const v8h*)(wh + ((size_t)(l_co * p.kh + it_r) * p.kw + it_q) * Cin8 + ci);
            if (l_mok && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                regA = *(const v8h*)(xh + ((size_t)(l_n * p.H + iy) * p.W + ix) * p.x_cstride + ci);
                // channels Cin .. Cin8-1 of a pixel are padding: never multiplied, whatever they hold
#pragma unroll
                for (int e = 1; e < 8; ++e)
                    if (ci + e >= p.Cin) regA[e] = (f16_t)0.f;
            }
        }
        if (++it_c == nchunk) {
            it_c = 0;
            if (++it_q == p.kw) { it_q = 0; ++it_r; }
        }
    };

    // ---- MFMA roles
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int rowW = wm * 32 + fr, rowA = wn * 32 + fr;
    int offW[2], offA[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {      // MFMA j contracts k 16 j .. 16 j + 15 of the chunk: slots 2 j and 2 j + 1, one per lane half
        offW[j] = rowW * RH_BK + (((2 * j + fh) ^ swz<4>(rowW)) << 3);
        offA[j] = rowA * RH_BK + (((2 * j + fh) ^ swz<4>(rowA)) << 3);
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    fetch();
#pragma unroll 1
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        *(v8h*)&sW[buf][lds_slot] = regW;
        *(v8h*)&sA[buf][lds_slot] = regA;
        if (it + 1 < total) fetch();
        __syncthreads();      // (two buffers, one barrier per chunk: as in rconv_f32_kernel)
        v8h wf[2], af[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            wf[j] = *(const v8h*)&sW[buf][offW[j]];
            af[j] = *(const v8h*)&sA[buf][offA[j]];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], af[j], acc, 0, 0, 0);
    }

    // ---- epilogue: the result layout of rconv_f32_kernel - lane = pixel, registers 4g .. 4g+3 = channels 8g + 4 fh .. +3 of the wave's 32
    const int m = mblk * RC_BM + wn * 32 + fr;
    if (m >= M) return;
    const size_t pix = (size_t)m;
    const bool do_relu = (p.flags & FCN_CONV_RELU) != 0, out32 = (p.flags & FCN_CONV_OUT_F32) != 0;
    float* dst32 = reinterpret_cast<float*>(p.y) + pix * p.y_cstride + p.y_coffset;
    f16_t* dst16 = reinterpret_cast<f16_t*>(p.y) + pix * p.y_cstride + p.y_coffset;
    // bias and ReLU on the lane's own four runs of four channels
    const int cbase = nblk * RC_BN + wm * 32;
    v4f v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = cbase + 8 * g + 4 * fh;
        v[g] = v4f{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p.bias && co + e < p.Cout) v[g][e] += p.bias[co + e];
            if (do_relu) v[g][e] = fmaxf(v[g][e], 0.f);
        }
    }
    if (!out32 && ((p.y_cstride | p.y_coffset) & 7) == 0 && ((unsigned)(size_t)p.y & 15) == 0) {
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
            const int co8 = cbase + 16 * gp + 8 * fh;
            if (co8 + 7 < p.Cout) {
                *(v8h*)(dst16 + co8) = out;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (co8 + e < p.Cout) dst16[co8 + e] = out[e];
            }
        }
        return;
    }
    // otherwise a run of four channels is one store where it is aligned as a whole: 16 bytes of floats, 8 bytes of halves
    const bool vec_ok = ((p.y_cstride | p.y_coffset) & 3) == 0 && ((unsigned)(size_t)p.y & (out32 ? 15 : 7)) == 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int co = cbase + 8 * g + 4 * fh;
        if (co >= p.Cout) continue;
        const int run = min(4, p.Cout - co);
        if (vec_ok && run == 4) {
            if (out32) {
                *(v4f*)(dst32 + co) = v[g];
            } else {
                const v4h h = {(f16_t)v[g][0], (f16_t)v[g][1], (f16_t)v[g][2], (f16_t)v[g][3]};      // round to nearest even, once
                *(v4h*)(dst16 + co) = h;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= run) break;
                if (out32) dst32[co + e] = v[g][e];
                else dst16[co + e] = (f16_t)v[g][e];      // a 2-byte store: the half that shares the word is not touched
            }
        }
    }
}

struct RWgradP {
    const float* x;
    const float* dy;
    float* out;             // dw (one split) or the workspace (a slab of Cout * taps * Cin4 floats per split)
    int N, H, W, Cin, x_cstride, Cout, kh, kw, pad_h, pad_w, stride_h, stride_w, dil, OH, OW;
    int dy_cstride, dy_coffset, dy_vec;
    int Cin4, M, nblk_ci, pix_per_split;
    unsigned long long slab;
};

__global__ __launch_bounds__(RC_THREADS) void rconv_wgrad_kernel(const RWgradP p) {
    const int coblk = blockIdx.x / p.nblk_ci, ciblk = blockIdx.x - coblk * p.nblk_ci;
    const int tap = blockIdx.y, r = tap / p.kw, q = tap - r * p.kw;
    const int split = blockIdx.z;
    const int m0 = split * p.pix_per_split;
    const int m1 = min(m0 + p.pix_per_split, p.M);

    __shared__ __attribute__((aligned(16))) float sD[2][RW_BP * 64];      // dy tile: [pixel][64 output channels]
    __shared__ __attribute__((aligned(16))) float sX[2][RW_BP * 64];      // x tile under the tap: [pixel][64 input channels]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- loader roles: a pixel of the chunk and four consecutive channels of both tiles
    const int lp = tid >> 4, lseg = tid & 15;
    const int l_co = coblk * 64 + lseg * 4, l_ci = ciblk * 64 + lseg * 4;
    const int nchunk = m1 > m0 ? (m1 - m0 + RW_BP - 1) / RW_BP : 0;

    v4f regD = {0.f, 0.f, 0.f, 0.f}, regX = {0.f, 0.f, 0.f, 0.f};
    int it_f = 0;
    auto fetch = [&]() {
        const int m = m0 + it_f * RW_BP + lp;
        ++it_f;
        regD = v4f{0.f, 0.f, 0.f, 0.f};
        regX = v4f{0.f, 0.f, 0.f, 0.f};
        if (m >= m1) return;
        if (l_co < p.Cout) {
            const float* src = p.dy + (size_t)m * p.dy_cstride + p.dy_coffset + l_co;
            if (p.dy_vec && l_co + 3 < p.Cout) {
                regD = *(const v4f*)src;
            } else {
                regD[0] = src[0];
                if (l_co + 1 < p.Cout) regD[1] = src[1];
                if (l_co + 2 < p.Cout) regD[2] = src[2];
                if (l_co + 3 < p.Cout) regD[3] = src[3];
            }
        }
        if (l_ci < p.Cin4) {
            const int ox = m % p.OW;
            const int t = m / p.OW;
            const int oy = t % p.OH, n = t / p.OH;
            const int iy = oy * p.stride_h - p.pad_h + r * p.dil, ix = ox * p.stride_w - p.pad_w + q * p.dil;
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                regX = *(const v4f*)(p.x + ((size_t)(n * p.H + iy) * p.W + ix) * p.x_cstride + l_ci);
                if (l_ci + 1 >= p.Cin) regX[1] = 0.f;
                if (l_ci + 2 >= p.Cin) regX[2] = 0.f;
                if (l_ci + 3 >= p.Cin) regX[3] = 0.f;
            }
        }
    };

    // ---- MFMA roles: A = 32 output channels x 2 pixels, B = 2 pixels x 32 input channels
    const int wm = wave & 1, wn = wave >> 1;
    const int fr = lane & 31, fh = lane >> 5;
    const int colD = wm * 32 + fr, colX = wn * 32 + fr;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    if (nchunk > 0) fetch();
#pragma unroll 1
    for (int it = 0; it < nchunk; ++it) {
        const int buf = it & 1;
        *(v4f*)&sD[buf][lp * 64 + lseg * 4] = regD;
        *(v4f*)&sX[buf][lp * 64 + lseg * 4] = regX;
        if (it + 1 < nchunk) fetch();
        __syncthreads();      // (two buffers, one barrier per chunk: as in rconv_f32_kernel)
#pragma unroll
        for (int t = 0; t < RW_BP / 2; ++t) {
            const float a = sD[buf][(2 * t + fh) * 64 + colD];
            const float b = sX[buf][(2 * t + fh) * 64 + colX];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }

    // ---- lane = input channel (column of the result), registers 4g .. 4g+3 = output channels 8g + 4 fh .. +3 of the wave's 32
    const int ci = ciblk * 64 + colX;
    if (ci >= p.Cin4) return;
    const int taps = p.kh * p.kw;
    float* out = p.out + (size_t)split * p.slab;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = coblk * 64 + wm * 32 + 8 * g + 4 * fh + e;
            if (co < p.Cout) out[((size_t)co * taps + tap) * p.Cin4 + ci] = ci < p.Cin ? acc[4 * g + e] : 0.f;      // pad columns: exact zeros
        }
}

// blocks 0 .. nred-1: dw = slab 0 + slab 1 + ... (ascending, four floats per thread); blocks nred ..: db[c] = sum over pixels of
// dy[pixel][c], every thread a strided run of pixels in ascending order, then a binary tree - the same order on every run
__global__ __launch_bounds__(256) void rconv_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw, long long total4, int splits,
                                                                  unsigned long long slab, int nred, const float* __restrict__ dy,
                                                                  float* __restrict__ db, int pixels, int cstride, int coffset) {
    if ((int)blockIdx.x < nred) {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if (i >= total4) return;
        v4f s = *(const v4f*)(ws + 4 * i);
        for (int k = 1; k < splits; ++k) s += *(const v4f*)(ws + (size_t)k * slab + 4 * i);
        *(v4f*)(dw + 4 * i) = s;
        return;
    }
    __shared__ float part[256];
    const int c = blockIdx.x - nred;
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

// wgrad = true: the descriptor of fcn_rconv2d_wgrad_f32 (w, bias, y2 and flags are not looked at; y names dY)
// half = true: the descriptor of fcn_rconv2d_prepare_f16 (x, w and y point to halves, y to floats under FCN_CONV_OUT_F32)
int validate(const fcn_rconv_desc& d, bool wgrad, bool half = false) {
    FCN_REQUIRE(d.x && d.y && (wgrad || d.w), FCN_E_ARG, "rconv: null x/w/y");
    FCN_REQUIRE(d.N > 0 && d.H > 0 && d.W > 0 && d.Cin > 0 && d.Cout > 0 && d.kh > 0 && d.kw > 0 && d.stride_h > 0 && d.stride_w > 0 &&
                    d.pad_h >= 0 && d.pad_w >= 0,
                FCN_E_ARG,
                "rconv: non-positive extent");
    FCN_REQUIRE(d.dilation >= 1, FCN_E_UNSUPPORTED, "rconv: dilation %d below 1", d.dilation);
    FCN_REQUIRE(d.kh * (long long)d.kw <= 4096, FCN_E_UNSUPPORTED, "rconv: kernel window %dx%d too large", d.kh, d.kw);
    const int vec = half ? 8 : 4;      // elements of a 16-byte load
    const int ci4 = (d.Cin + vec - 1) & ~(vec - 1);
    FCN_REQUIRE(d.x_cstride % vec == 0 && d.x_cstride >= ci4, FCN_E_ALIGN, "rconv: x_cstride (%d) must be a multiple of %d holding Cin (%d) padded to %d",
                d.x_cstride, vec, d.Cin, vec);
    FCN_REQUIRE(((uintptr_t)d.x & 15) == 0 && (wgrad || ((uintptr_t)d.w & 15) == 0), FCN_E_ALIGN, "rconv: x / w must be 16-byte aligned");
    if (half && !(d.flags & FCN_CONV_OUT_F32))
        FCN_REQUIRE(((uintptr_t)d.y & 1) == 0 && (!d.bias || ((uintptr_t)d.bias & 3) == 0), FCN_E_ALIGN, "rconv: y must be 2-byte, bias 4-byte aligned");
    else
        FCN_REQUIRE(((uintptr_t)d.y & 3) == 0 && (wgrad || !d.bias || ((uintptr_t)d.bias & 3) == 0), FCN_E_ALIGN, "rconv: y / bias must be 4-byte aligned");
    const long long eh = (long long)d.dilation * (d.kh - 1) + 1, ew = (long long)d.dilation * (d.kw - 1) + 1;
    const long long nh = (long long)d.H + 2ll * d.pad_h - eh, nw = (long long)d.W + 2ll * d.pad_w - ew;
    FCN_REQUIRE(nh >= 0 && nw >= 0, FCN_E_ARG, "rconv: the window (%lldx%lld) exceeds the padded image", eh, ew);
    FCN_REQUIRE(d.OH == nh / d.stride_h + 1 && d.OW == nw / d.stride_w + 1, FCN_E_ARG,
                "rconv: OH/OW (%d,%d) is not (H + 2 pad - (dil (k-1) + 1)) / stride + 1 per axis = (%lld,%lld)", d.OH, d.OW, nh / d.stride_h + 1,
                nw / d.stride_w + 1);
    FCN_REQUIRE(d.y_coffset >= 0 && d.y_cstride >= d.y_coffset + d.Cout, FCN_E_ARG, "rconv: output slice exceeds y_cstride");
    if (half) {      // the training epilogues stay float32
        FCN_REQUIRE((d.flags & ~(FCN_CONV_RELU | FCN_CONV_OUT_F32)) == 0 && !d.y2, FCN_E_UNSUPPORTED,
                    "rconv: flags 0x%x outside FCN_CONV_RELU | FCN_CONV_OUT_F32, or y2 set (half floats: forward only)", d.flags);
    } else if (!wgrad) {
        FCN_REQUIRE((d.flags & ~(FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK)) == 0, FCN_E_UNSUPPORTED,
                    "rconv: flags 0x%x outside FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK (float32 only)", d.flags);
        if (d.flags & FCN_CONV_MASK)
            FCN_REQUIRE(d.y2 && ((uintptr_t)d.y2 & 3) == 0 && d.y2_coffset >= 0 && d.y2_cstride >= d.y2_coffset + d.Cout, FCN_E_ARG,
                        "rconv: FCN_CONV_MASK needs y2 with a slice of Cout channels");
    }
    FCN_REQUIRE((long long)d.N * d.H * d.W * d.x_cstride < (1ll << 31) && (long long)d.N * d.OH * d.OW * d.y_cstride < (1ll << 31) &&
                    (long long)d.kh * d.kw * d.Cout * ci4 < (1ll << 31) &&
                    (wgrad || half || !(d.flags & FCN_CONV_MASK) || (long long)d.N * d.OH * d.OW * d.y2_cstride < (1ll << 31)),
                FCN_E_UNSUPPORTED, "rconv: tensor too large for 32-bit element offsets");
    return 0;
}

long long tiles_x(const fcn_rconv_desc& d) {
    return ((long long)d.N * d.OH * d.OW + RC_BM - 1) / RC_BM * ((d.Cout + RC_BN - 1) / RC_BN);
}

// pixel splits of the weight gradient: enough workgroups to fill the chip, at least 256 pixels each, a multiple of the chunk
struct WgradPlan { int splits, pix_per_split, nblk_co, nblk_ci; };
WgradPlan wgrad_plan(const fcn_rconv_desc& d) {
    WgradPlan wp;
    const int ci4 = (d.Cin + 3) & ~3;
    wp.nblk_co = (d.Cout + 63) / 64;
    wp.nblk_ci = (ci4 + 63) / 64;
    const long long M = (long long)d.N * d.OH * d.OW;
    const long long tiles = (long long)wp.nblk_co * wp.nblk_ci * d.kh * d.kw;
    long long want = (1024 + tiles - 1) / tiles;
    const long long most = (M + 255) / 256;
    if (want > most) want = most;
    if (want > RW_MAX_SPLITS) want = RW_MAX_SPLITS;
    if (want < 1) want = 1;
    long long pps = (M + want - 1) / want;
    pps = (pps + RW_BP - 1) / RW_BP * RW_BP;
    wp.pix_per_split = (int)pps;
    wp.splits = (int)((M + pps - 1) / pps);      // (no empty split)
    return wp;
}

}  // namespace
}  // namespace fcn

using namespace fcn;

// ---- the host side: every refusal is made here, before the first HIP call
extern "C" {

int fcn_rconv2d_num_configs(void) { return RC_CONFIGS; }
int fcn_rconv2d_num_configs_f16(void) { return RH_CONFIGS; }

size_t fcn_rconv2d_workspace_bytes(const fcn_rconv_desc* h_descs, int n) {
    (void)h_descs;
    return n > 0 ? (size_t)n * sizeof(RConvP) : 0;
}

static int rconv_prepare(const fcn_rconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_rconv_plan* h_out, bool half) {
    FCN_REQUIRE(h_descs && h_out && n > 0, FCN_E_ARG, "rconv prepare: null descriptors / plan or n <= 0");
    FCN_REQUIRE(n <= 65535, FCN_E_UNSUPPORTED, "rconv prepare: more than 65535 problems");
    FCN_REQUIRE(cfg_request >= -1 && cfg_request < (half ? RH_CONFIGS : RC_CONFIGS), FCN_E_ARG, "rconv prepare: unknown configuration %d", cfg_request);
    long long gx = 0, total = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = validate(h_descs[i], false, half);
        if (rc) return rc;
        const long long tx = tiles_x(h_descs[i]);
        gx = tx > gx ? tx : gx;
        total += tx;
    }
    FCN_REQUIRE(gx < (1ll << 31) && total < (1ll << 31), FCN_E_UNSUPPORTED, "rconv prepare: too many tiles for one launch");
    FCN_REQUIRE(d_workspace, FCN_E_ARG, "rconv prepare: null workspace");
    FCN_REQUIRE(!half || ((uintptr_t)d_workspace & 15) == 0, FCN_E_ALIGN, "rconv prepare: the workspace must be 16-byte aligned");
    std::vector<RConvP> ps((size_t)n);
    for (int i = 0; i < n; ++i) {
        const fcn_rconv_desc& d = h_descs[i];
        RConvP& p = ps[(size_t)i];
        p.x = d.x; p.w = d.w; p.bias = d.bias; p.y = d.y; p.y2 = (d.flags & FCN_CONV_MASK) ? d.y2 : nullptr;
        p.N = d.N; p.H = d.H; p.W = d.W; p.Cin = d.Cin; p.x_cstride = d.x_cstride; p.Cout = d.Cout; p.kh = d.kh; p.kw = d.kw;
        p.pad_h = d.pad_h; p.pad_w = d.pad_w; p.stride_h = d.stride_h; p.stride_w = d.stride_w; p.dil = d.dilation; p.OH = d.OH; p.OW = d.OW;
        p.y_cstride = d.y_cstride; p.y_coffset = d.y_coffset; p.y2_cstride = d.y2_cstride; p.y2_coffset = d.y2_coffset; p.flags = d.flags;
        p.Cin4 = half ? (d.Cin + 7) & ~7 : (d.Cin + 3) & ~3;
        p.nblk_n = (d.Cout + RC_BN - 1) / RC_BN;
        p.M = d.N * d.OH * d.OW;
    }
    FCN_HIP(hipMemcpy(d_workspace, ps.data(), ps.size() * sizeof(RConvP), hipMemcpyHostToDevice));
    h_out->d_probs = d_workspace;
    h_out->n = n;
    h_out->cfg = half ? RH_CFG_BASE : 0;
    h_out->grid_x = (int32_t)gx;
    h_out->grid_y = 1;
    h_out->total_tiles = (int32_t)total;
    return 0;
}

int fcn_rconv2d_prepare(const fcn_rconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_rconv_plan* h_out) {
    return rconv_prepare(h_descs, n, d_workspace, cfg_request, h_out, false);
}

int fcn_rconv2d_prepare_f16(const fcn_rconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_rconv_plan* h_out) {
    return rconv_prepare(h_descs, n, d_workspace, cfg_request, h_out, true);
}

int fcn_rconv2d_f32(const fcn_rconv_plan* h_plan, fcn_stream_t s) {
    FCN_REQUIRE(h_plan && h_plan->d_probs && h_plan->n > 0 && h_plan->grid_x > 0 && h_plan->grid_y == 1 && h_plan->n <= 65535 && h_plan->cfg == 0,
                FCN_E_ARG, "rconv: the plan was not filled by fcn_rconv2d_prepare");
    hipLaunchKernelGGL(rconv_f32_kernel, dim3((unsigned)h_plan->grid_x, 1u, (unsigned)h_plan->n), dim3(RC_THREADS), 0, as_stream(s),
                       (const RConvP*)h_plan->d_probs);
    FCN_LAUNCH_CHECK("rconv_f32_kernel");
    return 0;
}

int fcn_rconv2d_f16(const fcn_rconv_plan* h_plan, fcn_stream_t s) {
    FCN_REQUIRE(h_plan && h_plan->d_probs && h_plan->n > 0 && h_plan->grid_x > 0 && h_plan->grid_y == 1 && h_plan->n <= 65535 &&
                    h_plan->cfg >= RH_CFG_BASE && h_plan->cfg < RH_CFG_BASE + RH_CONFIGS,
                FCN_E_ARG, "rconv: the plan was not filled by fcn_rconv2d_prepare_f16");
    hipLaunchKernelGGL(rconv_f16_kernel, dim3((unsigned)h_plan->grid_x, 1u, (unsigned)h_plan->n), dim3(RC_THREADS), 0, as_stream(s),
                       (const RConvP*)h_plan->d_probs);
    FCN_LAUNCH_CHECK("rconv_f16_kernel");
    return 0;
}

size_t fcn_rconv2d_wgrad_workspace_floats(const fcn_rconv_desc* h_d) {
    if (!h_d || validate(*h_d, true)) return 0;
    const WgradPlan wp = wgrad_plan(*h_d);
    if (wp.splits <= 1) return 0;
    return (size_t)wp.splits * h_d->Cout * h_d->kh * h_d->kw * ((h_d->Cin + 3) & ~3);
}

int fcn_rconv2d_wgrad_f32(const fcn_rconv_desc* h_d, float* dw, float* db, float* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(h_d && dw, FCN_E_ARG, "rconv wgrad: null descriptor / dw");
    const fcn_rconv_desc& d = *h_d;
    const int rc = validate(d, true);
    if (rc) return rc;
    FCN_REQUIRE(((uintptr_t)dw & 15) == 0 && (!db || ((uintptr_t)db & 3) == 0), FCN_E_ALIGN, "rconv wgrad: dw must be 16-byte, db 4-byte aligned");
    const WgradPlan wp = wgrad_plan(d);
    const int ci4 = (d.Cin + 3) & ~3, taps = d.kh * d.kw;
    const unsigned long long slab = (unsigned long long)d.Cout * taps * ci4;
    FCN_REQUIRE(wp.splits == 1 || d_workspace, FCN_E_ARG, "rconv wgrad: %d pixel splits need a workspace", wp.splits);
    FCN_REQUIRE(wp.splits == 1 || ((uintptr_t)d_workspace & 15) == 0, FCN_E_ALIGN, "rconv wgrad: the workspace must be 16-byte aligned");
    FCN_REQUIRE((long long)wp.nblk_co * wp.nblk_ci < (1ll << 31) && taps <= 65535, FCN_E_UNSUPPORTED, "rconv wgrad: too many tiles for one launch");
    RWgradP p;
    p.x = d.x; p.dy = d.y; p.out = wp.splits == 1 ? dw : d_workspace;
    p.N = d.N; p.H = d.H; p.W = d.W; p.Cin = d.Cin; p.x_cstride = d.x_cstride; p.Cout = d.Cout; p.kh = d.kh; p.kw = d.kw;
    p.pad_h = d.pad_h; p.pad_w = d.pad_w; p.stride_h = d.stride_h; p.stride_w = d.stride_w; p.dil = d.dilation; p.OH = d.OH; p.OW = d.OW;
    p.dy_cstride = d.y_cstride; p.dy_coffset = d.y_coffset;
    p.dy_vec = (((uintptr_t)d.y & 15) == 0 && ((d.y_cstride | d.y_coffset) & 3) == 0) ? 1 : 0;
    p.Cin4 = ci4; p.M = d.N * d.OH * d.OW; p.nblk_ci = wp.nblk_ci; p.pix_per_split = wp.pix_per_split;
    p.slab = slab;
    hipLaunchKernelGGL(rconv_wgrad_kernel, dim3((unsigned)(wp.nblk_co * wp.nblk_ci), (unsigned)taps, (unsigned)wp.splits), dim3(RC_THREADS), 0, as_stream(s), p);
    FCN_LAUNCH_CHECK("rconv_wgrad_kernel");
    const long long total4 = (long long)(slab / 4);
    const int nred = wp.splits > 1 ? (int)((total4 + 255) / 256) : 0;
    const int nsum = db ? d.Cout : 0;
    if (nred + nsum > 0) {
        hipLaunchKernelGGL(rconv_wgrad_finish_kernel, dim3((unsigned)(nred + nsum)), dim3(256), 0, as_stream(s), (const float*)d_workspace, dw, total4,
                           wp.splits, slab, nred, d.y, db, p.M, d.y_cstride, d.y_coffset);
        FCN_LAUNCH_CHECK("rconv_wgrad_finish_kernel");
    }
    return 0;
}

}  // extern "C"
