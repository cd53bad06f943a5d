// InnerProduct above FCN_IP_MAX_ROWS input rows on the matrix cores of gfx950 (the streaming kernels of inner_product.hip hold every
// row's sums in registers and stop at 32 rows; from about 48 rows on the layer is bound by arithmetic, not by the bank's bytes).
//
// The layer's three products are ONE product out[i][j] = sum_r A[i][r] * B[j][r] over operands that differ only in how they lie in
// memory:
//
//                 out (I x J)        A (rows i)                      B (rows j)                     reduction r
//  forward        y[m][n]            x[m][k]    k contiguous         w[n][k]   k contiguous         k < K
//  bwd_data       dX[m][k]           dY[m][n]   n contiguous         w[n][k]   k (= j) contiguous   n < N
//  bwd_weights    dW[n][k]           dY[m][n]   n (= i) contiguous   x[m][k]   k (= j) contiguous   m < M
//
// so there is one kernel, ip_gemm_kernel<T, StageA, StageB>: a workgroup of four waves owns a 64 x 64 tile of out and walks the reduction
// in chunks of 128 bytes per row (32 floats / 64 halves).  A stager (four of them below: r contiguous with 16-byte or 4-byte loads, the
// tile's rows contiguous with 4-byte or 16-byte loads) brings a 64-row chunk of its operand from global memory into
// registers (32 bytes per lane) and from there into LDS as [row][r] with rows 144 bytes apart (16 bytes of padding: the 16-byte
// fragment reads of 32 consecutive rows fall on distinct bank groups); the loads of chunk c + 1 are in flight while the MFMAs of chunk c
// run.  Each wave owns one 32 x 32 accumulator: v_mfma_f32_32x32x2_f32 (lane half h takes r = 16 h + q of the chunk in step q, for both
// operands alike - the order of a sum inside a chunk is free as long as it is fixed) or v_mfma_f32_32x32x16_f16 (a lane's 16-byte
// fragment is 8 consecutive r of its row).  A is the instruction's row operand and B its column operand, so the lanes of a result
// register are 32 consecutive j: stores of y, dX and dW coalesce.
//
// Rows past I / J are loaded from the last valid row and never stored.  Reduction elements past the end are ZEROS IN REGISTERS, never
// loaded (what lies behind a row's K elements may be NaN).  No atomics: where the tiles cannot fill the chip the reduction is cut into
// slices (a function of the shape alone), the slices leave float32 partial tiles in the workspace and a second launch adds them in
// slice order and applies the epilogue (bias, ReLU, accumulate, rounding to halves), which is the same code in both places.
#include "common.h"

using namespace fcn;

namespace {

constexpr int GT = 64;                 // tile rows and columns
constexpr int GROW = 144;              // bytes of an LDS row: 128 of data, 16 of padding
constexpr int GCHUNK_BYTES = 128;      // reduction bytes per row and chunk
constexpr int GTHREADS = 256;
constexpr int G_TARGET_WGS = 1024;     // four workgroups per CU: a workgroup alone on a CU waits at its barriers with the MFMA pipe idle
constexpr int G_MIN_CHUNKS = 8;        // a slice is at least this many chunks long

constexpr int EP_RELU = 1, EP_ACCUM = 2, EP_HALF = 4;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct Operand {
    const void* base;
    int stride, off, rows;     // element (row, r): see the stagers
};

struct GemmArgs {
    Operand a, b;
    const float* bias;         // per column j, or NULL
    void* out;                 // out[i * ostride + ooff + j]
    float* ws;                 // [S][I][J] when S > 1
    int ostride, ooff, I, J, R, ep, cps, S, tiles_i;
};

// ---- stagers: load() fills 32 bytes per lane from a 64-row chunk starting at reduction index r0 (elements at or past r_end are zeros),
//      store() puts them into the LDS tile as [row][r] ----

// element (row, r) at base[row * stride + off + r], r contiguous, 16-byte loads along r (stride, off, r0 and r_end are multiples of 16 bytes)
template <typename T>
struct StageRowK16 {
    static constexpr int E = 16 / (int)sizeof(T);
    static __device__ __forceinline__ void load(f32x4 (&v)[2], const Operand& o, int row0, int r0, int r_end, int tid) {
        const T* base = reinterpret_cast<const T*>(o.base);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = tid + GTHREADS * t, row = u >> 3, r = r0 + (u & 7) * E;
            v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < r_end) v[t] = *reinterpret_cast<const f32x4*>(base + (size_t)min(row0 + row, o.rows - 1) * o.stride + o.off + r);
        }
    }
    static __device__ __forceinline__ void store(const f32x4 (&v)[2], char* tile, int tid) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = tid + GTHREADS * t;
            *reinterpret_cast<f32x4*>(tile + (u >> 3) * GROW + (u & 7) * 16) = v[t];
        }
    }
};

// float32, element (row, r) at base[row * stride + off + r], r contiguous, any offset: 32 lanes side by side along r
struct StageRowK1 {
    static __device__ __forceinline__ void load(f32x4 (&v)[2], const Operand& o, int row0, int r0, int r_end, int tid) {
        const float* base = reinterpret_cast<const float*>(o.base);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int e = tid + GTHREADS * t, row = e >> 5, r = r0 + (e & 31);
            float x = 0.f;
            if (r < r_end) x = base[(size_t)min(row0 + row, o.rows - 1) * o.stride + o.off + r];
            v[t >> 2][t & 3] = x;
        }
    }
    static __device__ __forceinline__ void store(const f32x4 (&v)[2], char* tile, int tid) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int e = tid + GTHREADS * t;
            reinterpret_cast<float*>(tile + (e >> 5) * GROW)[e & 31] = v[t >> 2][t & 3];
        }
    }
};

// float32, element (row, r) at base[r * stride + off + row], the tile's ROWS contiguous: 64 lanes side by side along the rows
struct StageKRow1 {
    static __device__ __forceinline__ void load(f32x4 (&v)[2], const Operand& o, int row0, int r0, int r_end, int tid) {
        const float* base = reinterpret_cast<const float*>(o.base);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int e = tid + GTHREADS * t, row = e & 63, r = r0 + (e >> 6);
            float x = 0.f;
            if (r < r_end) x = base[(size_t)r * o.stride + o.off + min(row0 + row, o.rows - 1)];
            v[t >> 2][t & 3] = x;
        }
    }
    static __device__ __forceinline__ void store(const f32x4 (&v)[2], char* tile, int tid) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int e = tid + GTHREADS * t;
            reinterpret_cast<float*>(tile + (e & 63) * GROW)[e >> 6] = v[t >> 2][t & 3];
        }
    }
};

// the same element order where off, stride and the row count are multiples of 4 floats (the bank in bwd_data, x in bwd_weights): a lane
// loads 16 bytes = four consecutive ROWS of one r - a group of four rows is inside or outside as a whole - and stores them as four floats
struct StageKRow4 {
    static __device__ __forceinline__ void load(f32x4 (&v)[2], const Operand& o, int row0, int r0, int r_end, int tid) {
        const float* base = reinterpret_cast<const float*>(o.base);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = tid + GTHREADS * t, row = min(row0 + 4 * (u & 15), o.rows - 4), r = r0 + (u >> 4);
            v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < r_end) v[t] = *reinterpret_cast<const f32x4*>(base + (size_t)r * o.stride + o.off + row);
        }
    }
    static __device__ __forceinline__ void store(const f32x4 (&v)[2], char* tile, int tid) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = tid + GTHREADS * t;
#pragma unroll
            for (int e = 0; e < 4; ++e) reinterpret_cast<float*>(tile + (4 * (u & 15) + e) * GROW)[u >> 4] = v[t][e];
        }
    }
};

// one chunk of a wave's 32 x 32 product from the two LDS tiles
template <typename T>
__device__ __forceinline__ f32x16 chunk_mfma(const char* arow, const char* brow, int h, f32x16 acc) {
    if constexpr (sizeof(T) == 4) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = *reinterpret_cast<const f32x4*>(arow + h * 64 + q * 16);
            b[q] = *reinterpret_cast<const f32x4*>(brow + h * 64 + q * 16);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q >> 2][q & 3], b[q >> 2][q & 3], acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f16x8 a = *reinterpret_cast<const f16x8*>(arow + q * 32 + h * 16);
            const f16x8 b = *reinterpret_cast<const f16x8*>(brow + q * 32 + h * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        }
    }
    return acc;
}

// bias, ReLU, accumulate and rounding: the one place a finished sum is written from
__device__ __forceinline__ void epilogue(const GemmArgs& g, int i, int j, float v) {
    if (g.bias) v += g.bias[j];
    if (g.ep & EP_RELU) v = fmaxf(v, 0.f);
    const size_t at = (size_t)i * g.ostride + g.ooff + j;
    if (g.ep & EP_HALF) {
        reinterpret_cast<_Float16*>(g.out)[at] = (_Float16)v;
    } else {
        float* p = reinterpret_cast<float*>(g.out) + at;
        *p = (g.ep & EP_ACCUM) ? *p + v : v;
    }
}

// grid: (tiles_i * tiles_j, S), i fastest: the workgroups that share a tile of B (the bank, in forward and bwd_data) run side by side
template <typename T, typename SA, typename SB>
__global__ __launch_bounds__(GTHREADS) void ip_gemm_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) char tiles[2][GT * GROW];
    constexpr int CH = GCHUNK_BYTES / (int)sizeof(T);        // reduction elements per chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = (int)blockIdx.x % g.tiles_i, tj = (int)blockIdx.x / g.tiles_i, slice = blockIdx.y;
    const int i0 = ti * GT, j0 = tj * GT;
    const int r_begin = slice * g.cps * CH, r_end = min(g.R, r_begin + g.cps * CH);

    f32x4 ra[2], rb[2];
    SA::load(ra, g.a, i0, r_begin, r_end, tid);
    SB::load(rb, g.b, j0, r_begin, r_end, tid);
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32, l31 = lane & 31, h = lane >> 5;
    const char* arow = tiles[0] + (wi + l31) * GROW;
    const char* brow = tiles[1] + (wj + l31) * GROW;
    for (int r0 = r_begin; r0 < r_end; r0 += CH) {           // (r_begin < r_end for every slice: see gemm_plan)
        SA::store(ra, tiles[0], tid);
        SB::store(rb, tiles[1], tid);
        __syncthreads();
        if (r0 + CH < r_end) {
            SA::load(ra, g.a, i0, r0 + CH, r_end, tid);
            SB::load(rb, g.b, j0, r0 + CH, r_end, tid);
        }
        acc = chunk_mfma<T>(arow, brow, h, acc);
        __syncthreads();
    }
    // register q of lane (l31, h) is out[wi + (q & 3) + 8 (q >> 2) + 4 h][wj + l31]
    const int j = j0 + wj + l31;
    if (j >= g.J) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + wi + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (i >= g.I) continue;
        if (g.S > 1) g.ws[((size_t)slice * g.I + i) * g.J + j] = acc[q];
        else epilogue(g, i, j, acc[q]);
    }
}

// out[i][j] = epilogue(sum over slices in slice order): one lane per output
__global__ __launch_bounds__(256) void ip_gemm_combine_kernel(GemmArgs g) {
    const long long at = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= (long long)g.I * g.J) return;
    const int i = (int)(at / g.J), j = (int)(at - (long long)i * g.J);
    float v = 0.f;
    for (int s = 0; s < g.S; ++s) v += g.ws[((size_t)s * g.I + i) * g.J + j];
    epilogue(g, i, j, v);
}

// ---- host side ----
struct GemmPlan { int S, cps; };

// Slices of the reduction so that about G_TARGET_WGS workgroups run (none where three quarters of that many tiles exist), each slice at least G_MIN_CHUNKS chunks long and none empty.
// A function of the extents and the element size alone: the workspace query and the launch agree, and so do two runs.
GemmPlan gemm_plan(long long I, long long J, int R, int esize) {
    const int chunks = cdiv(R, GCHUNK_BYTES / esize);
    const long long tiles = (long long)cdiv(I, GT) * cdiv(J, GT);
    int S = tiles >= G_TARGET_WGS * 3 / 4 ? 1 : (int)((G_TARGET_WGS + tiles - 1) / tiles);
    if (S > chunks / G_MIN_CHUNKS) S = chunks / G_MIN_CHUNKS;
    if (S < 1) S = 1;
    const int cps = cdiv(chunks, S);
    return GemmPlan{cdiv(chunks, cps), cps};
}

size_t gemm_ws_bytes(long long I, long long J, int R, int esize) {
    const GemmPlan p = gemm_plan(I, J, R, esize);
    return p.S > 1 ? (size_t)p.S * (size_t)I * (size_t)J * 4 : 0;
}

template <typename T, typename SA, typename SB>
int gemm_launch(const char* who, GemmArgs g, int esize, void* d_workspace, fcn_stream_t s) {
    const GemmPlan p = gemm_plan(g.I, g.J, g.R, esize);
    FCN_REQUIRE(p.S == 1 || (d_workspace && aligned16(d_workspace)), p.S == 1 || d_workspace ? FCN_E_ALIGN : FCN_E_ARG,
                "%s: this shape needs the workspace of fcn_ip_gemm_workspace_bytes (16-byte aligned)", who);
    g.ws = reinterpret_cast<float*>(d_workspace);
    g.S = p.S;
    g.cps = p.cps;
    g.tiles_i = cdiv(g.I, GT);
    const long long tiles = (long long)g.tiles_i * cdiv(g.J, GT);
    FCN_REQUIRE(tiles < (1ll << 31), FCN_E_UNSUPPORTED, "%s: more than 2^31 output tiles", who);
    hipLaunchKernelGGL((ip_gemm_kernel<T, SA, SB>), dim3((unsigned)tiles, p.S), dim3(GTHREADS), 0, as_stream(s), g);
    FCN_LAUNCH_CHECK(who);
    if (p.S > 1) {
        hipLaunchKernelGGL(ip_gemm_combine_kernel, dim3(cdiv((long long)g.I * g.J, 256)), dim3(256), 0, as_stream(s), g);
        FCN_LAUNCH_CHECK(who);
    }
    return 0;
}

// the checks every entry point shares (those of the streaming kernels without the row limit); every one precedes the first HIP call
int gemm_check(const char* who, const void* a, const void* b, const void* c, int M, int K, int N, int E) {
    FCN_REQUIRE(a && b && c && M > 0 && K > 0 && N > 0, FCN_E_ARG, "%s: null pointer or non-positive extent", who);
    FCN_REQUIRE(K % E == 0 && aligned16(a) && aligned16(b) && aligned16(c), FCN_E_ALIGN,
                "%s: K must be a multiple of %d elements, pointers of 16 bytes", who, E);
    FCN_REQUIRE((long long)N * K < (1ll << 31), FCN_E_UNSUPPORTED, "%s: bank past 2^31 elements", who);
    return 0;
}

int gemm_bwd_check(const char* who, int M, int K, int N, int dy_cstride, int dy_coffset, int rstride) {
    FCN_REQUIRE(rstride >= K && dy_coffset >= 0 && dy_cstride >= dy_coffset + N, FCN_E_ARG, "%s: row stride below K or slice out of range", who);
    FCN_REQUIRE(rstride % 4 == 0 && dy_cstride % 4 == 0, FCN_E_ALIGN, "%s: strides must be multiples of 16 bytes", who);
    FCN_REQUIRE((long long)M * rstride < (1ll << 31) && (long long)M * dy_cstride < (1ll << 31), FCN_E_UNSUPPORTED, "%s: views past 2^31 elements",
                who);
    return 0;
}

template <typename T>
int gemm_fwd(const char* who, const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset, int M, int K,
             int N, int flags, void* d_workspace, fcn_stream_t s) {
    constexpr int E = 16 / (int)sizeof(T);
    if (int rc = gemm_check(who, x, w, y, M, K, N, E)) return rc;
    const int allowed = sizeof(T) == 2 ? (FCN_CONV_RELU | FCN_CONV_OUT_F32) : FCN_CONV_RELU;
    FCN_REQUIRE((flags & ~allowed) == 0, FCN_E_ARG, "%s: flags 0x%x outside 0x%x", who, flags, allowed);
    const bool half_out = sizeof(T) == 2 && !(flags & FCN_CONV_OUT_F32);
    const int YE = half_out ? 8 : 4;
    FCN_REQUIRE(x_rstride >= K && y_coffset >= 0 && y_cstride >= y_coffset + N, FCN_E_ARG, "%s: row stride below K or slice out of range", who);
    FCN_REQUIRE(x_rstride % E == 0 && y_cstride % YE == 0 && (!bias || aligned16(bias)), FCN_E_ALIGN,
                "%s: strides must be multiples of 16 bytes, pointers of 16 bytes", who);
    FCN_REQUIRE((long long)M * x_rstride < (1ll << 31) && (long long)M * y_cstride < (1ll << 31), FCN_E_UNSUPPORTED, "%s: views past 2^31 elements",
                who);
    GemmArgs g{};
    g.a = Operand{x, x_rstride, 0, M};
    g.b = Operand{w, K, 0, N};
    g.bias = bias;
    g.out = y;
    g.ostride = y_cstride, g.ooff = y_coffset, g.I = M, g.J = N, g.R = K;
    g.ep = ((flags & FCN_CONV_RELU) ? EP_RELU : 0) | (half_out ? EP_HALF : 0);
    return gemm_launch<T, StageRowK16<T>, StageRowK16<T>>(who, g, (int)sizeof(T), d_workspace, s);
}

}  // namespace

extern "C" {

size_t fcn_ip_gemm_workspace_bytes(int M, int K, int N, int esize) {
    if (M <= 0 || K <= 0 || N <= 0 || (esize != 2 && esize != 4)) return 0;
    size_t need = gemm_ws_bytes(M, N, K, esize);                           // forward
    if (esize == 4) {
        const size_t d = gemm_ws_bytes(M, K, N, 4), w = gemm_ws_bytes(N, K, M, 4);      // bwd_data, bwd_weights
        if (d > need) need = d;
        if (w > need) need = w;
    }
    return need;
}

int fcn_ip_gemm_fwd_f32(const float* x, int x_rstride, const float* w, const float* bias, float* y, int y_cstride, int y_coffset, int M, int K,
                        int N, int flags, void* d_workspace, fcn_stream_t s) {
    return gemm_fwd<float>("ip_gemm_fwd_f32", x, x_rstride, w, bias, y, y_cstride, y_coffset, M, K, N, flags, d_workspace, s);
}

int fcn_ip_gemm_fwd_f16(const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset, int M, int K, int N,
                        int flags, void* d_workspace, fcn_stream_t s) {
    return gemm_fwd<_Float16>("ip_gemm_fwd_f16", x, x_rstride, w, bias, y, y_cstride, y_coffset, M, K, N, flags, d_workspace, s);
}

int fcn_ip_gemm_bwd_data_f32(const float* dy, int dy_cstride, int dy_coffset, const float* w, float* dx, int dx_rstride, int M, int K, int N,
                             int flags, void* d_workspace, fcn_stream_t s) {
    const char* who = "ip_gemm_bwd_data_f32";
    if (int rc = gemm_check(who, dy, w, dx, M, K, N, 4)) return rc;
    FCN_REQUIRE((flags & ~FCN_CONV_ACCUM) == 0, FCN_E_ARG, "%s: flags 0x%x outside FCN_CONV_ACCUM", who, flags);
    if (int rc = gemm_bwd_check(who, M, K, N, dy_cstride, dy_coffset, dx_rstride)) return rc;
    GemmArgs g{};
    g.a = Operand{dy, dy_cstride, dy_coffset, M};          // (m, n) at dy[m * cstride + coffset + n]
    g.b = Operand{w, K, 0, K};                             // (k, n) at w[n * K + k]
    g.out = dx;
    g.ostride = dx_rstride, g.ooff = 0, g.I = M, g.J = K, g.R = N;
    g.ep = (flags & FCN_CONV_ACCUM) ? EP_ACCUM : 0;
    return gemm_launch<float, StageRowK1, StageKRow4>(who, g, 4, d_workspace, s);
}

int fcn_ip_gemm_bwd_weights_f32(const float* x, int x_rstride, const float* dy, int dy_cstride, int dy_coffset, float* dw, float* db, int M, int K,
                                int N, int accumulate, void* d_workspace, fcn_stream_t s) {
    const char* who = "ip_gemm_bwd_weights_f32";
    if (int rc = gemm_check(who, x, dy, dw, M, K, N, 4)) return rc;
    FCN_REQUIRE(accumulate == 0 || accumulate == 1, FCN_E_ARG, "%s: accumulate must be 0 or 1", who);
    if (int rc = gemm_bwd_check(who, M, K, N, dy_cstride, dy_coffset, x_rstride)) return rc;
    FCN_REQUIRE(!db || aligned16(db), FCN_E_ALIGN, "%s: db must be 16-byte aligned", who);
    GemmArgs g{};
    g.a = Operand{dy, dy_cstride, dy_coffset, N};          // (n, m) at dy[m * cstride + coffset + n]
    g.b = Operand{x, x_rstride, 0, K};                     // (k, m) at x[m * rstride + k]
    g.out = dw;
    g.ostride = K, g.ooff = 0, g.I = N, g.J = K, g.R = M;
    g.ep = accumulate ? EP_ACCUM : 0;
    if (int rc = gemm_launch<float, StageKRow1, StageKRow4>(who, g, 4, d_workspace, s)) return rc;
    if (db) return ip_bias_grad(who, dy, db, dy_cstride, dy_coffset, M, N, accumulate, s);
    return 0;
}

}  // extern "C"
