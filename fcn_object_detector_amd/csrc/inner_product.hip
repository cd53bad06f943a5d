// InnerProduct (Caffe InnerProductLayer) for gfx950 at M <= FCN_IP_MAX_ROWS input rows: y[M][N] = x[M][K] * w[N][K]^T + bias.
//
// At the batch sizes of a deployed classifier (1, CaffeNet's 10) the layer is a weight stream: fc6 of CaffeNet reads 151 MB of float32
// for 75 MFLOP per image.  So all four kernels are built around ONE pass over the bank (or over dW) with 16-byte accesses:
//
//  forward       a wave owns IP_R rows of w (output channels) and a slice of K.  Per step a lane takes 16 bytes of each row, lanes side
//                by side (1 KB per row and step), IP_U steps deep: IP_R * IP_U 16-byte loads are issued back to back straight into VGPRs
//                before the first is waited for (no LDS round trip: nothing shares a weight).  The M input rows are the shared operand;
//                they are re-read through L1 / L2 (the four waves of a workgroup walk the same K slice).  All M rows accumulate against
//                the weights held in registers, so a weight byte is fetched once whatever M is.  Lane sums are combined by a fixed
//                xor-shuffle tree; K slices (needed to fill the chip when N is small) leave float32 partial sums in the workspace and
//                a second small launch adds them in slice order, adds the bias and applies ReLU.  No atomics: results do not depend on
//                the run.
//  bwd_data      the same stream read the other way: a lane owns 4 consecutive k of dX for all M rows and walks a slice of the rows
//                of w; dY of the slice lies in LDS and is read as a broadcast.  No cross-lane reduction at all; the n slices are added
//                in slice order by a second launch.
//  bwd_weights   a write stream: a lane keeps x[0..M)[k..k+3] in registers and writes 16 bytes of dW per output channel; each element
//                of dW has one writer.  db is a tiny launch of its own.
#include "common.h"

using namespace fcn;

namespace {

constexpr int IP_R = 4;          // weight rows per wave (forward)
constexpr int IP_U = 4;          // steps of 64 lanes x 16 bytes per row issued before the first wait (forward): IP_R * IP_U KB per wave
constexpr int IP_WAVES = 4;      // waves per workgroup
constexpr int IP_NS_MAX = 256;   // rows of w per slice of the backward kernels (dY slice in LDS: MT * IP_NS_MAX floats)
constexpr int IP_UN = 8;         // rows of w in flight per lane (bwd_data)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T> struct Elem;
template <> struct Elem<float> {
    typedef f32x4 V;
    static constexpr int E = 4;
    static __device__ __forceinline__ V zero() { return V{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ float dot(V a, V b, float c) {
        c = __builtin_fmaf(a.x, b.x, c);
        c = __builtin_fmaf(a.y, b.y, c);
        c = __builtin_fmaf(a.z, b.z, c);
        return __builtin_fmaf(a.w, b.w, c);
    }
};
template <> struct Elem<_Float16> {
    typedef f16x8 V;
    static constexpr int E = 8;
    static __device__ __forceinline__ V zero() { return V{0, 0, 0, 0, 0, 0, 0, 0}; }
    // v_dot2_f32_f16: two half products added into a float32 accumulator
    static __device__ __forceinline__ float dot(V a, V b, float c) {
        c = __builtin_amdgcn_fdot2(f16x2{a[0], a[1]}, f16x2{b[0], b[1]}, c, false);
        c = __builtin_amdgcn_fdot2(f16x2{a[2], a[3]}, f16x2{b[2], b[3]}, c, false);
        c = __builtin_amdgcn_fdot2(f16x2{a[4], a[5]}, f16x2{b[4], b[5]}, c, false);
        return __builtin_amdgcn_fdot2(f16x2{a[6], a[7]}, f16x2{b[6], b[7]}, c, false);
    }
};

template <bool NT, typename V>
__device__ __forceinline__ V load16(const V* p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}

// sum over the 64 lanes in a fixed order; every lane ends with the total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct FwdArgs {
    const void* x;
    const void* w;
    const float* bias;
    void* y;
    float* ws;
    int x_rstride, y_cstride, y_coffset, M, K, N, flags, sps, S;
};

__device__ __forceinline__ void store_out(void* y, size_t i, float v, bool half) {
    if (half) reinterpret_cast<_Float16*>(y)[i] = (_Float16)v;
    else reinterpret_cast<float*>(y)[i] = v;
}

// grid: (ceil(N / (IP_R * IP_WAVES)), S).  a.sps: steps (of 64 * E elements) per K slice, a multiple of IP_U.
template <typename T, int MT, bool NT>
__global__ __launch_bounds__(64 * IP_WAVES) void ip_fwd_kernel(FwdArgs a) {
    typedef typename Elem<T>::V V;
    constexpr int E = Elem<T>::E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = ((int)blockIdx.x * IP_WAVES + wave) * IP_R;
    if (n0 >= a.N) return;                                   // no barrier below
    const int slice = blockIdx.y;
    const int K = a.K, M = a.M;
    const int k_begin = slice * a.sps * 64 * E;
    const int k_end = min(K, k_begin + a.sps * 64 * E);
    const T* __restrict__ w = reinterpret_cast<const T*>(a.w);
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
    size_t wrow[IP_R];
#pragma unroll
    for (int r = 0; r < IP_R; ++r) wrow[r] = (size_t)min(n0 + r, a.N - 1) * K;      // rows past N: a valid row, never stored

    float acc[IP_R][MT];
#pragma unroll
    for (int r = 0; r < IP_R; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;

    for (int kb = k_begin; kb < k_end; kb += IP_U * 64 * E) {
        V wv[IP_U][IP_R];
        int kk[IP_U];
        if (kb + IP_U * 64 * E <= k_end) {
#pragma unroll
            for (int u = 0; u < IP_U; ++u) {
                kk[u] = kb + (u * 64 + lane) * E;
#pragma unroll
                for (int r = 0; r < IP_R; ++r) wv[u][r] = load16<NT>(reinterpret_cast<const V*>(w + wrow[r] + kk[u]));
            }
        } else {                                             // the last steps of K: lanes past the end hold zeros and re-read k = 0
#pragma unroll
            for (int u = 0; u < IP_U; ++u) {
                const int k = kb + (u * 64 + lane) * E;
                const bool in = k < k_end;
                kk[u] = in ? k : 0;
#pragma unroll
                for (int r = 0; r < IP_R; ++r) {
                    wv[u][r] = Elem<T>::zero();
                    if (in) wv[u][r] = load16<NT>(reinterpret_cast<const V*>(w + wrow[r] + k));
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const size_t xrow = (size_t)min(m, M - 1) * a.x_rstride;      // rows past M: a valid row, never stored
            V xv[IP_U];
#pragma unroll
            for (int u = 0; u < IP_U; ++u) xv[u] = *reinterpret_cast<const V*>(x + xrow + kk[u]);
#pragma unroll
            for (int u = 0; u < IP_U; ++u)
#pragma unroll
                for (int r = 0; r < IP_R; ++r) acc[r][m] = Elem<T>::dot(wv[u][r], xv[u], acc[r][m]);
        }
    }

    // lane (r * MT + m) % 64 keeps the total of output (n0 + r, m)
    constexpr int KEEP = (IP_R * MT + 63) / 64;
    float keep[KEEP];
#pragma unroll
    for (int i = 0; i < KEEP; ++i) keep[i] = 0.f;
#pragma unroll
    for (int r = 0; r < IP_R; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const float t = wave_sum(acc[r][m]);
            const int idx = r * MT + m;
            if (lane == (idx & 63)) keep[idx >> 6] = t;
        }
#pragma unroll
    for (int i = 0; i < KEEP; ++i) {
        const int idx = i * 64 + lane;
        const int r = idx / MT, m = idx - r * MT, n = n0 + r;
        if (idx >= IP_R * MT || n >= a.N || m >= M) continue;
        float v = keep[i];
        if (a.S > 1) {
            a.ws[((size_t)slice * M + m) * a.N + n] = v;
        } else {
            if (a.bias) v += a.bias[n];
            if (a.flags & FCN_CONV_RELU) v = fmaxf(v, 0.f);
            store_out(a.y, (size_t)m * a.y_cstride + a.y_coffset + n, v, sizeof(T) == 2 && !(a.flags & FCN_CONV_OUT_F32));
        }
    }
}

// y[m][n] = act(sum over slices in slice order + bias): one lane per output
__global__ __launch_bounds__(256) void ip_fwd_combine_kernel(FwdArgs a, int half_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M * a.N) return;
    const int m = i / a.N, n = i - m * a.N;
    float v = 0.f;
    for (int s = 0; s < a.S; ++s) v += a.ws[((size_t)s * a.M + m) * a.N + n];
    if (a.bias) v += a.bias[n];
    if (a.flags & FCN_CONV_RELU) v = fmaxf(v, 0.f);
    store_out(a.y, (size_t)m * a.y_cstride + a.y_coffset + n, v, half_out != 0);
}

struct BwdArgs {
    const float* x;      // bwd_weights: the layer's input
    const float* dy;
    const float* w;      // bwd_data
    float* out;          // bwd_data: dX, or the slabs [S][M][K] when S > 1; bwd_weights: dW
    int x_rstride, dy_cstride, dy_coffset, out_rstride, M, K, N, NS, S, accumulate;
};

// dY of rows [ns0, ns0 + NS) of w into LDS as [MT][IP_NS_MAX], zeros past M and past N
template <int MT>
__device__ __forceinline__ void stage_dy(float (*sdy)[IP_NS_MAX], const BwdArgs& a, int ns0) {
    for (int i = threadIdx.x; i < MT * IP_NS_MAX; i += 64 * IP_WAVES) {
        const int m = i / IP_NS_MAX, j = i - m * IP_NS_MAX, n = ns0 + j;
        sdy[m][j] = (m < a.M && j < a.NS && n < a.N) ? a.dy[(size_t)m * a.dy_cstride + a.dy_coffset + n] : 0.f;
    }
    __syncthreads();
}

// grid: (ceil(K / 1024), S).  NS is a multiple of IP_UN.
template <int MT>
__global__ __launch_bounds__(64 * IP_WAVES) void ip_bwd_data_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sdy[MT][IP_NS_MAX];
    const int ns0 = (int)blockIdx.y * a.NS;
    stage_dy<MT>(sdy, a, ns0);
    const int k = ((int)blockIdx.x * 64 * IP_WAVES + (int)threadIdx.x) * 4;
    if (k >= a.K) return;                                    // K is a multiple of 4: a lane is inside with all four or outside
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ns1 = min(a.NS, a.N - ns0);                    // rows of this slice
    for (int j = 0; j < ns1; j += IP_UN) {
        f32x4 wv[IP_UN];
#pragma unroll
        for (int u = 0; u < IP_UN; ++u)                      // rows past N: row N - 1 again, against dY = 0
            wv[u] = *reinterpret_cast<const f32x4*>(a.w + (size_t)min(ns0 + j + u, a.N - 1) * a.K + k);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int u4 = 0; u4 < IP_UN; u4 += 4) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(&sdy[m][j + u4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[m].x = __builtin_fmaf(d[e], wv[u4 + e].x, acc[m].x);
                    acc[m].y = __builtin_fmaf(d[e], wv[u4 + e].y, acc[m].y);
                    acc[m].z = __builtin_fmaf(d[e], wv[u4 + e].z, acc[m].z);
                    acc[m].w = __builtin_fmaf(d[e], wv[u4 + e].w, acc[m].w);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (m < a.M && a.S > 1) {
            *reinterpret_cast<f32x4*>(a.out + ((size_t)blockIdx.y * a.M + m) * a.K + k) = acc[m];
        } else if (m < a.M) {
            f32x4* p = reinterpret_cast<f32x4*>(a.out + (size_t)m * a.out_rstride + k);
            *p = a.accumulate ? *p + acc[m] : acc[m];
        }
    }
}

// dX[m][k..k+3] (+)= sum over slices in slice order
__global__ __launch_bounds__(256) void ip_bwd_data_combine_kernel(const float* __restrict__ slabs, float* __restrict__ dx, int dx_rstride, int M,
                                                                  int K, int S, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, per = K / 4;
    if (i >= M * per) return;
    const int m = i / per, k = (i - m * per) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) v += *reinterpret_cast<const f32x4*>(slabs + ((size_t)s * M + m) * K + k);
    f32x4* p = reinterpret_cast<f32x4*>(dx + (size_t)m * dx_rstride + k);
    *p = accumulate ? *p + v : v;
}

// grid: (ceil(K / 1024), S).  NS is a multiple of 4.
template <int MT>
__global__ __launch_bounds__(64 * IP_WAVES) void ip_bwd_weights_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float sdy[MT][IP_NS_MAX];
    const int ns0 = (int)blockIdx.y * a.NS;
    stage_dy<MT>(sdy, a, ns0);
    const int k = ((int)blockIdx.x * 64 * IP_WAVES + (int)threadIdx.x) * 4;
    if (k >= a.K) return;
    f32x4 xv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        xv[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (m < a.M) xv[m] = *reinterpret_cast<const f32x4*>(a.x + (size_t)m * a.x_rstride + k);
    }
    const int ns1 = min(a.NS, a.N - ns0);
    for (int j = 0; j < ns1; j += 4) {
        f32x4 g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < MT; ++m) {                        // rows past M: dY = 0 and x = 0
            const f32x4 d = *reinterpret_cast<const f32x4*>(&sdy[m][j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                g[e].x = __builtin_fmaf(d[e], xv[m].x, g[e].x);
                g[e].y = __builtin_fmaf(d[e], xv[m].y, g[e].y);
                g[e].z = __builtin_fmaf(d[e], xv[m].z, g[e].z);
                g[e].w = __builtin_fmaf(d[e], xv[m].w, g[e].w);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j + e < ns1) {
                f32x4* p = reinterpret_cast<f32x4*>(a.out + (size_t)(ns0 + j + e) * a.K + k);
                *p = a.accumulate ? *p + g[e] : g[e];
            }
        }
    }
}

// db[n] (+)= sum over m in row order
__global__ __launch_bounds__(256) void ip_bias_grad_kernel(const float* __restrict__ dy, float* __restrict__ db, int dy_cstride, int dy_coffset,
                                                           int M, int N, int accumulate) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float v = 0.f;
    for (int m = 0; m < M; ++m) v += dy[(size_t)m * dy_cstride + dy_coffset + n];
    db[n] = accumulate ? db[n] + v : v;
}

// ---- host side ----
struct FwdPlan { int S, sps; };

// K slices so that about 2048 waves run (two per SIMD on 256 CUs), in whole groups of IP_U steps.  A function of the shape alone: the
// workspace query and the launch agree, and so do two runs.
FwdPlan fwd_plan(int K, int N, int E) {
    const int groups = cdiv(cdiv(K, 64 * E), IP_U), waves = cdiv(N, IP_R);
    int S = cdiv(2048, waves);
    if (S > groups) S = groups;
    const int gps = cdiv(groups, S);
    return FwdPlan{cdiv(groups, gps), gps * IP_U};
}

struct BwdPlan { int S, NS; };

BwdPlan bwd_plan(int K, int N, int target_wgs, int unit) {
    const int kwgs = cdiv(K, 1024);
    int S = cdiv(target_wgs, kwgs);
    if (S > N) S = N;
    int NS = cdiv(cdiv(N, S), unit) * unit;
    if (NS > IP_NS_MAX) NS = IP_NS_MAX;
    return BwdPlan{cdiv(N, NS), NS};
}
inline BwdPlan bwd_data_plan(int K, int N) { return bwd_plan(K, N, 256, IP_UN); }
inline BwdPlan bwd_weights_plan(int K, int N) { return bwd_plan(K, N, 1024, 4); }

int round_mt(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : M <= 16 ? 16 : 32; }

// the checks every entry point shares; every one precedes the first HIP call
int ip_check(const char* who, const void* a, const void* b, const void* c, int M, int K, int N, int E) {
    FCN_REQUIRE(a && b && c && M > 0 && K > 0 && N > 0, FCN_E_ARG, "%s: null pointer or non-positive extent", who);
    FCN_REQUIRE(K % E == 0 && aligned16(a) && aligned16(b) && aligned16(c), FCN_E_ALIGN,
                "%s: K must be a multiple of %d elements, pointers of 16 bytes", who, E);
    FCN_REQUIRE(M <= FCN_IP_MAX_ROWS, FCN_E_UNSUPPORTED, "%s: %d rows (at most %d: larger batches run through fcn_ip_gemm_*)", who, M,
                FCN_IP_MAX_ROWS);
    FCN_REQUIRE((long long)N * K < (1ll << 31), FCN_E_UNSUPPORTED, "%s: bank past 2^31 elements", who);
    return 0;
}

template <typename T>
int ip_fwd(const char* who, const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset, int M, int K,
           int N, int flags, void* d_workspace, fcn_stream_t s) {
    constexpr int E = 16 / (int)sizeof(T);
    if (int rc = ip_check(who, x, w, y, M, K, N, E)) return rc;
    const int allowed = sizeof(T) == 2 ? (FCN_CONV_RELU | FCN_CONV_OUT_F32 | FCN_IP_WEIGHTS_NT) : (FCN_CONV_RELU | FCN_IP_WEIGHTS_NT);
    FCN_REQUIRE((flags & ~allowed) == 0, FCN_E_ARG, "%s: flags 0x%x outside 0x%x", who, flags, allowed);
    const bool half_out = sizeof(T) == 2 && !(flags & FCN_CONV_OUT_F32);
    const int YE = half_out ? 8 : 4;
    FCN_REQUIRE(x_rstride >= K && y_coffset >= 0 && y_cstride >= y_coffset + N, FCN_E_ARG, "%s: row stride below K or slice out of range", who);
    FCN_REQUIRE(x_rstride % E == 0 && y_cstride % YE == 0 && (!bias || aligned16(bias)), FCN_E_ALIGN,
                "%s: strides must be multiples of 16 bytes, pointers of 16 bytes", who);
    FCN_REQUIRE((long long)M * x_rstride < (1ll << 31) && (long long)M * y_cstride < (1ll << 31), FCN_E_UNSUPPORTED, "%s: views past 2^31 elements",
                who);
    const FwdPlan p = fwd_plan(K, N, E);
    FCN_REQUIRE(p.S == 1 || (d_workspace && aligned16(d_workspace)), p.S == 1 || d_workspace ? FCN_E_ALIGN : FCN_E_ARG,
                "%s: this shape needs the workspace of fcn_inner_product_workspace_bytes (16-byte aligned)", who);
    FwdArgs a{x, w, bias, y, reinterpret_cast<float*>(d_workspace), x_rstride, y_cstride, y_coffset, M, K, N, flags & ~FCN_IP_WEIGHTS_NT, p.sps, p.S};
    const dim3 grid(cdiv(N, IP_R * IP_WAVES), p.S), block(64 * IP_WAVES);
    const bool nt = (flags & FCN_IP_WEIGHTS_NT) != 0;
#define FCN_IP_FWD(MT)                                                                              \
    case MT:                                                                                        \
        if (nt) hipLaunchKernelGGL((ip_fwd_kernel<T, MT, true>), grid, block, 0, as_stream(s), a);   \
        else hipLaunchKernelGGL((ip_fwd_kernel<T, MT, false>), grid, block, 0, as_stream(s), a);     \
        break;
    switch (round_mt(M)) {
        FCN_IP_FWD(1) FCN_IP_FWD(2) FCN_IP_FWD(4) FCN_IP_FWD(8) FCN_IP_FWD(16) FCN_IP_FWD(32)
    }
#undef FCN_IP_FWD
    FCN_LAUNCH_CHECK(who);
    if (p.S > 1) {
        hipLaunchKernelGGL(ip_fwd_combine_kernel, dim3(cdiv((long long)M * N, 256)), dim3(256), 0, as_stream(s), a, half_out ? 1 : 0);
        FCN_LAUNCH_CHECK(who);
    }
    return 0;
}

int bwd_check(const char* who, int M, int K, int N, int dy_cstride, int dy_coffset, int rstride) {
    FCN_REQUIRE(rstride >= K && dy_coffset >= 0 && dy_cstride >= dy_coffset + N, FCN_E_ARG, "%s: row stride below K or slice out of range", who);
    FCN_REQUIRE(rstride % 4 == 0 && dy_cstride % 4 == 0, FCN_E_ALIGN, "%s: strides must be multiples of 16 bytes", who);
    FCN_REQUIRE((long long)M * rstride < (1ll << 31) && (long long)M * dy_cstride < (1ll << 31), FCN_E_UNSUPPORTED, "%s: views past 2^31 elements",
                who);
    return 0;
}

}  // namespace

// the serial-over-M column sum, shared with ip_gemm.hip (common.h)
int fcn::ip_bias_grad(const char* who, const float* dy, float* db, int dy_cstride, int dy_coffset, int M, int N, int accumulate, fcn_stream_t s) {
    hipLaunchKernelGGL(ip_bias_grad_kernel, dim3(cdiv(N, 256)), dim3(256), 0, as_stream(s), dy, db, dy_cstride, dy_coffset, M, N, accumulate);
    FCN_LAUNCH_CHECK(who);
    return 0;
}

extern "C" {

size_t fcn_inner_product_fwd_workspace_bytes(int M, int K, int N, int esize) {
    if (M <= 0 || K <= 0 || N <= 0 || M > FCN_IP_MAX_ROWS || (esize != 2 && esize != 4)) return 0;
    const FwdPlan p = fwd_plan(K, N, 16 / esize);
    return p.S > 1 ? (size_t)p.S * M * N * 4 : 0;
}

size_t fcn_inner_product_workspace_bytes(int M, int K, int N) {
    if (M <= 0 || K <= 0 || N <= 0 || M > FCN_IP_MAX_ROWS) return 0;
    size_t need = 0;
    for (int E = 4; E <= 8; E += 4) {
        const FwdPlan p = fwd_plan(K, N, E);
        if (p.S > 1 && (size_t)p.S * M * N * 4 > need) need = (size_t)p.S * M * N * 4;
    }
    const BwdPlan b = bwd_data_plan(K, N);
    if (b.S > 1 && (size_t)b.S * M * K * 4 > need) need = (size_t)b.S * M * K * 4;
    return need;
}

int fcn_inner_product_fwd_f32(const float* x, int x_rstride, const float* w, const float* bias, float* y, int y_cstride, int y_coffset, int M,
                              int K, int N, int flags, void* d_workspace, fcn_stream_t s) {
    return ip_fwd<float>("inner_product_fwd_f32", x, x_rstride, w, bias, y, y_cstride, y_coffset, M, K, N, flags, d_workspace, s);
}

int fcn_inner_product_fwd_f16(const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset, int M, int K,
                              int N, int flags, void* d_workspace, fcn_stream_t s) {
    return ip_fwd<_Float16>("inner_product_fwd_f16", x, x_rstride, w, bias, y, y_cstride, y_coffset, M, K, N, flags, d_workspace, s);
}

int fcn_inner_product_bwd_data_f32(const float* dy, int dy_cstride, int dy_coffset, const float* w, float* dx, int dx_rstride, int M, int K, int N,
                                   int flags, void* d_workspace, fcn_stream_t s) {
    const char* who = "inner_product_bwd_data_f32";
    if (int rc = ip_check(who, dy, w, dx, M, K, N, 4)) return rc;
    FCN_REQUIRE((flags & ~FCN_CONV_ACCUM) == 0, FCN_E_ARG, "%s: flags 0x%x outside FCN_CONV_ACCUM", who, flags);
    if (int rc = bwd_check(who, M, K, N, dy_cstride, dy_coffset, dx_rstride)) return rc;
    const BwdPlan p = bwd_data_plan(K, N);
    FCN_REQUIRE(p.S == 1 || (d_workspace && aligned16(d_workspace)), p.S == 1 || d_workspace ? FCN_E_ALIGN : FCN_E_ARG,
                "%s: this shape needs the workspace of fcn_inner_product_workspace_bytes (16-byte aligned)", who);
    const int acc = (flags & FCN_CONV_ACCUM) ? 1 : 0;
    BwdArgs a{nullptr, dy, w, p.S > 1 ? reinterpret_cast<float*>(d_workspace) : dx, 0, dy_cstride, dy_coffset, dx_rstride, M, K, N, p.NS, p.S, acc};
    const dim3 grid(cdiv(K, 256 * IP_WAVES), p.S), block(64 * IP_WAVES);
#define FCN_IP_BWD(MT) case MT: hipLaunchKernelGGL((ip_bwd_data_kernel<MT>), grid, block, 0, as_stream(s), a); break;
    switch (round_mt(M)) { FCN_IP_BWD(1) FCN_IP_BWD(2) FCN_IP_BWD(4) FCN_IP_BWD(8) FCN_IP_BWD(16) FCN_IP_BWD(32) }
#undef FCN_IP_BWD
    FCN_LAUNCH_CHECK(who);
    if (p.S > 1) {
        hipLaunchKernelGGL(ip_bwd_data_combine_kernel, dim3(cdiv((long long)M * (K / 4), 256)), dim3(256), 0, as_stream(s),
                           reinterpret_cast<const float*>(d_workspace), dx, dx_rstride, M, K, p.S, acc);
        FCN_LAUNCH_CHECK(who);
    }
    return 0;
}

int fcn_inner_product_bwd_weights_f32(const float* x, int x_rstride, const float* dy, int dy_cstride, int dy_coffset, float* dw, float* db, int M,
                                      int K, int N, int accumulate, fcn_stream_t s) {
    const char* who = "inner_product_bwd_weights_f32";
    if (int rc = ip_check(who, x, dy, dw, M, K, N, 4)) return rc;
    FCN_REQUIRE(accumulate == 0 || accumulate == 1, FCN_E_ARG, "%s: accumulate must be 0 or 1", who);
    if (int rc = bwd_check(who, M, K, N, dy_cstride, dy_coffset, x_rstride)) return rc;
    FCN_REQUIRE(!db || aligned16(db), FCN_E_ALIGN, "%s: db must be 16-byte aligned", who);
    const BwdPlan p = bwd_weights_plan(K, N);
    BwdArgs a{x, dy, nullptr, dw, x_rstride, dy_cstride, dy_coffset, K, M, K, N, p.NS, p.S, accumulate};
    const dim3 grid(cdiv(K, 256 * IP_WAVES), p.S), block(64 * IP_WAVES);
#define FCN_IP_BWD(MT) case MT: hipLaunchKernelGGL((ip_bwd_weights_kernel<MT>), grid, block, 0, as_stream(s), a); break;
    switch (round_mt(M)) { FCN_IP_BWD(1) FCN_IP_BWD(2) FCN_IP_BWD(4) FCN_IP_BWD(8) FCN_IP_BWD(16) FCN_IP_BWD(32) }
#undef FCN_IP_BWD
    FCN_LAUNCH_CHECK(who);
    if (db) return ip_bias_grad(who, dy, db, dy_cstride, dy_coffset, M, N, accumulate, s);
    return 0;
}

}  // extern "C"
