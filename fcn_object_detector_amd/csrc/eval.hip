// Validation-pass kernels (Solver::Test, `caffe test`): the running sum of a net's output blobs over test_iter forwards, kept in
// HBM, and Caffe's Accuracy layer.  Both sit inside the test engine's captured forward graph, so a whole pass is test_iter graph
// launches and one read-back.
#include "common.h"

namespace fcn {

// ---------------------------------------------------------------------------------------------------------------------------
// acc[n][c][p] += x[n][p][coffset + c]: an NHWC view with a padded channel stride summed into an NCHW accumulator.
// One workgroup moves a tile of 64 pixels x 16 channels through LDS: the read is contiguous along the channels of a pixel (16-byte
// loads when the view is aligned and a whole quad lies inside the view), the read-modify-write of the accumulator is contiguous
// along the pixels of a channel.  Exactly one float add per element per call; padding channels are neither read nor written.
constexpr int SA_TP = 64, SA_TC = 16;
__global__ __launch_bounds__(256) void score_accumulate_tile_kernel(float* __restrict__ acc, const float* __restrict__ x, int pixels, int C,
                                                                    int x_cstride, int x_coffset, int vec) {
    __shared__ float tile[SA_TC][SA_TP + 1];
    const int n = blockIdx.z, c0 = blockIdx.y * SA_TC, p0 = blockIdx.x * SA_TP;
    const int tid = threadIdx.x;
    {
        const int p = tid >> 2, q = (tid & 3) * 4;      // four lanes cover the 16 channels of one pixel
        if (p0 + p < pixels) {
            const float* src = x + ((size_t)n * pixels + p0 + p) * x_cstride + x_coffset + c0 + q;
            if (vec && c0 + q + 3 < C) {
                const float4 v = *reinterpret_cast<const float4*>(src);
                tile[q][p] = v.x;
                tile[q + 1][p] = v.y;
                tile[q + 2][p] = v.z;
                tile[q + 3][p] = v.w;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (c0 + q + k < C) tile[q + k][p] = src[k];
            }
        }
    }
    __syncthreads();
    const int p = tid & 63, cg = (tid >> 6) * 4;      // one wave per four channels, its lanes along the pixels
    if (p0 + p < pixels) {
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + cg + k;
            if (c < C) {
                float* a = acc + ((size_t)n * C + c) * pixels + p0 + p;
                *a = *a + tile[cg + k][p];
            }
        }
    }
}

// pixels == 1 (loss scalars, the Accuracy tops): NHWC and NCHW order agree, one element per lane
__global__ __launch_bounds__(256) void score_accumulate_flat_kernel(float* __restrict__ acc, const float* __restrict__ x, int N, int C,
                                                                    int x_cstride, int x_coffset) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * C) return;
    const int n = t / C, c = t - n * C;
    acc[t] = acc[t] + x[(size_t)n * x_cstride + x_coffset + c];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Accuracy (BVLC Caffe master's AccuracyLayer over the channel axis).  One lane owns one pixel's channel vector (C is 2..21 in
// the nets this is for); counts are integers: per-workgroup partials in the workspace, then one workgroup sums them in index order.
constexpr int ACC_MAX_BLOCKS = 256;
constexpr int ACC_MAX_CLASSES = 128;      // with per-class output (workspace rows hold 2 + 2 * C counts)

__global__ __launch_bounds__(256) void accuracy_partial_kernel(const float* __restrict__ x, const float* __restrict__ label,
                                                               int* __restrict__ partial, long long pixels, int C, int x_cstride,
                                                               int label_cstride, int top_k, int has_ignore, int ignore_label, int per_class,
                                                               int vec) {
    __shared__ int s_ok[256], s_n[256];
    __shared__ int s_cls[2 * ACC_MAX_CLASSES];      // [c] labelled pixels of class c, [C + c] the correct ones among them
    if (per_class) {
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) s_cls[i] = 0;
        __syncthreads();
    }
    int ok = 0, cnt = 0;
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < pixels; pix += (long long)gridDim.x * blockDim.x) {
        const int lab = (int)label[(size_t)pix * label_cstride];
        if (has_ignore && lab == ignore_label) continue;
        ++cnt;
        if (lab < 0 || lab >= C) continue;      // counted, wrong, and never used as an index
        const float* xp = x + (size_t)pix * x_cstride;
        const float xl = xp[lab];
        int ge = 0;      // channels other than the label whose score is at least the label's: ties count against the label
        int c = 0;
        if (vec) {
            for (; c + 3 < C; c += 4) {
                const float4 v = *reinterpret_cast<const float4*>(xp + c);
                ge += (v.x >= xl && c != lab) + (v.y >= xl && c + 1 != lab) + (v.z >= xl && c + 2 != lab) + (v.w >= xl && c + 3 != lab);
            }
        }
        for (; c < C; ++c) ge += (xp[c] >= xl && c != lab);
        const int good = ge < top_k;
        ok += good;
        if (per_class) {
            atomicAdd(&s_cls[lab], 1);
            if (good) atomicAdd(&s_cls[C + lab], 1);
        }
    }
    s_ok[threadIdx.x] = ok;
    s_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_ok[threadIdx.x] += s_ok[threadIdx.x + o];
            s_n[threadIdx.x] += s_n[threadIdx.x + o];
        }
        __syncthreads();
    }
    const int row = per_class ? 2 + 2 * C : 2;
    int* out = partial + (size_t)blockIdx.x * row;
    if (threadIdx.x == 0) {
        out[0] = s_ok[0];
        out[1] = s_n[0];
    }
    if (per_class)
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) out[2 + i] = s_cls[i];
}

__global__ __launch_bounds__(64) void accuracy_final_kernel(const int* __restrict__ partial, int nblocks, int C, float* __restrict__ d_acc,
                                                            float* __restrict__ d_per_class) {
    const int row = d_per_class ? 2 + 2 * C : 2;
    if (threadIdx.x == 0) {
        long long ok = 0, cnt = 0;
        for (int b = 0; b < nblocks; ++b) {
            ok += partial[(size_t)b * row];
            cnt += partial[(size_t)b * row + 1];
        }
        *d_acc = cnt ? (float)ok / (float)cnt : 0.f;
    }
    if (d_per_class) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            long long n_c = 0, ok_c = 0;
            for (int b = 0; b < nblocks; ++b) {
                n_c += partial[(size_t)b * row + 2 + c];
                ok_c += partial[(size_t)b * row + 2 + C + c];
            }
            d_per_class[c] = n_c ? (float)ok_c / (float)n_c : 0.f;
        }
    }
}

}  // namespace fcn

using namespace fcn;

extern "C" {

int fcn_score_accumulate_f32(float* acc, const float* x, int N, int pixels, int C, int x_cstride, int x_coffset, fcn_stream_t s) {
    FCN_REQUIRE(acc && x && N > 0 && pixels > 0 && C > 0 && x_coffset >= 0 && x_cstride >= x_coffset + C, FCN_E_ARG,
                "score_accumulate: bad args");
    FCN_REQUIRE(N <= 65535 && (long long)N * C <= 0x7fffffffLL, FCN_E_ARG, "score_accumulate: batch too large");
    hipStream_t st = as_stream(s);
    if (pixels == 1) {
        hipLaunchKernelGGL(score_accumulate_flat_kernel, dim3(cdiv((long long)N * C, 256)), dim3(256), 0, st, acc, x, N, C, x_cstride, x_coffset);
    } else {
        const int vec = ((uintptr_t)x & 15) == 0 && x_cstride % 4 == 0 && x_coffset % 4 == 0;
        hipLaunchKernelGGL(score_accumulate_tile_kernel, dim3(cdiv(pixels, SA_TP), cdiv(C, SA_TC), N), dim3(256), 0, st, acc, x, pixels, C,
                           x_cstride, x_coffset, vec);
    }
    FCN_LAUNCH_CHECK("score_accumulate");
    return 0;
}

size_t fcn_accuracy_workspace_bytes(void) { return (size_t)ACC_MAX_BLOCKS * (2 + 2 * ACC_MAX_CLASSES) * sizeof(int); }

int fcn_accuracy_f32(const float* x, const float* label, float* d_acc, float* d_per_class, int N, int pixels, int C, int x_cstride,
                     int label_cstride, int top_k, int has_ignore, int ignore_label, void* d_workspace, fcn_stream_t s) {
    FCN_REQUIRE(x && label && d_acc && d_workspace && N > 0 && pixels > 0 && C > 0 && x_cstride >= C && label_cstride >= 1 && top_k >= 1,
                FCN_E_ARG, "accuracy: bad args");
    FCN_REQUIRE(!d_per_class || C <= ACC_MAX_CLASSES, FCN_E_ARG, "accuracy: per-class output for at most %d classes", ACC_MAX_CLASSES);
    FCN_REQUIRE(((uintptr_t)d_workspace & 3) == 0, FCN_E_ALIGN, "accuracy: workspace must be 4-byte aligned");
    hipStream_t st = as_stream(s);
    int blocks = cdiv(pixels, 256);
    if (blocks > ACC_MAX_BLOCKS) blocks = ACC_MAX_BLOCKS;
    int* partial = reinterpret_cast<int*>(d_workspace);
    const int vec = ((uintptr_t)x & 15) == 0 && x_cstride % 4 == 0;
    hipLaunchKernelGGL(accuracy_partial_kernel, dim3(blocks), dim3(256), 0, st, x, label, partial, (long long)pixels, C, x_cstride,
                       label_cstride, top_k, has_ignore, ignore_label, d_per_class ? 1 : 0, vec);
    hipLaunchKernelGGL(accuracy_final_kernel, dim3(1), dim3(64), 0, st, partial, blocks, C, d_acc, d_per_class);
    FCN_LAUNCH_CHECK("accuracy");
    return 0;
}

}  // extern "C"
