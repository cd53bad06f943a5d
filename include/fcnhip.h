/*
 * fcnhip.h — C ABI of libfcnhip.so, the MI355X (gfx950) engine behind the
 * pycaffe-compatible shim in fcn_object_detector_amd/python/caffe.
 *
 * The reference has no FFI of its own for this path: its arithmetic lives in an
 * external Caffe install reached through pycaffe (reference:
 * scripts/fcn_object_detector.py:9,68-69,87,317 and
 * scripts/data_argumentation_layer/data_argumentation_layer.py:4,14) and through
 * the `caffe train` binary (reference: train/train.sh:25-28).  Each entry point
 * below names the Caffe/OpenCV call of the reference it stands in for.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless its name starts
 *     with h_; shapes are int32; activations are NHWC float32 with an explicit
 *     channel stride (`*_cstride`, floats per pixel) so several producers can write
 *     channel slices of one buffer (Concat without a copy);
 *   - every function returns 0 on success, a negative value = -hipError_t, a positive
 *     value = argument-validation code (FCN_E_*); fcn_last_error_string() returns a
 *     thread-local message.  Nothing aborts, nothing prints;
 *   - everything is enqueued on the caller's stream (fcn_stream_t, may be NULL for the
 *     default stream) and is asynchronous unless the name ends in _sync;
 *   - the caller owns every buffer; the library keeps no pointer past a call except
 *     inside an fcn_graph_t it was asked to capture.
 */
#ifndef FCNHIP_H_
#define FCNHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCN_ABI_VERSION 2

/* argument-validation codes (positive returns) */
#define FCN_E_ARG       1   /* null pointer / non-positive extent            */
#define FCN_E_ALIGN     2   /* channel count / stride / pointer not 16-B ok  */
#define FCN_E_UNSUPPORTED 3 /* geometry the kernels do not implement          */
#define FCN_E_STATE     4   /* call not valid in the current state            */
#define FCN_E_CAPACITY  5   /* output capacity too small                      */

typedef void* fcn_stream_t;
typedef void* fcn_event_t;
typedef void* fcn_graph_t;
typedef void* fcn_comm_t;

/* ---- runtime: replaces caffe.set_device / set_mode_gpu (fcn_object_detector.py:68-69)
 *      and Caffe's SyncedMemory allocation + H<->D copies behind blob.data ---- */
int  fcn_abi_version(void);
const char* fcn_last_error_string(void);
int  fcn_device_count(int* count);
int  fcn_init(int device);                 /* per-thread hipSetDevice; idempotent, thread-safe */
int  fcn_device_name(char* h_buf, int len);
int  fcn_device_sync(void);
int  fcn_malloc(void** p, size_t bytes);
int  fcn_free(void* p);
int  fcn_host_malloc(void** h_p, size_t bytes);   /* pinned host memory for blob.data views */
int  fcn_host_free(void* h_p);
int  fcn_memset_async(void* p, int value, size_t bytes, fcn_stream_t s);
int  fcn_memcpy_h2d_async(void* dst, const void* h_src, size_t bytes, fcn_stream_t s);
int  fcn_memcpy_d2h_async(void* h_dst, const void* src, size_t bytes, fcn_stream_t s);
int  fcn_memcpy_d2d_async(void* dst, const void* src, size_t bytes, fcn_stream_t s);
int  fcn_stream_create(fcn_stream_t* s);
int  fcn_stream_destroy(fcn_stream_t s);
int  fcn_stream_sync(fcn_stream_t s);
int  fcn_event_create(fcn_event_t* e);
int  fcn_event_destroy(fcn_event_t e);
int  fcn_event_record(fcn_event_t e, fcn_stream_t s);
int  fcn_event_sync(fcn_event_t e);
int  fcn_event_elapsed_ms(fcn_event_t start, fcn_event_t stop, float* h_ms);
int  fcn_stream_wait_event(fcn_stream_t s, fcn_event_t e);   /* later work on s waits for e (overlap of collectives) */
/* hipGraph capture of a whole Net::Forward / ForwardBackward launch sequence */
int  fcn_graph_begin(fcn_stream_t s);
int  fcn_graph_end(fcn_stream_t s, fcn_graph_t* g);
int  fcn_graph_launch(fcn_graph_t g, fcn_stream_t s);
int  fcn_graph_destroy(fcn_graph_t g);
/* The stream of replica `index` of a frame pipeline (several engines of one net, one frame each in flight): non-blocking like
 * fcn_stream_create's, created at the HIGHEST stream priority the device reports.  The HIP runtime hands out hardware queues from one
 * pool per priority, each pool as large as the process's queue limit (4 by default): the replicas' streams then share no hardware queue
 * with the null stream or with the process's plain streams.  All replicas take the same priority, so none outranks another - but they do
 * outrank the process's plain streams (and work of other processes at normal priority) wherever the hardware arbitrates between queues.
 * A pool holds as many queues as the limit: replicas 0 .. FCN_REPLICA_STREAMS - 1 (the default limit) take priority streams; a higher or
 * negative index would only alias a queue inside that pool and takes a plain stream instead, as does every index on a device without
 * stream priorities or under a runtime that refuses the request.  fcn_stream_is_prioritized reports which kind a stream is (*h_yes = 1:
 * created at the device's highest priority, and the device has more than one; else 0).  Destroyed with fcn_stream_destroy. */
#define FCN_REPLICA_STREAMS 4
int  fcn_stream_create_replica(fcn_stream_t* s, int index);
int  fcn_stream_is_prioritized(fcn_stream_t s, int* h_yes);

/* ---- blob layout at the pycaffe boundary (blob.data is NCHW) ---- */
/* dst[n,h,w,dst_coffset + c] = src[n,c,h,w] + shift; dst channel stride dst_cstride.  `shift` lets the
 * upload of the net input absorb a following Power(shift) layer (models/deploy.prototxt:8-16). */
int  fcn_nchw_to_nhwc_f32(const float* src, float* dst, int N, int C, int H, int W,
                          int dst_cstride, int dst_coffset, float shift, fcn_stream_t s);
int  fcn_nhwc_to_nchw_f32(const float* src, float* dst, int N, int C, int H, int W,
                          int src_cstride, int src_coffset, fcn_stream_t s);
/* several (small) blobs in ONE launch - net.forward() hands back both head blobs of models/deploy.prototxt with it (up to 8 blobs) */
typedef struct fcn_layout_desc {
    const float* src;   /* NHWC, channel stride src_cstride, the blob's channels at src_coffset .. */
    float* dst;         /* NCHW, dense */
    int32_t N, C, H, W, src_cstride, src_coffset;
} fcn_layout_desc;
int  fcn_nhwc_to_nchw_multi_f32(const fcn_layout_desc* h_descs, int n, fcn_stream_t s);

/* ---- Convolution (+bias, fused in-place ReLU / Sigmoid):
 *      Caffe ConvolutionLayer::Forward_gpu, ReLULayer, SigmoidLayer as run by
 *      net.forward() (fcn_object_detector.py:87) over models/deploy.prototxt:8-2176 ---- */
#define FCN_CONV_RELU      1   /* y = max(y, 0)                                  */
#define FCN_CONV_SIGMOID2  2   /* y2 = sigmoid(y) is written as well (y2 != NULL) */
#define FCN_CONV_ACCUM     4   /* y += result (gradient fan-in when the kernel runs as a data-gradient pass) */
#define FCN_CONV_MASK     64   /* y = (y2 > 0) ? result : 0 with y2 read at the result's position (y2_cstride / y2_coffset): the ReLU
                                * backward of the layer below, applied by the LAST data-gradient pass that writes its gradient   */
#define FCN_CONV_IMAGE_ONES 128 /* with FCN_CONV_F16 on an 8-half pixel image (the first layer of an f16 net): the caller promises that channels 3
                                * and 4 of x hold the constant 1 at every pixel and channels 5..7 contribute nothing (zero pixels or zero
                                * weights) - the folded Power shift of models/deploy.prototxt:8-16.  Their products are then added
                                * as per-tap constants (f32) instead of being multiplied; pixels outside the image count as 0, as ever.
                                * What the half first-layer kernels READ (tests/test_gpu_guarded_f16.py pins it): with this flag
                                * (conv_first7_f16x4_kernel) halves 0..3 of every pixel and halves 0..4 of every filter tap - halves 4..7
                                * of a pixel and 5..7 of a tap are NOT READ and may hold anything; without it (conv_first7_f16_kernel, and
                                * the tiled kernels) all eight halves of pixel and tap are loaded and MULTIPLIED, so the pad channels must
                                * be the caller's zeros (a NaN times zero is a NaN).  Cout: a multiple of 8 in 40 .. 64 */
#define FCN_CONV_OUT_F32   8   /* with FCN_CONV_F16: y is float32 (the detection heads feed the f32 decode kernel)   */
#define FCN_CONV_OUT_F16  32   /* float32 x and w, y stored as half floats: the first layer of an f16 net keeps its input in
                                * float32 (models/deploy.prototxt shifts a [0,1] image by -127: 16 half-float levels)   */
#define FCN_CONV_F16      16   /* x, w and y hold IEEE half floats (v_mfma_f32_32x32x16_f16, f32 accumulate, f32 bias):
                                * BASELINE configs[4].  Cin and x_cstride must then be multiples of 8; the pointers of
                                * the descriptor are typed float* for both element types */
typedef struct fcn_conv_desc {
    const float* x;      /* NHWC input, channel stride x_cstride                           */
    const float* w;      /* weights [Cout][kh][kw][Cin]  (OHWI, Cin contiguous)            */
    const float* bias;   /* [Cout] or NULL                                                 */
    float*       y;      /* NHWC output; element (m, n) at y[m*y_cstride + y_coffset + n]  */
    float*       y2;     /* second output for FCN_CONV_SIGMOID2 (same indexing via y2_*)   */
    int32_t N, H, W, Cin, x_cstride;
    int32_t Cout, kh, kw, pad, stride, OH, OW;
    int32_t y_cstride, y_coffset, y2_cstride, y2_coffset;
    int32_t flags;
    float   in_shift;    /* reserved, must be 0 (a Power(shift) input transform is applied by the producer of x) */
} fcn_conv_desc;
/* one problem */
int  fcn_conv2d_fwd_f32(const fcn_conv_desc* h_desc, fcn_stream_t s);
/* n independent problems in ONE launch (the branches of an inception module).  prepare() validates
 * and uploads the problems into d_workspace (fcn_conv2d_group_workspace_bytes(n) bytes, owned by
 * the caller, alive as long as the group is used) with a synchronous copy - call it at plan time,
 * not inside a graph capture; the launch itself is a pure kernel launch and can be captured. */
typedef struct fcn_conv_group {
    void*   d_probs;
    int32_t n;
    int32_t cfg;          /* tile configuration chosen by prepare() */
    int32_t total_tiles;
} fcn_conv_group;
size_t fcn_conv2d_group_workspace_bytes(int n);
/* cfg_request: -1 = built-in heuristic, 0 .. fcn_conv2d_num_configs()-1 = that tile configuration (the engine
 * times every configuration once per launch at plan time and keeps the fastest) */
int  fcn_conv2d_num_configs(void);
/* The last two configurations are not tile shapes of the implicit-GEMM kernel but shape-specific kernels; prepare() returns
 * FCN_E_UNSUPPORTED when one is requested for a group it does not take (a tuner walking all configurations skips those):
 *   fcn_conv2d_first_layer_config()      conv_first7_kernel: a single 7x7 / stride 2 / pad 3 problem on 4-channel pixels with
 *                                        33..64 output channels (conv1/7x7_s2 of models/deploy.prototxt), ReLU optional; the
 *                                        built-in heuristic picks it for the problems it takes.  It multiplies channels 0..2 ONLY:
 *                                        channel 3 of every pixel of x and of every filter tap of w is the pad channel of a
 *                                        3-channel image and is NOT READ (it may hold anything; a net with four real input
 *                                        channels must keep this kernel off - FCN_CONV_FIRST7=0 - or give its first layer
 *                                        another width).  tests/test_gpu_guarded.py::test_first_layer_kernel pins it;
 *   fcn_conv2d_first_layer_config() + 1  conv_dot1x1_kernel: groups of 1x1 / stride 1 / unpadded float32 problems over the same
 *                                        pixels with at most 32 output channels in all, counted in slices of 8 per problem (the
 *                                        detection heads cvg/classifier + bbox/regressor); ReLU and FCN_CONV_SIGMOID2 allowed. */
int  fcn_conv2d_first_layer_config(void);
/* A "tail": narrow 1x1 problems (the detection heads cvg/classifier + bbox/regressor, deploy.prototxt:2363-2410 - 4 + 16 outputs over the
 * 1024 channels of inception_5b/output) evaluated BY THE LAUNCHES THAT PRODUCE THEIR INPUT instead of a launch of their own: every tile
 * that has written 32 channels of a block of pixels leaves their contribution to the narrow outputs in `scratch`, and the tile that
 * arrives last at a pixel block adds the contributions in channel order (a fixed order: bit-reproducible), applies bias / ReLU /
 * sigmoid and writes the narrow problems' outputs.  Announce the tail for a workspace BEFORE fcn_conv2d_group_prepare[_fused] on that
 * workspace; every problem of the group whose y is heads[0].x then contributes (it must be a float32 bias + ReLU problem over the same
 * pixels writing whole 32-channel groups of that blob).  finalize = 1 for the launch that completes the blob, 0 for an earlier launch
 * that writes part of it (partial sums only).  Tile configurations 23, 24, 25 and 27 have a tail variant; prepare() returns
 * FCN_E_UNSUPPORTED for the others.  heads: float32 1x1 / stride 1 problems reading the same blob, outputs in whole groups of four
 * channels, at most 24 in all; flags within FCN_CONV_RELU | FCN_CONV_SIGMOID2.  scratch / arrive: device memory of
 * fcn_conv2d_tail_scratch_bytes() / fcn_conv2d_tail_arrive_bytes() bytes, arrive zeroed once by the caller (launches leave it zero);
 * two launches that share them must not overlap in time.  fcn_conv2d_group_attach_tail(ws, NULL) and fcn_conv2d_group_release(ws) forget it. */
typedef struct fcn_conv_tail {
    int32_t n;                 /* 1..4 narrow problems */
    int32_t finalize;
    fcn_conv_desc heads[4];
    float*  scratch;
    void*   arrive;
} fcn_conv_tail;
size_t fcn_conv2d_tail_scratch_bytes(const fcn_conv_tail* t);
size_t fcn_conv2d_tail_arrive_bytes(const fcn_conv_tail* t);
int  fcn_conv2d_group_attach_tail(void* d_workspace, const fcn_conv_tail* t);
/* LDS bytes one workgroup of that configuration holds (a CU has 160 KiB: it bounds how many workgroups - of this or of a
 * concurrent launch on another stream - fit on a CU); -1 for an unknown index */
int  fcn_conv2d_config_lds_bytes(int cfg);
/* how many waves of a workgroup split K and reduce through LDS in that configuration (1 = no K split); -1 for an unknown index */
int  fcn_conv2d_config_waves_k(int cfg);
int  fcn_conv2d_group_prepare(const fcn_conv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_conv_group* h_out);
int  fcn_conv2d_fwd_group_f32(const fcn_conv_group* h_group, fcn_stream_t s);
/* MAX poolings that read the same bottoms as the group's convolutions (an inception module's 3x3 stride-1 pool beside
 * its 1x1 convolutions) can ride in the group's launch as extra workgroups instead of a launch of their own.
 * Needs C, x_cstride, y_cstride, y_coffset multiples of 4 and 16-byte aligned pointers; idx may be NULL. */
typedef struct fcn_pool_desc {
    const float* x; float* y; int32_t* idx;
    int32_t N, H, W, C, x_cstride, k, stride, pad, OH, OW, y_cstride, y_coffset;
    int32_t f16;           /* 1: x / y hold half floats (C and the strides then multiples of 8), must match the group's convolutions */
} fcn_pool_desc;
int  fcn_conv2d_group_prepare_fused(const fcn_conv_desc* h_descs, int n, const fcn_pool_desc* h_pools, int npools, void* d_workspace,
                                    int cfg_request, fcn_conv_group* h_out);
/* The library keeps a host copy of every prepared group, keyed by its d_workspace.  Call this before freeing (or reusing for
 * something else) a workspace that was handed to a prepare call: the entry is erased, so that a later allocation that happens
 * to get the same device address can never pick up a stale plan.  Unknown pointers are ignored (returns 0). */
int  fcn_conv2d_group_release(void* d_workspace);

/* ---- Pooling / LRN / pointwise: Caffe PoolingLayer, LRNLayer, EltwiseLayer ---- */
/* MAX pool, ceil-mode output size computed by the caller (OH, OW), window clipped to the
 * image, first maximum in raster order wins; idx (may be NULL) receives iy*W+ix per output */
int  fcn_maxpool_fwd_f32(const float* x, float* y, int32_t* idx, int N, int H, int W, int C,
                         int x_cstride, int k, int stride, int pad, int OH, int OW,
                         int y_cstride, int y_coffset, fcn_stream_t s);
int  fcn_avepool_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride,
                         int k, int stride, int pad, int OH, int OW, int y_cstride, int y_coffset,
                         fcn_stream_t s);
/* LRN ACROSS_CHANNELS: y = x * (k + alpha/n * sum x^2)^-beta ; scale (may be NULL) keeps the base */
int  fcn_lrn_fwd_f32(const float* x, float* y, float* scale, int pixels, int C, int x_cstride,
                     int y_cstride, int local_size, float alpha, float beta, float k, fcn_stream_t s);
/* MAX pooling and LRN (ACROSS_CHANNELS, local_size 5) of one blob in a single pass, inference only: lrn_first 0 computes
 * LRN(maxpool(x)) (deploy.prototxt pool1/3x3_s2 -> pool1/norm1), 1 computes maxpool(LRN(x)) (conv2/norm2 -> pool2/3x3_s2);
 * the blob between the two layers is never written.  C, the strides and the pointers must allow 16-byte channel groups
 * (FCN_E_UNSUPPORTED otherwise: run fcn_maxpool_fwd_f32 and fcn_lrn_fwd_f32). */
int  fcn_maxpool_lrn5_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad,
                              int OH, int OW, int y_cstride, int lrn_first, float alpha, float beta, float lrn_k, fcn_stream_t s);
/* pool -> LRN -> 1x1 convolution (+ bias, optional ReLU) in ONE launch: deploy.prototxt pool1/3x3_s2 -> pool1/norm1 ->
 * conv2/3x3_reduce (:54-104).  y[pixel][y_coffset + co] = act(bias[co] + sum_c w[co][c] * LRN(maxpool(x))[pixel][c]); w is
 * [Cout][C] row-major.  Neither the pooled nor the normalised blob is written.  3 x 3 windows and 64 -> 64 channels only
 * (FCN_E_UNSUPPORTED otherwise: fcn_maxpool_lrn5_fwd_f32 + fcn_conv2d_fwd_f32).  The pooling is exact; the LRN takes s^-0.75 from the
 * hardware reciprocal square root / square root (1 ulp each: within 1e-6 of fcn_maxpool_lrn5_fwd_f32(lrn_first = 0)); the convolution
 * sums K on the matrix cores in its own order (float32). */
int  fcn_maxpool_lrn5_conv1x1_fwd_f32(const float* x, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad,
                                      int OH, int OW, float alpha, float beta, float lrn_k, const float* w, const float* bias,
                                      int Cout, int relu, float* y, int y_cstride, int y_coffset, fcn_stream_t s);
/* the half twin (x, w, y hold halves, bias float32; 3 x 3 / stride 2 / unpadded windows only): the LDS-patch form of
 * fcn_maxpool_lrn5_fwd_f16 whose last step multiplies the normalised tile by the filter bank (v_mfma_f32_16x16x16_f16, f32 accumulate,
 * one rounding after bias and ReLU) */
int  fcn_maxpool_lrn5_conv1x1_fwd_f16(const void* x, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad,
                                      int OH, int OW, float alpha, float beta, float lrn_k, const void* w, const float* bias,
                                      int Cout, int relu, void* y, int y_cstride, int y_coffset, fcn_stream_t s);
int  fcn_relu_fwd_f32(const float* x, float* y, size_t count, float negative_slope, fcn_stream_t s);
int  fcn_sigmoid_fwd_f32(const float* x, float* y, size_t count, fcn_stream_t s);
int  fcn_power_fwd_f32(const float* x, float* y, size_t count, float power, float scale, float shift, fcn_stream_t s);
#define FCN_ELT_PROD 0
#define FCN_ELT_SUM  1
#define FCN_ELT_MAX  2
/* y = a (op) b over `count` contiguous floats; SUM uses coefficients ca, cb */
int  fcn_eltwise_fwd_f32(const float* a, const float* b, float* y, size_t count, int op,
                         float ca, float cb, fcn_stream_t s);
/* copies C channels of every pixel between strided NHWC buffers (Concat / Slice fallback) */
int  fcn_copy_channels_f32(const float* src, float* dst, int pixels, int C, int src_cstride,
                           int src_coffset, int dst_cstride, int dst_coffset, fcn_stream_t s);
/* grouped bilinear-style Deconvolution, group == channels, one filter [k][k] per channel:
 * Caffe DeconvolutionLayer with `group: C` as in train/fcn_bbox/train_val.prototxt:544-565 */
/* Softmax over the channels of every pixel (Caffe SoftmaxLayer, axis 1) */
int  fcn_softmax_fwd_f32(const float* x, float* y, int pixels, int C, int x_cstride, int y_cstride, fcn_stream_t s);
int  fcn_deconv_depthwise_fwd_f32(const float* x, const float* w, const float* bias, float* y,
                                  int N, int H, int W, int C, int x_cstride, int k, int stride, int pad,
                                  int OH, int OW, int y_cstride, int y_coffset, fcn_stream_t s);

/* ---- inference pre-processing: demean_rgb_image + cv.resize + HWC->CHW
 *      (fcn_object_detector.py:79-82, 407-413) ---- */
/* h/w x 3 uint8 BGR frame -> NHWC float32 (C padded to dst_cstride) in [0,1]:
 * (px - mean[c] - min) / (max - min) over the whole frame, then bilinear resize to (H, W), then + shift
 * (the net's Power(shift) input transform, models/deploy.prototxt:8-16; pass 0 to get the blob itself).
 * d_minmax is a 32-byte device scratch (per-channel uint8 min and max, as int32). */
int  fcn_preprocess_bgr8(const uint8_t* frame, int h, int w, float* dst, int H, int W, int dst_cstride,
                         float shift, float* d_minmax, fcn_stream_t s);

/* ---- half-float activation path (BASELINE configs[4]: batched inference with f16 storage, f32 accumulation).
 *      Convolutions take FCN_CONV_F16 in fcn_conv_desc.flags; these are the layout converters and the other layers
 *      of models/deploy.prototxt in that element type.  Channel counts / strides are multiples of 8 (16 bytes). ---- */
int  fcn_nchw_f32_to_nhwc_f16(const float* src, void* dst, int N, int C, int H, int W, int dst_cstride, int dst_coffset, float shift,
                              fcn_stream_t s);
int  fcn_nhwc_f16_to_nchw_f32(const void* src, float* dst, int N, int C, int H, int W, int src_cstride, int src_coffset, fcn_stream_t s);
int  fcn_maxpool_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad, int OH, int OW,
                         int y_cstride, int y_coffset, fcn_stream_t s);
int  fcn_lrn_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int y_cstride, int local_size, float alpha, float beta,
                     float k, fcn_stream_t s);
/* the half twin of fcn_maxpool_lrn5_fwd_f32 (8-channel groups).  Against fcn_maxpool_fwd_f16 + fcn_lrn_fwd_f16 run one after the other
 * (either order): 3x3 / stride 2 / pad 0 poolings of at most 192 channels take an LDS-patch kernel whose LRN differs from the stand-alone
 * one in the last float32 bit of scale^-beta on a few elements - fewer than 1e-4 of the outputs differ, each by ONE f16 ulp
 * (tests/test_gpu_f16.py asserts exactly that bound); every other geometry is bit-identical to the two launches. */
int  fcn_maxpool_lrn5_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad,
                              int OH, int OW, int y_cstride, int lrn_first, float alpha, float beta, float lrn_k, fcn_stream_t s);
/* The other layers of the VGG16 nets (train/fcn_bbox, train/bounding_box/deploy.prototxt) on half blobs: twins of fcn_avepool_fwd_f32,
 * fcn_deconv_depthwise_fwd_f32, fcn_eltwise_fwd_f32, fcn_softmax_fwd_f32 and fcn_copy_channels_f32.  A lane moves 8 channels (16 bytes),
 * sums in float32 and rounds once (to nearest even) at the store.  Common contract: pointers 16-byte aligned, x_cstride / y_cstride /
 * y_coffset multiples of 8 halves (of 4 floats for a float32 output) else FCN_E_ALIGN; null pointers and non-positive extents FCN_E_ARG;
 * every check precedes the first HIP call.  C is the REAL channel count and need not be a multiple of 8: exactly channels
 * y_coffset .. y_coffset + C - 1 of every output pixel are written, no w / bias element beyond C is read, and the pad channels of x up to
 * the next multiple of 8 may be read but never reach a written value.  Results do not depend on the run (no atomics).
 * out_f32 = 1: y holds float32 (an output blob of an f16 engine, which the decode kernels read). */
/* Caffe divisor (window clipped to H + pad), sum over the part inside the image.  Windows of 64 pixels and more are summed by a whole
 * workgroup per output pixel (pixel lanes stride over the window, partial sums meet in LDS in a fixed tree); smaller ones by one lane. */
int  fcn_avepool_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad, int OH, int OW,
                         int y_cstride, int y_coffset, fcn_stream_t s);
/* x halves; w float32 [C][k][k] and bias float32 [C] (may be NULL), as fcn_deconv_depthwise_fwd_f32 takes them */
int  fcn_deconv_depthwise_fwd_f16(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C, int x_cstride,
                                  int k, int stride, int pad, int OH, int OW, int y_cstride, int y_coffset, int out_f32, fcn_stream_t s);
/* over `count` contiguous halves, count a positive multiple of 8 (whole strided rows, pad channels included); y may be a */
int  fcn_eltwise_fwd_f16(const void* a, const void* b, void* y, size_t count, int op, float ca, float cb, fcn_stream_t s);
/* channels 0 .. C-1 of every pixel; one exp per element while C <= 32 */
int  fcn_softmax_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int y_cstride, int out_f32, fcn_stream_t s);
/* strides multiples of 8 halves; offsets that are both multiples of 8 move 16 bytes per lane, any other offset one half per lane */
int  fcn_copy_channels_f16(const void* src, void* dst, int pixels, int C, int src_cstride, int src_coffset, int dst_cstride,
                           int dst_coffset, fcn_stream_t s);
/* n windows of ONE frame -> the n images of an N x H x W x dst_cstride blob: the node's multi-window path
 * (scripts/fcn_object_detector.py run_detector2 :198-211 with detection_window_roi :257-277) demeans and normalises the WHOLE frame
 * (min / max over the frame), crops stride x stride windows plus a central one, and resizes each to the net's input.  h_rois: n x
 * (x, y, w, h) int32 on the HOST, every window inside the frame, n <= 32; d_minmax: 32 bytes.  Same arithmetic as
 * fcn_preprocess_bgr8 (float64, float resize coefficients). */
int  fcn_preprocess_bgr8_rois(const uint8_t* frame, int h, int w, const int32_t* h_rois, int n, void* dst, int dst_f16, int H, int W,
                              int dst_cstride, float shift, float* d_minmax, fcn_stream_t s);
/* dst_f16 of the two calls below: 0 = float32 blob, 1 = half blob (channels 0..2 of every pixel are written, nothing else), 3 = the
 * half image of an f16 engine - 8-half pixels whose channels 3 and 4 hold the constant 1 and 5..7 zero (FCN_CONV_IMAGE_ONES): the whole
 * pixel (b, g, r, 1, 1, 0, 0, 0) leaves in ONE 16-byte store (dst_cstride must be 8, dst 16-byte aligned). */
/* n equally sized frames (h*w*3 bytes apart) -> the n images of an N x H x W x dst_cstride blob in three launches;
 * each frame is normalised with its own min / max.  d_minmax: 32 bytes per frame. */
int  fcn_preprocess_bgr8_batch(const uint8_t* frames, int n, int h, int w, void* dst, int dst_f16, int H, int W, int dst_cstride,
                               float shift, float* d_minmax, fcn_stream_t s);
int  fcn_preprocess_bgr8_f16(const uint8_t* frame, int h, int w, void* dst, int H, int W, int dst_cstride, float shift, float* d_minmax,
                             fcn_stream_t s);

/* ---- training-scene synthesis on the device: the pixel work of ArgumentationEngineMapping.argument
 *      (scripts/data_argumentation_layer/argumentation_engine.py:651-746) and the whole-image flip of
 *      random_argumentation (:143-188).  The random decisions stay on the host; images live in HBM. ---- */
typedef struct fcn_scene_obj {
    const uint8_t* img;    /* src_h x src_w x 3 BGR, as stored (unflipped)                                   */
    const uint8_t* mask;   /* src_h x src_w, nonzero = object                                                */
    int32_t src_h, src_w;
    int32_t flip;          /* cv.flip code applied to the object before cropping: 0, 1, -1; anything else: none */
    int32_t roi_x, roi_y, roi_w, roi_h;   /* crop in the flipped image                                          */
    int32_t out_w, out_h;  /* size after the optional bilinear rescale                                        */
    int32_t cx, cy;        /* paste position in the scene (may be negative / hang over the border)            */
    int32_t label1;        /* value written to the class mask (label + 1)                                     */
} fcn_scene_obj;
/* out_img (H x W x 3) = bilinear resize of the background crop, then the objects pasted in order where their (resized)
 * mask is nonzero, then the whole-image flip `final_flip` (0, 1, -1; else none); out_mask (H x W, may be NULL) = label1
 * of the last object covering the pixel, 0 elsewhere.  d_objs: nobj records in device memory. */
int  fcn_compose_scene_bgr8(const uint8_t* bg, int bg_h, int bg_w, int crop_x, int crop_y, int crop_w, int crop_h,
                            const fcn_scene_obj* d_objs, int nobj, int final_flip, uint8_t* out_img, uint8_t* out_mask,
                            int H, int W, fcn_stream_t s);
/* The same scene seen through the window (view_x, view_y, view_w, view_h) of the flipped H x W scene: out_img is
 * view_h x view_w x 3, out_mask view_h x view_w; either may be NULL.  This is the "zoom in" crop of random_argumentation
 * (argumentation_engine.py:156-172, crop_image_dimension :190-236), which crops the image but not the class mask. */
int  fcn_compose_scene_view_bgr8(const uint8_t* bg, int bg_h, int bg_w, int crop_x, int crop_y, int crop_w, int crop_h,
                                 const fcn_scene_obj* d_objs, int nobj, int final_flip, uint8_t* out_img, uint8_t* out_mask,
                                 int H, int W, int view_x, int view_y, int view_w, int view_h, fcn_stream_t s);

/* ---- colour augmentation of a composed scene: color_space_argumentation (argumentation_engine.py:308-322), an
 *      imgaug Sequential restated from the operators' documented definitions (imgaug itself is an un-vendored submodule).
 *      All images are h x w x 3 uint8, every stage rounds half-to-even and saturates to uint8 like the library's
 *      uint8 pipeline.  src and dst must not alias. ---- */
#define FCN_GAUSS_MAX_RADIUS 15
/* GaussianBlur: separable, half-kernel taps[0..radius] (centre first, float32, normalised by the caller), reflect-101
 * border; tmp: h*w*3 floats of scratch */
int  fcn_blur_gauss_bgr8(const uint8_t* src, uint8_t* dst, float* tmp, int h, int w, const float* h_taps, int radius, fcn_stream_t s);
/* AverageBlur (cv2.blur): k x k box, anchor k/2, reflect-101 border, round(sum * (1.0 / k^2)) in double; 1 <= k <= 15 */
int  fcn_blur_box_bgr8(const uint8_t* src, uint8_t* dst, int h, int w, int k, fcn_stream_t s);
/* MedianBlur (cv2.medianBlur): per-channel median of the k x k window, replicated border; k in {3, 5, 7} */
int  fcn_blur_median_bgr8(const uint8_t* src, uint8_t* dst, int h, int w, int k, fcn_stream_t s);
typedef struct fcn_color_params {
    float sharpen_centre;  /* (1 - a) + a * (8 + lightness): centre of the 3x3 Sharpen matrix            */
    float sharpen_off;     /* -a: its eight other entries (reflect-101 border)                           */
    int32_t add[3];        /* Add: per-channel integer offsets                                           */
    float mul[3];          /* Multiply: per-channel factors                                              */
    float gray_alpha;      /* Grayscale: out = gray_keep * v + gray_alpha * grey                         */
    float gray_keep;       /* 1 - gray_alpha, rounded to float32 by the caller                           */
} fcn_color_params;
/* Sharpen -> Add -> Multiply -> Grayscale in one pass.  grey = (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14: OpenCV's
 * RGB2GRAY fixed point applied to the channels in storage order, as imgaug does to the reference's BGR image. */
int  fcn_color_augment_bgr8(const uint8_t* src, uint8_t* dst, int h, int w, const fcn_color_params* h_params, fcn_stream_t s);

/* class mask (h x w uint8) -> H x W label blob, one float per pixel at stride dst_cstride (nearest neighbour: top[1] of
 * the data layer in HEAD's mask mode, data_argumentation_layer.py:113-121) */
int  fcn_mask_to_label_f32(const uint8_t* mask, int h, int w, float* dst, int H, int W, int dst_cstride, fcn_stream_t s);

/* ---- DetectNet post-processing: gridbox_to_boxes + vote_boxes -> cv.groupRectangles
 *      (fcn_object_detector.py:337-394; OpenCV 3 objdetect groupRectangles/partition) ---- */
#define FCN_RECT_ROUND_NEAREST_EVEN 0  /* OpenCV vector<Rect> converter: saturate_cast<int>(double) = cvRound */
#define FCN_RECT_ROUND_TRUNCATE     1  /* C (int) cast                                                          */
typedef struct fcn_detect_params {
    int32_t num_classes;     /* C : coverage channels decoded                                  */
    int32_t gy, gx;          /* grid                                                            */
    int32_t cell_w, cell_h;  /* im_sz / grid (integer division, fcn_object_detector.py:368-369) */
    int32_t cvg_cstride, cvg_coffset;   /* NHWC coverage map: cvg[(y*gx+x)*cvg_cstride + cvg_coffset + c] */
    int32_t box_cstride, box_coffset;   /* NHWC bbox map, channels 4c..4c+3 of class c                     */
    float   prob_thresh;     /* ~detection_threshold (0.5)   */
    int32_t group_thresh;    /* ~min_boxes (3)               */
    double  eps;             /* ~nms_eps (0.2); OpenCV takes it as a double */
    int32_t min_height;      /* 20: keep if rect[3]-rect[1] >= min_height (fcn_object_detector.py:346) */
    int32_t round_mode;      /* FCN_RECT_ROUND_*             */
    int32_t max_out;         /* capacity of the output arrays per (image, class) slot */
} fcn_detect_params;
/* One to eight workgroups per (image, class) - the SimilarRects tests of a problem with many candidates are dealt to
 * several workgroups whose forests the last one to arrive merges (small batches only: a full batch fills the chip with one
 * per problem); slot = image * num_classes + class.  Zero-fill the workspace once after allocating it (the arrival words
 * carry a launch tag and are never reset; an uninitialised word matches a live tag with probability 2^-24) and do not
 * share it between launches that may run concurrently.  Outputs per slot:
 * out_rects[slot][max_out][4] int32 (x, y, w, h exactly as groupRectangles returns them, in its
 * cluster order), out_weights[slot][max_out] int32 (cluster size n; the reference's confidence is
 * log(n)), out_count[slot] int32 (may exceed max_out: then only max_out entries were stored).
 * Concatenating the slots of one image in class order reproduces the reference's nested loops
 * (fcn_object_detector.py:104-118).  Any grid; at most 5120 CANDIDATES (cells at or above prob_thresh) per (image, class) -
 * enough for every cell of a 640 x 480 frame at stride 8 - beyond which that slot's out_count is -1 and nothing else of the
 * slot is written.  d_workspace:
 * fcn_detect_workspace_bytes() bytes; image strides are in floats. */
size_t fcn_detect_workspace_bytes(const fcn_detect_params* h_p, int batch);
int  fcn_detect_decode_group(const float* cvg, const float* bbox, int batch,
                             size_t cvg_image_stride, size_t box_image_stride,
                             const fcn_detect_params* h_p, void* d_workspace,
                             int32_t* out_rects, int32_t* out_weights,
                             int32_t* out_count, fcn_stream_t s);

/* ---- run_detector2 after net.forward(): the node's score maps -> the frame-sized probability map and one box per (window, class)
 *      (scripts/fcn_object_detector.py:208-236 with create_mask_labels :279-303; OpenCV's cv.resize / findContours / contourArea /
 *      boundingRect restated in oracle/mask_ref.py).  score: NHWC float32 blob of N windows (the node's net.blobs['score']), classes at
 *      channels coffset .. coffset + C - 1 of cstride; class 0 is the background and is skipped, as in the reference.  h_rects: HOST
 *      array N x (x, y, w, h), the windows' places in the frame - all of one size (detection_window_roi :257-277), N <= 32.
 *      For every window n and class c = 1 .. C-1: values below prob_thresh become 0, x 255, bilinear resize to (w, h), truncating
 *      uint8 cast; the map is OR-ed into pmap (frame_h x frame_w bytes on the device, 4-byte aligned, zeroed by the caller) at the
 *      window's place, and out[(n * (C - 1) + c - 1) * 5 ..] = found, x, y, w, h: the bounding rectangle, in WINDOW coordinates, of the
 *      contour with the largest area (found = 0: no contour of positive area; the reference's 10-pixel padding and the window's origin
 *      are added by the caller).  d_workspace: fcn_score_masks_workspace_bytes() bytes, uninitialised.  pmap must be ALLOCATED up to a
 *      multiple of 4 bytes: the OR is a 32-bit atomic on aligned words, and the up to three bytes behind frame_h * frame_w are read and
 *      written back unchanged. ---- */
size_t fcn_score_masks_workspace_bytes(int n_windows, int num_classes, int w, int h);
int  fcn_score_masks(const float* score, int N, int C, int H, int W, int cstride, int coffset, const int32_t* h_rects, float prob_thresh,
                     uint8_t* pmap, int frame_h, int frame_w, void* d_workspace, int32_t* out, fcn_stream_t s);

/* ---- DetectNet target generation: ArgumentationEngine.bounding_box_parameterized_labels
 *      (argumentation_engine.py:69-109, 26-55, 272-292) ---- */
/* rects: [total][4] int32 (x, y, w, h); labels: [total] int32; rect_offsets: [batch+1] int32 prefix.
 * Outputs are NCHW float32 exactly as the Python layer's tops (data_argumentation_layer.py:67-72):
 * foreground (batch, C, gy, gx); bbox/size/obj/cvg_block (batch, 4C, gy, gx). */
int  fcn_gen_targets(const int32_t* rects, const int32_t* labels, const int32_t* rect_offsets, int batch,
                     int num_classes, int gy, int gx, int stride, double iou_thresh,
                     float* foreground, float* bbox, float* size, float* obj, float* cvg_block,
                     fcn_stream_t s);
/* same arithmetic, written straight into the engine's NHWC blob buffers (element (img, cell, channel) at
 * [(img*gy*gx + cell) * cstride + channel]) so a training step needs no host round trip for its labels */
int  fcn_gen_targets_nhwc(const int32_t* rects, const int32_t* labels, const int32_t* rect_offsets, int batch,
                          int num_classes, int gy, int gx, int stride, double iou_thresh,
                          float* foreground, int fg_cstride, float* bbox, float* size, float* obj, float* cvg_block,
                          int blk_cstride, fcn_stream_t s);

/* ---- training: Net::Backward + losses + solver update as run by `caffe train` (train/train.sh:25-28) over the
 *      loss tail models/train_val.prototxt:53-72,2237-2281 with the settings of train/<net>/solver.prototxt ---- */
/* Weight / bias gradient of a Convolution layer.  `d` describes the FORWARD problem; d->y / y_cstride / y_coffset name the
 * gradient of the layer's output (d->w, d->bias, d->y2 are ignored).  dw is [Cout][kh][kw][Cin] like the forward weights,
 * db is [Cout] or NULL.  Bit-reproducible (pixel splits are summed in a fixed order).  Workspace size in floats: */
size_t fcn_conv2d_wgrad_workspace_floats(const fcn_conv_desc* h_d, int* h_splits);
int  fcn_conv2d_wgrad_f32(const fcn_conv_desc* h_d, float* dw, float* db, float* d_workspace, fcn_stream_t s);
/* Up to 4 layers in ONE launch (+ one grouped fixed-order reduction): the output convolutions of an inception module become
 * ready together and most of them are too small to fill the chip alone.  dbs[i] may be NULL. */
size_t fcn_conv2d_wgrad_group_workspace_floats(const fcn_conv_desc* h_ds, int n);
int  fcn_conv2d_wgrad_group_f32(const fcn_conv_desc* h_ds, float* const* h_dws, float* const* h_dbs, int n, float* d_workspace,
                                fcn_stream_t s);
/* The same four calls with the launch configuration named by the caller (the training engine times every configuration once per
 * launch at plan time and keeps the fastest, as the forward engine does): cfg_request -1 = the built-in heuristic (what the calls
 * above use), 0 .. fcn_conv2d_wgrad_num_configs() - 1 = that configuration.  The last one, fcn_conv2d_wgrad_split_config(), is
 * the role-split kernel (eight waves with fixed staging / multiplying roles, a region shape per problem); the others are tile
 * shapes of the 64-wide family.  The workspace of a launch depends on its configuration: size it with the SAME cfg_request (or
 * with the maximum over the ones that may be used).  Every configuration is bit-reproducible; two configurations differ in the
 * last bits (their pixel split counts differ). */
int  fcn_conv2d_wgrad_num_configs(void);
int  fcn_conv2d_wgrad_split_config(void);
size_t fcn_conv2d_wgrad_workspace_floats_cfg(const fcn_conv_desc* h_d, int cfg_request, int* h_splits);
int  fcn_conv2d_wgrad_cfg_f32(const fcn_conv_desc* h_d, float* dw, float* db, float* d_workspace, int cfg_request, fcn_stream_t s);
size_t fcn_conv2d_wgrad_group_workspace_floats_cfg(const fcn_conv_desc* h_ds, int n, int cfg_request);
int  fcn_conv2d_wgrad_group_cfg_f32(const fcn_conv_desc* h_ds, float* const* h_dws, float* const* h_dbs, int n, float* d_workspace,
                                    int cfg_request, fcn_stream_t s);
/* Filter bank of the data-gradient pass: wt[c][kh-1-r][kw-1-q][k] = w[k][r][q][c] (w: [Cout][kh][kw][Cin4],
 * wt: [Cin][kh][kw][Cout4], zero padded).  dX = fcn_conv2d_fwd_f32(dY, wt) with pad' = k-1-pad for stride-1 layers. */
int  fcn_conv_weights_flip_f32(const float* w, float* wt, int Cout, int kh, int kw, int Cin, int Cin4, int Cout4, fcn_stream_t s);
/* All filter banks of a net in ONE launch: segment i flips w_base + w_offset (floats) into wt_base + wt_offset. */
typedef struct fcn_flip_seg { uint64_t w_offset, wt_offset; int32_t Cout, kh, kw, Cin, Cin4, Cout4; } fcn_flip_seg;
int  fcn_conv_weights_flip_batch_f32(const float* w_base, float* wt_base, const fcn_flip_seg* d_segs, int nseg, fcn_stream_t s);
int  fcn_relu_bwd_f32(const float* dy, const float* y, float* dx, int pixels, int C, int cstride, fcn_stream_t s);
/* Backward of a ReLU layer of its own: dx (+)= y > 0 ? dy : negative_slope * dy over the C real channels of pixels of cstride floats
 * (pad channels are left alone).  negative_slope >= 0 only: then the sign of the output y is the sign of the input.  dx == dy (in
 * place) is allowed without accumulate. */
int  fcn_relu_bwd_slope_f32(const float* dy, const float* y, float* dx, int pixels, int C, int cstride, float negative_slope, int accumulate,
                            fcn_stream_t s);
int  fcn_sigmoid_bwd_f32(const float* y, const float* dy, float* dx, size_t count, int accumulate, fcn_stream_t s);
int  fcn_maxpool_bwd_f32(const float* dy, const int32_t* idx, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset,
                         int k, int stride, int pad, int OH, int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);
/* The same with the ReLU backward of the blob dx belongs to folded in (relu_y = that blob's activation, may be NULL): used when
 * the pooling backward is the LAST pass that writes the gradient (FCN_CONV_MASK is the convolution's counterpart). */
int  fcn_maxpool_bwd_mask_f32(const float* dy, const int32_t* idx, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset,
                              int k, int stride, int pad, int OH, int OW, int dy_cstride, int dy_coffset, int accumulate,
                              const float* relu_y, int relu_y_cstride, int relu_y_coffset, fcn_stream_t s);
/* AVE pool backward (Caffe PoolingLayer, pool: AVE), the argument list of fcn_maxpool_bwd_f32 without idx:
 * dX[n][iy][ix][c] (+)= sum over the windows (oy, ox) that contain (iy, ix), in ascending (oy, ox) order, of dY[n][oy][ox][c] / divisor(oy, ox),
 * divisor = the window clipped to the padded extent, what fcn_avepool_fwd_f32 divides by.  A gather with one writer per element and no
 * atomics: the same call gives the same bits.  Pixels under no window (stride > k) get zero, or stay as they are with accumulate; only
 * channels dx_coffset .. dx_coffset + C - 1 are written (C need not be a multiple of 4).
 * Contract: null pointers, non-positive extents, negative pad, a last window that starts outside the image, a negative offset or a
 * slice wider than its stride FCN_E_ARG; dx_cstride, dx_coffset, dy_cstride or dy_coffset not a multiple of 4 floats, dy or dx off
 * 16 bytes FCN_E_ALIGN; a view past 2^31 elements FCN_E_UNSUPPORTED.  Every check precedes the first HIP call. */
int  fcn_avepool_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset,
                         int k, int stride, int pad, int OH, int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);
int  fcn_lrn_bwd_f32(const float* x, const float* y, const float* scale, const float* dy, float* dx, int pixels, int C,
                     int x_cstride, int y_cstride, int local_size, float alpha, float beta, int accumulate, fcn_stream_t s);
/* Dropout (TRAIN): y = x * mask / (1 - ratio); mask of element (n,c,h,w) = hash(NCHW index, seed) >= ratio * 2^32.
 * The same call with the same seed applied to the gradient is the backward pass. */
int  fcn_dropout_f32(const float* x, float* y, int N, int C, int H, int W, int x_cstride, int x_coffset, int y_cstride,
                     int y_coffset, float ratio, unsigned seed, unsigned index_offset, fcn_stream_t s);
/* index_offset is added to the NCHW index: rank r of a data-parallel job passes r*N*C*H*W so that the masks of the
 * shards together equal the mask of the undivided batch */
/* kind 0 = L1Loss (NVIDIA Caffe): loss = sum|a-b|/num, da = sign(a-b) * weight/num;
 * kind 1 = EuclideanLoss: loss = sum(a-b)^2/(2 num), da = (a-b) * weight/num.  da may be NULL; d_loss is one device float. */
int  fcn_loss_f32(int kind, const float* a, const float* b, float* da, float* d_loss, int pixels, int C, int cstride, int num,
                  float weight, fcn_stream_t s);
/* SoftmaxWithLoss (train/fcn_bbox/train_val.prototxt:838-847): x NHWC scores, label one float per pixel (class id);
 * loss = -sum log p[label] / (valid pixels if normalize else N); dx (may be NULL) = (p - onehot) * weight / denom.
 * d_workspace: fcn_softmax_loss_workspace_bytes() bytes, 8-byte aligned.  The reduction order is fixed. */
size_t fcn_softmax_loss_workspace_bytes(void);
int  fcn_softmax_loss_f32(const float* x, const float* label, float* dx, float* d_loss, int N, int pixels, int C, int x_cstride,
                          int label_cstride, int normalize, int has_ignore, int ignore_label, float weight, void* d_workspace,
                          fcn_stream_t s);
/* Gradient w.r.t. the input of the depthwise deconvolution (fcn_deconv_depthwise_fwd_f32): H, W are the INPUT extents */
int  fcn_deconv_depthwise_bwd_f32(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int dx_cstride, int k,
                                  int stride, int pad, int OH, int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);
/* Solver update over one flat parameter buffer cut into segments (one per learnable blob). */
typedef struct fcn_solver_seg { uint64_t offset, count; float lr_mult, decay_mult; } fcn_solver_seg;
/* SGD: g' = g*grad_scale + wd*decay_mult*w ; hist = momentum*hist + rate*lr_mult*g' ; w -= hist */
int  fcn_sgd_update_f32(float* w, const float* g, float* hist, const fcn_solver_seg* d_segs, int nseg, float rate, float momentum,
                        float weight_decay, float grad_scale, fcn_stream_t s);
/* Adam (Caffe AdamSolver): m,v moments, w -= rate*lr_mult*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+delta) */
int  fcn_adam_update_f32(float* w, const float* g, float* m, float* v, const fcn_solver_seg* d_segs, int nseg, float rate,
                         float beta1, float beta2, float delta, float weight_decay, int t, float grad_scale, fcn_stream_t s);
/* Every solver type of Caffe's SolverParameter in one entry point (public BVLC Caffe sgd_solvers, restated).  Per element of a segment,
 * with clip = *d_clip (1.0 when d_clip is NULL), lr = rate*lr_mult and
 *   g' = g*grad_scale*clip + weight_decay*decay_mult * (w for FCN_REG_L2, sign(w) for FCN_REG_L1):
 *   SGD       h1 = momentum*h1 + lr*g' ;  w -= h1
 *   NESTEROV  h_old = h1 ; h1 = momentum*h1 + lr*g' ;  w -= (1+momentum)*h1 - momentum*h_old
 *   ADAGRAD   h1 += g'^2 ;  w -= lr*g' / (sqrt(h1) + delta)
 *   RMSPROP   h1 = rms_decay*h1 + (1-rms_decay)*g'^2 ;  w -= lr*g' / (sqrt(h1) + delta)
 *   ADADELTA  h1 = momentum*h1 + (1-momentum)*g'^2 ; u = g'*sqrt((h2+delta)/(h1+delta)) ; h2 = momentum*h2 + (1-momentum)*u^2 ;  w -= lr*u
 *   ADAM      as fcn_adam_update_f32 with beta1 = momentum, beta2 = momentum2, step t
 * h2 is read for ADADELTA and ADAM only (NULL otherwise).  Segments with lr_mult == 0 and the elements outside every segment are
 * neither read into a result nor written.  With FCN_REG_L2 and d_clip == NULL, SGD and ADAM give the bits of fcn_sgd_update_f32 /
 * fcn_adam_update_f32.  FCN_E_ARG: null pointer, nseg outside 1 .. 65535, unknown kind / regularization, momentum or rms_decay
 * outside [0, 1) (ADAM: momentum2 too, t < 1); FCN_E_ALIGN: w, g, h1, h2 or d_segs not 16-byte aligned.  Checked before any HIP call. */
#define FCN_SOLVER_SGD      0
#define FCN_SOLVER_NESTEROV 1
#define FCN_SOLVER_ADAGRAD  2
#define FCN_SOLVER_RMSPROP  3
#define FCN_SOLVER_ADADELTA 4
#define FCN_SOLVER_ADAM     5
#define FCN_REG_L2 0
#define FCN_REG_L1 1
int  fcn_solver_update_f32(int kind, float* w, const float* g, float* h1, float* h2, const fcn_solver_seg* d_segs, int nseg, float rate,
                           float momentum, float momentum2, float rms_decay, float delta, float weight_decay, int regularization, int t,
                           float grad_scale, const float* d_clip, fcn_stream_t s);
/* Gradient clipping (Caffe's clip_gradients) without a host read-back: *d_clip = min(1, clip_gradients / (norm_scale * sqrt(sumsq))),
 * sumsq = the sum of g^2 over every segment (also written to *d_sumsq unless NULL); exactly 1.0 when the norm does not exceed the
 * threshold.  norm_scale: what the buffer is a multiple of (1 / ranks after a summing all-reduce).  The sum is a fixed-order
 * two-stage tree in float64 (per-workgroup partials in d_workspace, fcn_grad_clip_workspace_bytes() bytes, 16-byte aligned, then
 * one workgroup in index order; no atomics): the same inputs give the same bits on every run.  Elements outside the segments are not read. */
size_t fcn_grad_clip_workspace_bytes(void);
int  fcn_grad_clip_f32(const float* g, const fcn_solver_seg* d_segs, int nseg, float clip_gradients, float norm_scale, float* d_clip,
                       float* d_sumsq, void* d_workspace, fcn_stream_t s);
/* Gradient accumulation of iter_size > 1: acc = first ? g : acc + g over count floats (both 16-byte aligned), one launch */
int  fcn_grad_accumulate_f32(float* acc, const float* g, size_t count, int first, fcn_stream_t s);

/* ---- validation pass (Solver::Test, `caffe test`) ---- */
/* Running sum of an output blob over the forwards of a test pass: acc[n][c][p] += x[n][p][x_coffset + c].  x: base of an NHWC
 * buffer with channel stride x_cstride (N images of `pixels` = H*W pixels; x_coffset selects the view's first channel); acc:
 * N*C*pixels floats in NCHW order, what Caffe's test_score[] holds.  Float32, exactly one add per element per call, so after k
 * calls the bits equal a host float32 running sum in call order.  N = pixels = C = 1 is a loss scalar.  16-byte loads when x is
 * 16-byte aligned and x_cstride, x_coffset are multiples of 4; channels outside [x_coffset, x_coffset + C) are neither read nor
 * written.  Zero acc with fcn_memset_async at the start of a pass. */
int  fcn_score_accumulate_f32(float* acc, const float* x, int N, int pixels, int C, int x_cstride, int x_coffset, fcn_stream_t s);
/* Accuracy (BVLC Caffe master's AccuracyLayer over the channel axis), arguments as fcn_softmax_loss_f32: x NHWC scores (view base,
 * `pixels` = N*H*W), label one float per pixel.  A pixel whose label equals ignore_label (has_ignore != 0) is skipped; a labelled
 * pixel is correct iff fewer than top_k channels j != label have x[j] >= x[label] (ties count against the label); a label outside
 * [0, C) counts as valid and wrong and never indexes x.  *d_acc = valid ? correct / valid : 0; d_per_class (may be NULL, C floats,
 * C <= 128) [c] = n_c ? correct_c / n_c : 0.  Integer counts: per-workgroup partials in d_workspace (fcn_accuracy_workspace_bytes()
 * bytes, 4-byte aligned), then one workgroup in index order; no atomics on floats, the same bits on every run.  16-byte loads
 * when x is 16-byte aligned and x_cstride is a multiple of 4; channels >= C are never read. */
size_t fcn_accuracy_workspace_bytes(void);
int  fcn_accuracy_f32(const float* x, const float* label, float* d_acc, float* d_per_class, int N, int pixels, int C, int x_cstride,
                      int label_cstride, int top_k, int has_ignore, int ignore_label, void* d_workspace, fcn_stream_t s);

/* ---- transposed (fractionally-strided) convolution: Caffe DeconvolutionLayer::Forward_gpu with group 1, and the bottom diff of
 *      a strided ConvolutionLayer::Backward_gpu.  NHWC float32, exact f32 on the matrix cores (v_mfma_f32_32x32x2_f32).
 *        b[n, oy, ox, cb] = bias[cb] + sum over ca, r, q, iy, ix with oy + pad - r == stride*iy, ox + pad - q == stride*ix,
 *                                      0 <= iy < H, 0 <= ix < W  of  w[ca][cb][r][q] * a[n, iy, ix, ca]
 *      OH / OW are explicit: any value in [stride*(H-1) + kh - 2 pad, that + stride - 1] (the data gradient of a convolution whose
 *      last rows / columns lay under no window: those outputs get bias / zero).  The outputs are evaluated phase by phase
 *      ((oy + pad) mod stride, (ox + pad) mod stride): each phase is a stride-1 correlation with its own sub-filter, no structural
 *      zero is multiplied, and all phases of all problems of a plan run in ONE launch.  Every output element is written by exactly
 *      one lane and the contraction is never split: the same bits on every run.
 *      flags: FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK with the meaning (and order: accumulate, ReLU, mask) they have in
 *      fcn_conv_desc; y2 is only read (FCN_CONV_MASK).  Channels Ca .. round4(Ca)-1 of `a` are padding and are never multiplied
 *      (they may hold anything); channels of b outside [b_coffset, b_coffset + Cb) are not touched.  16-byte stores when
 *      b (y2) is 16-byte aligned with strides / offsets in multiples of 4, scalar stores otherwise and for a last partial group.
 *      Refused on the host before any launch: FCN_E_ARG (null pointer, non-positive extent, OH / OW outside the range above,
 *      slice wider than its stride, FCN_CONV_MASK without y2), FCN_E_ALIGN (a_cstride not a multiple of 4 or below round4(Ca);
 *      a / w not 16-byte aligned), FCN_E_UNSUPPORTED (stride > 64, pad >= kh or kw, other flags, tensors past 2^31 elements). ---- */
typedef struct fcn_tconv_desc {
    const float* a;      /* NHWC input, channel stride a_cstride (a multiple of 4, >= round4(Ca))               */
    const float* w;      /* bank packed by fcn_tconv_bank_pack_f32: [kh][kw][Cb][round4(Ca)]                     */
    const float* bias;   /* [Cb] or NULL                                                                         */
    float*       b;      /* NHWC output; channel cb of pixel m at b[m*b_cstride + b_coffset + cb]                */
    float*       y2;     /* FCN_CONV_MASK: the activation whose sign masks the result (same indexing via y2_*)   */
    int32_t N, H, W, Ca, a_cstride;
    int32_t Cb, kh, kw, pad, stride, OH, OW;
    int32_t b_cstride, b_coffset, y2_cstride, y2_coffset;
    int32_t flags;
} fcn_tconv_desc;
typedef struct fcn_tconv_plan {
    void*   d_probs;
    int32_t n;
    int32_t cfg;          /* tile configuration chosen by prepare() */
    int32_t grid_x, grid_y;
    int32_t total_tiles;
} fcn_tconv_plan;
/* number of tile configurations (cfg_request: -1 = built-in choice, 0 .. count-1); one today: 64 pixels x 64 channels x 16 k */
int    fcn_tconv2d_num_configs(void);
size_t fcn_tconv2d_workspace_bytes(const fcn_tconv_desc* h_descs, int n);
/* validates and uploads n problems into d_workspace with a synchronous copy (plan time, not inside a graph capture); the
 * workspace must stay alive as long as the plan is used */
int    fcn_tconv2d_prepare(const fcn_tconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_tconv_plan* h_out);
/* one pure kernel launch for all problems and phases of the plan: capturable */
int    fcn_tconv2d_f32(const fcn_tconv_plan* h_plan, fcn_stream_t s);
/* packed[(r*kw + q)*Cb + cb][ca] = w[ca][r][q][cb], zero for Ca <= ca < round4(Ca).  w is [Ca][kh][kw][w_cstride] (cb contiguous):
 * the OHWI bank of a Convolution read for its data gradient (Ca = Cout, Cb = Cin, w_cstride = round4(Cin)), and the device layout of a
 * group-1 Deconvolution blob (Ca = Cin, Cb = Cout, w_cstride = round4(Cout)).  fcn_tconv_bank_floats(): floats of `packed`. */
size_t fcn_tconv_bank_floats(int Ca, int Cb, int kh, int kw);
int    fcn_tconv_bank_pack_f32(const float* w, float* packed, int Ca, int Cb, int w_cstride, int kh, int kw, fcn_stream_t s);
/* The transposed convolution in half floats (inference; the data gradient of a strided convolution stays float32), the contract above
 * with these differences.  The SAME descriptor: its a, w and b point to IEEE halves (declared float* - pass the addresses), b to
 * float32 under FCN_CONV_OUT_F32; bias is float32 or NULL.  a: NHWC halves, a_cstride a multiple of 8 and >= round8(Ca), 16-byte
 * aligned; channels Ca .. round8(Ca)-1 of a pixel are padding and are never multiplied, whatever they hold.  w: the bank packed by
 * fcn_tconv_bank_pack_f16, [kh][kw][Cb][round8(Ca)] halves, 16-byte aligned.  Sums are float32 on the matrix cores
 * (v_mfma_f32_32x32x16_f16); a half result is rounded to nearest even once from the float32 sum (after bias and ReLU).  flags:
 * FCN_CONV_RELU | FCN_CONV_OUT_F32; every other flag (FCN_CONV_ACCUM, FCN_CONV_MASK) and a non-NULL y2 are FCN_E_UNSUPPORTED.  b needs
 * 2-byte alignment (4-byte under FCN_CONV_OUT_F32) and any b_cstride >= b_coffset + Cb.  Halves go out in 16-byte stores (eight
 * channels) when b is 16-byte aligned and b_cstride / b_coffset are multiples of 8, in 8-byte stores (four channels) when b is 8-byte
 * aligned with multiples of 4, else in 2-byte stores; float32 results as in the float32 kernel.  A last partial run goes out in scalar
 * stores: a half that shares a 32-bit word with the slice's first or last half is not touched.  One launch for all phases and problems
 * of a plan, every output element written by exactly one lane, no atomics: the same bits on every run.
 * Two tile configurations: 0 = 64 lattice pixels x 64 channels, 1 = 128 lattice pixels x 32 channels; one holds for the whole plan.
 * cfg_request -1 takes 1 when no problem of the plan has more than 32 output channels (a score layer has 21) and 0 otherwise.
 * A plan records its element type in `cfg`: fcn_tconv2d_prepare numbers its configurations from 0, fcn_tconv2d_prepare_f16 from
 * FCN_TCONV_CFG_F16, and each launch refuses the other's plan with FCN_E_ARG.  The workspace is that of fcn_tconv2d_workspace_bytes. */
#define FCN_TCONV_CFG_F16 256
int    fcn_tconv2d_num_configs_f16(void);
int    fcn_tconv2d_prepare_f16(const fcn_tconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_tconv_plan* h_out);
/* one pure kernel launch for all problems and phases of the plan: capturable */
int    fcn_tconv2d_f16(const fcn_tconv_plan* h_plan, fcn_stream_t s);
/* the bank in halves: packed[(r*kw + q)*Cb + cb][ca] = w[ca][r][q][cb], zero for Ca <= ca < round8(Ca).  w is [Ca][kh][kw][w_cstride]
 * halves (cb contiguous): the device layout of a group-1 Deconvolution blob over a half bottom (w_cstride = round8(Cout)); 2-byte
 * aligned, packed 16-byte aligned.  fcn_tconv_bank_halves(): halves of `packed`. */
size_t fcn_tconv_bank_halves(int Ca, int Cb, int kh, int kw);
int    fcn_tconv_bank_pack_f16(const void* w, void* packed, int Ca, int Cb, int w_cstride, int kh, int kw, fcn_stream_t s);
/* db[c] = sum over pixels of dy[pixel*cstride + coffset + c], c < C: the bias gradient of a Deconvolution (the weight-gradient kernel
 * sums ITS y, which after the role swap is the layer's input).  One workgroup per channel, fixed order: bit-reproducible. */
int    fcn_channel_sum_f32(const float* dy, float* db, int pixels, int C, int cstride, int coffset, fcn_stream_t s);

/* ---- per-axis ("rectangular") and dilated ("atrous") convolution: Caffe ConvolutionLayer whose two spatial axes differ in kernel
 *      extent, pad or stride (kernel_h / kernel_w, pad_h / pad_w, stride_h / stride_w: the 1x7 / 7x1 and 1x3 / 3x1 pairs of
 *      Inception-v3 / v4, the k x 1 + 1 x k pairs of ENet / ERFNet), and Caffe ConvolutionLayer with convolution_param { dilation: d }
 *      (DeepLab-LargeFOV conv5_* / fc6, the DeepLab-v2 ASPP branches): a square dilated layer is the case with equal axes (kh = kw,
 *      pad_h = pad_w, stride_h = stride_w).  Forward, data gradient and weight gradient, with one dilation for both axes.  NHWC
 *      float32, exact f32 on the matrix cores (v_mfma_f32_32x32x2_f32).  With zeros outside the image:
 *        y[n, oy, ox, co] = bias[co] + sum over ci, r, q of w[co][r][q][ci] * x[n, oy*stride_h - pad_h + r*dil, ox*stride_w - pad_w + q*dil, ci]
 *        OH = (H + 2 pad_h - (dil*(kh-1) + 1)) / stride_h + 1     (floor)        OW likewise with kw, pad_w, stride_w
 *      The bank is the Convolution's parameter blob as the engine keeps it, [Cout][kh][kw][round4(Cin)] with Cin contiguous: no
 *      repacking.  All problems of a plan run in ONE launch (the four ASPP branches read one blob with four dilations).  Every output
 *      element is written by exactly one lane, the contraction is never split across lanes that meet in memory, there are no float
 *      atomics: the same bits on every run.
 *      flags: FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK with the meaning (and order: accumulate, ReLU, mask) they have in
 *      fcn_tconv_desc; y2 is only read (FCN_CONV_MASK).  Channels Cin .. round4(Cin)-1 of `x` are padding and are never multiplied
 *      (they may hold anything: the rule of fcn_tconv_desc, not of the dense kernels); channels of y outside [y_coffset, y_coffset + Cout)
 *      are not touched.  16-byte stores when y (y2) is 16-byte aligned with strides / offsets in multiples of 4, scalar stores otherwise
 *      and for a last partial group.  dilation >= 1; a square problem (equal extents, pads and strides) with dilation == 1 is legal
 *      and equals the dense convolution.
 *      The data gradient of a layer with stride_h == stride_w == 1 is the same kernel on dY with the flipped bank of
 *      fcn_conv_weights_flip_batch_f32 (which takes kh and kw separately), pad_h' = dil*(kh-1) - pad_h, pad_w' = dil*(kw-1) - pad_w, the
 *      same dilation, and FCN_CONV_ACCUM / FCN_CONV_MASK as the dense data-gradient passes use them.
 *      Refused on the host before the first HIP call: FCN_E_ARG (null x / w / y, null descriptors / plan / workspace, n <= 0, unknown
 *      cfg_request, non-positive extent or stride, negative pad, window larger than the padded image, OH / OW not the value above,
 *      slice wider than its stride, FCN_CONV_MASK without y2 or with a y2 slice narrower than Cout, a plan that prepare() did not fill,
 *      null dw, pixel splits without a workspace), FCN_E_ALIGN (x_cstride not a multiple of 4 or below round4(Cin); x / w / dw / the
 *      workspace not 16-byte aligned; y / bias / db not 4-byte aligned), FCN_E_UNSUPPORTED (other flags, dilation < 1, more than 4096
 *      taps, more than 65535 problems, tensors past 2^31 elements). ---- */
typedef struct fcn_rconv_desc {
    const float* x;      /* NHWC input, channel stride x_cstride (a multiple of 4, >= round4(Cin))               */
    const float* w;      /* weights [Cout][kh][kw][round4(Cin)]  (OHWI, Cin contiguous, 16-byte aligned)         */
    const float* bias;   /* [Cout] or NULL                                                                       */
    float*       y;      /* NHWC output; channel co of pixel m at y[m*y_cstride + y_coffset + co]                */
    float*       y2;     /* FCN_CONV_MASK: the activation whose sign masks the result (same indexing via y2_*)   */
    int32_t N, H, W, Cin, x_cstride;
    int32_t Cout, kh, kw, pad_h, pad_w, stride_h, stride_w, OH, OW;
    int32_t y_cstride, y_coffset, y2_cstride, y2_coffset;
    int32_t flags;
    int32_t dilation;
} fcn_rconv_desc;
typedef struct fcn_rconv_plan {
    void*   d_probs;
    int32_t n;
    int32_t cfg;          /* tile configuration chosen by prepare() */
    int32_t grid_x, grid_y;
    int32_t total_tiles;
} fcn_rconv_plan;
/* number of tile configurations (cfg_request: -1 = built-in choice, 0 .. count-1); one today: 64 pixels x 64 channels x 16 k */
int    fcn_rconv2d_num_configs(void);
size_t fcn_rconv2d_workspace_bytes(const fcn_rconv_desc* h_descs, int n);
/* validates and uploads n problems into d_workspace with a synchronous copy (plan time, not inside a graph capture); the
 * workspace must stay alive as long as the plan is used */
int    fcn_rconv2d_prepare(const fcn_rconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_rconv_plan* h_out);
/* one pure kernel launch for all problems of the plan: capturable */
int    fcn_rconv2d_f32(const fcn_rconv_plan* h_plan, fcn_stream_t s);
/* The forward in half floats (inference; training stays float32), the contract above with these differences.  The SAME descriptor:
 * its x, w and y point to IEEE halves (declared float* - pass the addresses), y to float32 under FCN_CONV_OUT_F32; bias is float32
 * or NULL.  x: NHWC halves, x_cstride a multiple of 8 and >= round8(Cin), 16-byte aligned; channels Cin .. round8(Cin)-1 of a pixel
 * are padding and are never multiplied.  w: [Cout][kh][kw][round8(Cin)] halves where the layer's parameter blob lies, 16-byte
 * aligned.  Sums are float32 on the matrix cores (v_mfma_f32_32x32x16_f16); a half result is rounded to nearest even once from the
 * float32 sum (after bias and ReLU).  flags: FCN_CONV_RELU | FCN_CONV_OUT_F32; every other flag and a non-NULL y2 are
 * FCN_E_UNSUPPORTED.  y needs 2-byte alignment (4-byte under FCN_CONV_OUT_F32) and any y_cstride >= y_coffset + Cout.  Halves go out
 * in 16-byte stores (eight channels) when y is 16-byte aligned and y_cstride / y_coffset are multiples of 8, in 8-byte stores (four
 * channels) when y is 8-byte aligned with multiples of 4, else in 2-byte stores; float32 results as in the float32 kernel.  A last
 * partial run goes out in scalar stores: a half that shares a 32-bit word with the slice's first or last half is not touched.  The workspace (fcn_rconv2d_workspace_bytes) must be 16-byte aligned (FCN_E_ALIGN).  One launch for all problems
 * of a plan, every output element written by exactly one lane, no atomics: the same bits on every run.
 * A plan records its element type in `cfg`: fcn_rconv2d_prepare numbers its configurations from 0, fcn_rconv2d_prepare_f16 from
 * FCN_RCONV_CFG_F16, and each launch refuses the other's plan with FCN_E_ARG. */
#define FCN_RCONV_CFG_F16 256
/* number of half-float tile configurations (cfg_request: -1 or 0 .. count-1); one today: 64 pixels x 64 channels x 32 k */
int    fcn_rconv2d_num_configs_f16(void);
int    fcn_rconv2d_prepare_f16(const fcn_rconv_desc* h_descs, int n, void* d_workspace, int cfg_request, fcn_rconv_plan* h_out);
/* one pure kernel launch for all problems of the plan: capturable */
int    fcn_rconv2d_f16(const fcn_rconv_plan* h_plan, fcn_stream_t s);
/* Weight / bias gradient, the contract of fcn_conv2d_wgrad_f32: `d` describes the FORWARD problem, d->y / y_cstride / y_coffset name dY
 * (d->w, d->bias, d->y2 and d->flags are ignored).  dw is [Cout][kh][kw][round4(Cin)], 16-byte aligned, and is OVERWRITTEN; its pad
 * columns Cin .. round4(Cin)-1 are written as exact zeros (the solver, clipping and weight decay run over the packed buffer as it is).
 * db is [Cout] or NULL.  The reduction runs over the pixels on the matrix cores; with more than one pixel split every split writes a
 * slab of the workspace (fcn_rconv2d_wgrad_workspace_floats() floats, 16-byte aligned; 0 = none needed, NULL allowed) and a second
 * small launch adds the slabs in ascending order and sums db: bit-reproducible, no atomics.  Nothing outside dw / db / the workspace
 * is written. */
size_t fcn_rconv2d_wgrad_workspace_floats(const fcn_rconv_desc* h_d);
int    fcn_rconv2d_wgrad_f32(const fcn_rconv_desc* h_d, float* dw, float* db, float* d_workspace, fcn_stream_t s);

/* ---- depthwise convolution: Caffe ConvolutionLayer with group == channels == num_output (the 3x3 layers of MobileNet v1 / v2 and
 *      MobileNet-SSD, the separable blocks of Xception / DeepLab-v3+), forward in float32 and in halves, data gradient and weight
 *      gradient, per-axis kernel / pad / stride and one dilation for both axes.  NHWC, vector units (kh*kw multiply-adds per element
 *      moved: bound by memory).  With zeros outside the image:
 *        y[n, oy, ox, c] = bias[c] + sum over r, q of w[r][q][c] * x[n, oy*stride_h - pad_h + r*dil, ox*stride_w - pad_w + q*dil, c]
 *        OH = (H + 2 pad_h - (dil*(kh-1) + 1)) / stride_h + 1     (floor)        OW likewise with kw, pad_w, stride_w
 *      The bank is tap-major and channel-contiguous, [kh][kw][roundS(C)] float32 with S the bottom's 16-byte segment (4 floats, 8
 *      halves), pad channels zero, 16-byte aligned; the bias is float32.  Every call is ONE pure kernel launch (capturable; the weight
 *      gradient with pixel splits: two), needs no prepare step and, forward and data gradient, no workspace and no LDS.  Every output
 *      element is written by exactly one lane, there are no float atomics, a second launch gives the same bits.
 *      cfg_request: -1 = built-in choice (the strip form for stride_w 1 on large blobs), 0 = one output pixel per lane (every geometry), 1 = a strip of output pixels along x per lane
 *      (4 in float32, 2 in halves): stride_w 1 or 2, dilation 1, kw 1 / 3 / 5 / 7, else FCN_E_UNSUPPORTED (a caller walking all
 *      configurations skips it); forward only.
 *      fwd_f32 flags: FCN_CONV_RELU | FCN_CONV_ACCUM | FCN_CONV_MASK, applied in the order accumulate, ReLU, mask; y2 is only read.
 *      fwd_f16: x and y hold halves (8 channels per lane, float32 accumulation, bank and bias float32); flags FCN_CONV_RELU |
 *      FCN_CONV_OUT_F32 (y is float32).
 *      Channels C .. roundS(C)-1 of x are padding: they never reach a real channel of y (they may hold anything); channels of y outside
 *      [y_coffset, y_coffset + C) are not touched.  16-byte stores when y (y2) is 16-byte aligned with strides / offsets in whole
 *      16-byte runs, scalar stores otherwise and for a last partial group.
 *      dgrad_f32: the descriptor is the FORWARD problem; y / y_cstride / y_coffset name dY (read) and x / x_cstride name dX (written,
 *      channels 0 .. C-1 of every pixel): dx[n, iy, ix, c] = sum of w[r][q][c] * dy[n, oy, ox, c] over the taps with oy*stride_h ==
 *      iy + pad_h - r*dil and ox*stride_w == ix + pad_w - q*dil in range - the same bank, no flip, any stride, any pad >= 0.  flags:
 *      FCN_CONV_ACCUM | FCN_CONV_MASK as the other data-gradient passes use them, y2 indexed at dX's pixel; bias is ignored.
 *      Refused on the host before the first HIP call: FCN_E_ARG (null descriptor / x / w / y / dw, non-positive extent or stride,
 *      negative pad, window larger than the padded image, OH / OW not the value above, slice wider than its stride, FCN_CONV_MASK
 *      without y2 or with a y2 slice narrower than C, unknown cfg_request, split_request outside 0 .. min(1024, N*OH*OW), pixel splits
 *      without a workspace), FCN_E_ALIGN (x_cstride not a multiple of S or below roundS(C); x / w / dw / the workspace not 16-byte
 *      aligned; y / bias / db not aligned to their elements), FCN_E_UNSUPPORTED (other flags, dilation < 1, more than 7 x 7 taps, a
 *      configuration that does not take the geometry, tensors past 2^31 elements). ---- */
typedef struct fcn_dwconv_desc {
    void*        x;      /* NHWC input, channel stride x_cstride (a multiple of S, >= roundS(C)); dX for dgrad (written)   */
    const float* w;      /* bank [kh][kw][roundS(C)] float32, 16-byte aligned                                              */
    const float* bias;   /* [C] float32 or NULL                                                                            */
    void*        y;      /* NHWC output; channel c of pixel m at y[m*y_cstride + y_coffset + c]; dY for dgrad / wgrad       */
    float*       y2;     /* FCN_CONV_MASK: the activation whose sign masks the result (same indexing via y2_*)             */
    int32_t N, H, W, C, x_cstride;
    int32_t kh, kw, pad_h, pad_w, stride_h, stride_w, OH, OW;
    int32_t y_cstride, y_coffset, y2_cstride, y2_coffset;
    int32_t flags;
    int32_t dilation;
} fcn_dwconv_desc;
int    fcn_dwconv2d_num_configs(void);
int    fcn_dwconv2d_fwd_f32(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s);
int    fcn_dwconv2d_fwd_f16(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s);
int    fcn_dwconv2d_dgrad_f32(const fcn_dwconv_desc* h_d, int cfg_request, fcn_stream_t s);
/* Weight / bias gradient: `d` describes the FORWARD problem, d->y / y_cstride / y_coffset name dY (d->w, d->bias, d->y2 and d->flags
 * are ignored).  dw is [kh][kw][round4(C)], 16-byte aligned, and is OVERWRITTEN; its pad channels are written as exact zeros whatever
 * the pad channels of x and dY hold.  db is [C] or NULL.  split_request: 0 = built-in choice, n > 0 = n pixel splits (fewer when a
 * split would be empty).  With one split dw and db are written directly; otherwise every split writes a slab of the workspace
 * (fcn_dwconv2d_wgrad_workspace_floats() floats for the same split_request - (kh*kw + 1) * round4(C) per split: the taps' rows, then
 * db's - 16-byte aligned; 0 = none needed, NULL allowed) and a second small launch adds the slabs in a fixed order (64 lanes per column,
 * each its slabs in ascending order, then a fold by halves): bit-reproducible, no atomics, 4 KiB of LDS in either launch. */
size_t fcn_dwconv2d_wgrad_workspace_floats(const fcn_dwconv_desc* h_d, int split_request);
int    fcn_dwconv2d_wgrad_f32(const fcn_dwconv_desc* h_d, float* dw, float* db, float* d_workspace, int split_request, fcn_stream_t s);

/* ---- Crop (Caffe CropLayer: the skip connections and the final score map of the published FCN-32s / 16s / 8s nets): a window copy
 *      between two NHWC views with channel strides, and its adjoint.  x / dX is the N x H x W view, y / dY the N x OH x OW window at
 *      (off_y, off_x); a crop along the channel axis is the caller adding its offset to x_coffset.
 *      Contract, as for fcn_copy_channels_f16: pointers 16-byte aligned and channel strides multiples of 16 bytes (4 floats / 8 halves)
 *      else FCN_E_ALIGN; null pointers, non-positive extents, a slice wider than its stride, a negative offset or off + O > extent on
 *      either axis FCN_E_ARG; a view past 2^31 elements FCN_E_UNSUPPORTED; every check precedes the first HIP call.  Channel offsets
 *      that are both multiples of the 16-byte group move 16 bytes per lane (the last C % group channels one by one), any other offset
 *      one element per lane.  Exactly channels y_coffset .. y_coffset + C - 1 of every output pixel are written, nothing outside
 *      channels x_coffset .. x_coffset + C - 1 of the window of x is read.  One pass, one writer per element, no atomics: results do
 *      not depend on the run. ---- */
/* y[n, oy, ox, y_coffset + c] = x[n, oy + off_y, ox + off_x, x_coffset + c], c < C */
int  fcn_crop_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x,
                      int OH, int OW, int y_cstride, int y_coffset, fcn_stream_t s);
int  fcn_crop_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x,
                      int OH, int OW, int y_cstride, int y_coffset, fcn_stream_t s);
/* the window copy, converting: x holds halves (x_cstride a multiple of 8), y float32 (y_cstride a multiple of 4) - the final score map of
 * a half-float FCN net, a float32 net output.  Exact.  16 bytes of halves per lane when x_coffset is a multiple of 8 and y_coffset of 4 */
int  fcn_crop_fwd_f16_f32(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int off_y, int off_x,
                          int OH, int OW, int y_cstride, int y_coffset, fcn_stream_t s);
/* accumulate 0: ONE launch writes channels dx_coffset .. dx_coffset + C - 1 of every pixel of dX - dY inside the window, zeros outside
 * (no memset in front).  accumulate 1: dX += dY inside the window and nothing outside it is touched (a blob with several consumers).
 * There is no half-float twin: the half-float engine is inference only. */
int  fcn_crop_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset, int off_y, int off_x,
                      int OH, int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);

/* ---- Interp (DeepLab-Caffe's InterpLayer: fc8_interp and label_shrink of the published DeepLab nets, the resizing of a pyramid-pooling
 *      head): bilinear resampling with aligned corners between two NHWC views with channel strides, and its adjoint.  x / dX is the
 *      N x H x W bottom, of which rows and columns -pad_beg .. H + pad_end - 1 (W alike) are the effective input of He x We; y / dY is
 *      N x OH x OW.  Output index o of n2 lies at position o (n1 - 1) / (n2 - 1) of the effective input's n1, kept in integers: cell
 *      i0 = num / (n2 - 1), neighbour i1 = min(i0 + 1, n1 - 1) with weight lam = float(num % (n2 - 1)) / float(n2 - 1), num = o (n1 - 1);
 *      position 0 when n1 or n2 is 1.  y = (1-ly) ((1-lx) p00 + lx p01) + ly ((1-lx) p10 + lx p11) in float32 without contraction; a
 *      weight of zero selects the pixel itself, so equal extents - and every output that falls on an input pixel - copy bit for bit.
 *      Contract: null pointers, non-positive extents, a positive pad, an effective extent below 1 or a slice wider than its stride
 *      FCN_E_ARG; a row or an axis past 2^31 lanes (OH * He, OW * We, W * x_cstride, OW * y_cstride, N * H, N * OH) or an output
 *      extent past 2^24 FCN_E_UNSUPPORTED; element offsets are 64-bit, so the views themselves may pass 2^31 bytes; every check precedes
 *      the first HIP call.  float32: strides and channel offsets that are all multiples of 4 floats under 16-byte aligned pointers move
 *      16 bytes per lane (the last C % 4 channels one by one), anything else one element per lane.  Exactly channels y_coffset ..
 *      y_coffset + C - 1 of every output pixel are written, nothing outside channels x_coffset .. x_coffset + C - 1 of the effective
 *      input is read.  No atomics anywhere: results do not depend on the run. ---- */
int  fcn_interp_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                        int OH, int OW, int y_cstride, int y_coffset, fcn_stream_t s);
/* halves in; halves (out_f32 0) or float32 (out_f32 1: a net's output behind the layer) out, rounded once from the float32 blend.  The
 * pointers must be 16-byte aligned, x_cstride and x_coffset multiples of 8 halves, y_cstride and y_coffset of 8 halves or 4 floats, else
 * FCN_E_ALIGN; C is free (the last C % 8 channels move one by one). */
int  fcn_interp_fwd_f16(const void* x, void* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                        int OH, int OW, int y_cstride, int y_coffset, int out_f32, fcn_stream_t s);
/* The adjoint as a gather: a pixel of dX sums, in ascending output row and ascending output column inside a row, the pixels of dY it fed
 * with a weight that is not zero.  accumulate 0: ONE launch writes channels dx_coffset .. dx_coffset + C - 1 of every pixel of dX - zero
 * where nothing feeds it: cropped away by the pads, or never read by a shrink (no memset in front).  accumulate 1: dX += the sum at the
 * pixels something feeds, and nothing else is touched (a blob with several consumers).  There is no half-float twin. */
int  fcn_interp_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, int dx_cstride, int dx_coffset, int pad_beg, int pad_end,
                        int OH, int OW, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);

/* ---- Upsample (the SegNet fork's UpsampleLayer: unpooling by the indices of an encoder's MAX pooling), its adjoint, and the pooling mask.
 *      idx is the packed [N * PH * PW][C] int32 argmax that fcn_maxpool_fwd_f32 / fcn_maxpool_idx_fwd_f16 write: iy * W + ix in the H x W
 *      plane of the pooling's bottom (-1: the window held no maximum).  x / dX is the pooled-size N x PH x PW view, y / dY the N x H x W
 *      one; k, stride and pad are the POOLING's, and PH / PW must be its ceil-mode extents of H / W (FCN_E_ARG otherwise, as for null
 *      pointers, non-positive extents and slices that leave their pixel).  Forward is a gather over y: y[n, idx[n, py, px, c], c] =
 *      x[n, py, px, c] and every other element of channels y_coffset .. y_coffset + C - 1 is written as +0.0 - one launch, no memset in
 *      front, no atomics, one writer per element.  Where windows overlap (k > stride) and several name one pixel, the window last in
 *      ascending (py, px) order wins: what Caffe's serial scatter leaves.  Only the windows that cover a pixel are asked about it: an
 *      index that lies outside its own window is never followed.  A lane moves 16 bytes of channels where C, the strides, the offsets and
 *      the pointers allow and single elements otherwise; pad channels of x may be read and never reach a written value; channels of y
 *      outside the slice are not written.  Pointers must be multiples of 4 bytes (FCN_E_ALIGN); a view of 2^31 elements or more is
 *      FCN_E_UNSUPPORTED.  Every refusal precedes the first HIP call.  Floor: the bytes of x + idx + y. ---- */
int  fcn_unpool_fwd_f32(const float* x, const int32_t* idx, float* y, int N, int PH, int PW, int C, int x_cstride, int x_coffset, int k, int stride,
                        int pad, int H, int W, int y_cstride, int y_coffset, fcn_stream_t s);
/* halves in (8-half segments: x 16-byte aligned, x_cstride and x_coffset multiples of 8, else FCN_E_ALIGN; C is free); halves out (out_f32
 * 0: y likewise) or float32 out (out_f32 1: a net's output behind the layer; any 4-byte aligned view, 16-byte stores where it allows).
 * idx stays int32. */
int  fcn_unpool_fwd_f16(const void* x, const int32_t* idx, void* y, int N, int PH, int PW, int C, int x_cstride, int x_coffset, int k, int stride,
                        int pad, int H, int W, int y_cstride, int y_coffset, int out_f32, fcn_stream_t s);
/* Upsample backward, a pure gather: dx[n, py, px, c] = dy[n, idx[n, py, px, c], c] (accumulate 0; 0 where idx is outside the plane) or
 * dx += the same in one float32 add (accumulate 1).  Every window that names a pixel receives its gradient, as in Caffe.  No half twin. */
int  fcn_unpool_bwd_f32(const float* dy, const int32_t* idx, float* dx, int N, int PH, int PW, int C, int dx_cstride, int dx_coffset, int k,
                        int stride, int pad, int H, int W, int dy_cstride, int dy_coffset, int accumulate, fcn_stream_t s);
/* fcn_maxpool_fwd_f16 that also writes idx (required), by the rule of fcn_maxpool_fwd_f32: window clipped to the image, first maximum in
 * raster order.  One kernel for every geometry; OH / OW must be the ceil-mode extents (FCN_E_ARG); C, the strides and y_coffset multiples
 * of 8 and all three pointers 16-byte aligned (FCN_E_ALIGN).  y equals fcn_maxpool_fwd_f16's bit for bit. */
int  fcn_maxpool_idx_fwd_f16(const void* x, void* y, int32_t* idx, int N, int H, int W, int C, int x_cstride, int k, int stride, int pad, int OH,
                             int OW, int y_cstride, int y_coffset, fcn_stream_t s);
/* the packed int32 argmax as Caffe's mask blob: dst (N x C x PH x PW float32, dense) = (float)idx.  For read-back only. */
int  fcn_pool_mask_to_nchw_f32(const int32_t* idx, float* dst, int N, int PH, int PW, int C, fcn_stream_t s);

/* ---- InnerProduct (Caffe InnerProductLayer) at M <= FCN_IP_MAX_ROWS input rows: y[m][n] = sum_k x[m][k] * w[n][k] + bias[n].
 *      x: M rows of K elements, x_rstride elements apart (a row of an NHWC blob of H*W*cstride elements IS such a row); w: the bank
 *      [N][K], K contiguous, in the order of the elements of a row of x (zero columns where x holds pad channels); y / dY: M pixels of
 *      y_cstride channels, the layer's N outputs at channel y_coffset (a member of a Concat over (N, C) blobs is written in place); bias may be NULL.
 *      At these row counts the layer is a stream over the bank: every byte of w (and of dW) crosses the memory bus once per call for
 *      every M, in 16-byte accesses; sums over lanes, over K slices (forward) and over slices of the rows of w (bwd_data) are combined
 *      in a fixed order, without atomics: the same call gives the same bits.  Shapes that are split leave partial sums in d_workspace
 *      (fcn_inner_product_workspace_bytes(M, K, N) bytes, valid for all four entry points and both element types; 0: none is needed and
 *      d_workspace may be NULL) and run a second small launch; all launches are capturable.
 *      Contract: null pointers (x, w, y, dy, dx, dw; the workspace where one is needed), non-positive extents, a row stride below K, a
 *      slice outside its pixel, unknown flags FCN_E_ARG; pointers off 16 bytes, K or a stride that is not a multiple of 16 bytes (4 floats
 *      / 8 halves) FCN_E_ALIGN; M > FCN_IP_MAX_ROWS (those row counts run through fcn_ip_gemm_* below, on the same operands), N * K
 *      or a view past 2^31 elements FCN_E_UNSUPPORTED.  Every check precedes the first HIP call. ---- */
#define FCN_IP_MAX_ROWS 32
#define FCN_IP_WEIGHTS_NT 256   /* forward flag: the loads of w carry the non-temporal hint (a bank read once, from cold caches) */
size_t fcn_inner_product_workspace_bytes(int M, int K, int N);
/* what the forward of one element type alone needs (esize 4: float32, 2: half floats; anything else 0): an inference engine holds
 * this per layer instead of the slabs of bwd_data, which are tens of megabytes for a large bank */
size_t fcn_inner_product_fwd_workspace_bytes(int M, int K, int N, int esize);
/* flags: FCN_CONV_RELU | FCN_IP_WEIGHTS_NT */
int  fcn_inner_product_fwd_f32(const float* x, int x_rstride, const float* w, const float* bias, float* y, int y_cstride, int y_coffset,
                               int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* x, w and y hold half floats, float32 accumulation and bias; flags: FCN_CONV_RELU | FCN_CONV_OUT_F32 (y is float32) | FCN_IP_WEIGHTS_NT */
int  fcn_inner_product_fwd_f16(const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset,
                               int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* The two backward entry points (the training planner applies the layer's own ReLU mask to dY before these calls).
 * dX[m][k] (+)= sum_n dY[m][n] * w[n][k];  flags: FCN_CONV_ACCUM adds into dX (gradient fan-in) */
int  fcn_inner_product_bwd_data_f32(const float* dy, int dy_cstride, int dy_coffset, const float* w, float* dx, int dx_rstride,
                                    int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* dW[n][k] (+)= sum_m dY[m][n] * x[m][k];  db[n] (+)= sum_m dY[m][n] (db may be NULL);  accumulate 1 adds (iter_size) */
int  fcn_inner_product_bwd_weights_f32(const float* x, int x_rstride, const float* dy, int dy_cstride, int dy_coffset,
                                       float* dw, float* db, int M, int K, int N, int accumulate, fcn_stream_t s);

/* ---- InnerProduct at any row count on the matrix cores (csrc/ip_gemm.hip): the same four products on the same operands as the block
 *      above - rows of x with a stride, the bank [N][K], y / dY as a channel window of wider pixels, bias may be NULL, ReLU in the
 *      forward epilogue - as an LDS-tiled GEMM (v_mfma_f32_32x32x2_f32 / v_mfma_f32_32x32x16_f16, float32 accumulation and bias).  Any
 *      M >= 1 is legal; engines send M > FCN_IP_MAX_ROWS here and M <= FCN_IP_MAX_ROWS to the streaming kernels, whose results these do
 *      not reproduce bit for bit (another order of summation).  One kernel serves all three products: forward reduces over K, bwd_data
 *      over N, bwd_weights over M; elements of a reduction past its end are zeros in registers and are never loaded (what lies behind
 *      the K elements of a row of x is never read), rows past M or N are never stored, and nothing outside [y_coffset, y_coffset + N)
 *      of a y pixel, [0, K) of a dX row or the N x K of dW is written.  No atomics: a shape with too few 64 x 64 output tiles to fill
 *      the chip has its reduction cut into slices - a function of (M, K, N, esize) alone - which leave float32 partial tiles in
 *      d_workspace; a second small launch adds them in slice order and applies bias, ReLU and accumulate.  The same call gives the same
 *      bits.  fcn_ip_gemm_workspace_bytes(M, K, N, esize) (esize 4: float32, all three products; 2: the half-float forward; anything
 *      else, or a non-positive extent: 0) is what any one call needs; 0: none is needed and d_workspace may be NULL.  Calls that run at
 *      the same time (the weight gradient on a second stream beside bwd_data) need a workspace each.
 *      Contract: as the block above without the row limit - null pointers (the workspace where one is needed), non-positive extents, a
 *      row stride below K, a slice outside its pixel, unknown flags FCN_E_ARG; pointers off 16 bytes, K or a stride that is not a
 *      multiple of 16 bytes FCN_E_ALIGN; N * K or a view past 2^31 elements FCN_E_UNSUPPORTED.  Every check precedes the first HIP
 *      call; all launches are capturable. ---- */
size_t fcn_ip_gemm_workspace_bytes(int M, int K, int N, int esize);
/* flags: FCN_CONV_RELU */
int  fcn_ip_gemm_fwd_f32(const float* x, int x_rstride, const float* w, const float* bias, float* y, int y_cstride, int y_coffset,
                         int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* x, w and y hold half floats; flags: FCN_CONV_RELU | FCN_CONV_OUT_F32 (y is float32) */
int  fcn_ip_gemm_fwd_f16(const void* x, int x_rstride, const void* w, const float* bias, void* y, int y_cstride, int y_coffset,
                         int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* dX[m][k] (+)= sum_n dY[m][n] * w[n][k];  flags: FCN_CONV_ACCUM adds the finished sum into dX (one rounded add per element) */
int  fcn_ip_gemm_bwd_data_f32(const float* dy, int dy_cstride, int dy_coffset, const float* w, float* dx, int dx_rstride,
                              int M, int K, int N, int flags, void* d_workspace, fcn_stream_t s);
/* dW[n][k] (+)= sum_m dY[m][n] * x[m][k];  db[n] (+)= sum_m dY[m][n] in row order (db may be NULL);  accumulate 1 adds (iter_size) */
int  fcn_ip_gemm_bwd_weights_f32(const float* x, int x_rstride, const float* dy, int dy_cstride, int dy_coffset,
                                 float* dw, float* db, int M, int K, int N, int accumulate, void* d_workspace, fcn_stream_t s);

/* ---- BatchNorm / Scale (Caffe BatchNormLayer, ScaleLayer over the channel axis) on NHWC views (csrc/batchnorm.hip).
 *      Views are the usual (pixels, C, cstride, coffset); a lane owns one 16-byte channel group of a pixel (4 floats / 8 halves).  Only
 *      channels coffset .. coffset + C - 1 of a view are ever written (C need not be a multiple of the group: the last group is stored
 *      in part, as fcn_avepool_bwd_f32 does); whole groups are LOADED, so strides and offsets are multiples of the group.
 *      Reductions use no atomics: slabs of pixels are folded by one workgroup each, their partial results lie in d_workspace
 *      (fcn_batchnorm_workspace_bytes(pixels, C) bytes, for both reducing entry points) and a second launch folds them per channel in a
 *      fixed order (lane l of a wave folds slabs l, l + 64, .. ascending, then the lanes fold by halves).  The same call gives the same bits.
 *      Contract of all five: null pointers, non-positive extents, a slice outside its pixel, operands that must come together and do not
 *      FCN_E_ARG; a stride or offset that is no multiple of the group, x / y / dy / dx / xhat / workspace off 16 bytes FCN_E_ALIGN.  Every
 *      check precedes the first HIP call; all launches are capturable. ---- */
size_t fcn_batchnorm_workspace_bytes(int pixels, int C);
/* Batch statistics of a view: save[c] = mean, save[C + c] = 1 / sqrt(var + eps), var = E[(x - mean)^2] (biased), centred per slab and
 * combined by Chan's formula - never E[x^2] - E[x]^2.  The three blobs (all or none) get Caffe's moving-average step in the same launch:
 * factor = factor * f + 1, mean_sum = mean_sum * f + mean, var_sum = var_sum * f + var * (m / (m - 1) if m > 1 else 1), m = pixels. */
int  fcn_batchnorm_stats_f32(const float* x, int pixels, int C, int x_cstride, int x_coffset, float* blob_mean, float* blob_var,
                             float* blob_factor, float moving_average_fraction, float eps, float* save, void* d_workspace, fcn_stream_t s);
/* y = relu?(gamma[c] * xhat + beta[c]), xhat = (x - mean[c]) * invstd[c].  mean / invstd: `save` (as fcn_batchnorm_stats_f32 left it), or
 * computed per channel from the three blobs in the kernel's prologue (global statistics: s = factor == 0 ? 0 : 1 / factor, mean = s *
 * mean_sum, invstd = 1 / sqrt(s * var_sum + eps)), or (0, 1) when both are NULL (Scale alone).  gamma, beta NULL: 1, 0.  xhat (may be
 * NULL): a buffer of its own, xhat_cstride floats per pixel, the view's channels at 0.  y may be x. */
int  fcn_batchnorm_apply_f32(const float* x, float* y, float* xhat, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                             int xhat_cstride, const float* save, const float* blob_mean, const float* blob_var, const float* blob_factor, float eps,
                             const float* gamma, const float* beta, int relu, fcn_stream_t s);
/* inference twin: x and y hold halves (groups of 8), the blobs, gamma and beta stay float32, arithmetic in float32 */
int  fcn_batchnorm_apply_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                             const float* blob_mean, const float* blob_var, const float* blob_factor, float eps, const float* gamma,
                             const float* beta, int relu, fcn_stream_t s);
/* sum_dy[c] = sum dy', sum_dyx[c] = sum dy' * xhat over the pixels; dy' = dy where relu_y > 0 and 0 elsewhere (relu_y NULL: dy' = dy).
 * With a Scale in the chain these are d(beta) and d(gamma); for Scale alone xhat is the layer's input.  Both are overwritten. */
int  fcn_batchnorm_bwd_reduce_f32(const float* dy, const float* xhat, const float* relu_y, int pixels, int C, int dy_cstride, int dy_coffset,
                                  int xhat_cstride, int xhat_coffset, int y_cstride, int y_coffset, float* sum_dy, float* sum_dyx,
                                  void* d_workspace, fcn_stream_t s);
/* dx (+)= gamma * invstd * (dy' - sum_dy / m - xhat * sum_dyx / m), m = pixels; with the sums NULL (global statistics, Scale alone)
 * dx (+)= gamma * invstd * dy' and xhat may be NULL.  invstd: save[C + c], or from blob_var / blob_factor / eps, or 1.  dx may be dy. */
int  fcn_batchnorm_bwd_apply_f32(const float* dy, const float* xhat, const float* relu_y, float* dx, int pixels, int C, int dy_cstride,
                                 int dy_coffset, int xhat_cstride, int xhat_coffset, int y_cstride, int y_coffset, int dx_cstride, int dx_coffset,
                                 const float* save, const float* blob_var, const float* blob_factor, float eps, const float* gamma,
                                 const float* sum_dy, const float* sum_dyx, int accumulate, fcn_stream_t s);

/* ---- Gated Scale (Caffe ScaleLayer with two bottoms over axis 0; with the residual, the SENet release's Axpy) on NHWC views
 *      (csrc/gate.hip): a per-image, per-channel multiplier taken from a blob of the net.  N images of ppi pixels each lie one behind
 *      the other in every view; the gate is float32, N rows of C values g_rstride >= C floats apart (4-byte aligned, read element by
 *      element, once per lane - never per pixel).  Views, groups and pad channels follow fcn_batchnorm_apply_*: a lane owns one 16-byte
 *      channel group of a pixel (4 floats / 8 halves), whole groups are LOADED (strides and offsets are multiples of the group), only
 *      channels coffset .. coffset + C - 1 are ever written.
 *      Contract of all four: null pointers, non-positive extents, a slice outside its pixel, g_rstride < C FCN_E_ARG; a stride or offset
 *      that is no multiple of the group, x / r / y / dy / dx / workspace off 16 bytes, the gate off 4 bytes FCN_E_ALIGN; more than 65535
 *      images or N * ppi >= 2^31 FCN_E_UNSUPPORTED.  Every check precedes the first HIP call; all launches are capturable. ---- */
/* y = relu?(x * gate[n, c] (+ r)): r may be NULL (its stride and offset are then ignored), relu applies after the add.  y may be x or r. */
int  fcn_scale_gate_fwd_f32(const float* x, const float* gate, const float* r, float* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                            int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s);
/* inference twin: x, r and y hold halves (groups of 8), the gate stays float32, arithmetic in float32, one rounding to half */
int  fcn_scale_gate_fwd_f16(const void* x, const float* gate, const void* r, void* y, int N, int ppi, int C, int x_cstride, int x_coffset,
                            int g_rstride, int r_cstride, int r_coffset, int y_cstride, int y_coffset, int relu, fcn_stream_t s);
/* dx (+)= dy * gate[n, c]; accumulate 1 adds into dx.  dx may be dy. */
int  fcn_scale_gate_bwd_data_f32(const float* dy, const float* gate, float* dx, int N, int ppi, int C, int dy_cstride, int dy_coffset,
                                 int g_rstride, int dx_cstride, int dx_coffset, int accumulate, fcn_stream_t s);
/* dgate[n, c] (+)= sum over the pixels of image n of dy * x, rows of dgate g_rstride floats apart.  No atomics: one workgroup folds a
 * slab of one image's pixels, the partial sums lie in d_workspace (fcn_scale_gate_workspace_bytes(N, ppi, C) bytes) and a second launch
 * folds them per (image, channel) in a fixed order (lane l of a wave folds slabs l, l + 64, .. ascending, then the lanes fold by
 * halves).  One launch pair covers all images; the same call gives the same bits. */
int  fcn_scale_gate_bwd_gate_f32(const float* dy, const float* x, float* dgate, int N, int ppi, int C, int dy_cstride, int dy_coffset,
                                 int x_cstride, int x_coffset, int g_rstride, int accumulate, void* d_workspace, fcn_stream_t s);
size_t fcn_scale_gate_workspace_bytes(int N, int ppi, int C);

/* ---- One-bottom activations with or without a learned per-channel parameter (Caffe PReLULayer, TanHLayer, BiasLayer over the channel
 *      axis) on NHWC views (csrc/act.hip).  Views, groups and pad channels follow fcn_batchnorm_apply_* and fcn_scale_gate_*: a lane owns
 *      one 16-byte channel group of a pixel (4 floats / 8 halves), whole groups are LOADED (strides and offsets are multiples of the
 *      group), only channels coffset .. coffset + C - 1 are ever written.  `param` is float32 in both element types: C values, or ONE
 *      value with param_shared (Caffe's channel_shared); it is read once per lane, never per pixel, and is NULL for TanH.
 *      Contract of all four: null operands, non-positive extents, an unknown mode, a slice outside its pixel, a missing parameter
 *      FCN_E_ARG; a stride or offset that is no multiple of the group, x / y / keep / dy / ref / dx / workspace off 16 bytes, param /
 *      dparam off 4 bytes FCN_E_ALIGN.  Every check precedes the first HIP call; all launches are capturable. ---- */
enum { FCN_ACT_PRELU = 0, FCN_ACT_TANH = 1, FCN_ACT_BIAS = 2 };
/* PReLU: y = x > 0 ? x : param[c] * x.  TanH: y = tanh(x).  Bias: y = x + param[c].  y may be x.  keep may be NULL; otherwise it is a
 * buffer of its own, keep_cstride >= C floats per pixel (a multiple of 4) with the view's channels at 0, and receives x unchanged in the
 * same launch (Caffe's bottom_memory_ of an in-place PReLU; laid out as xhat is for fcn_batchnorm_apply_f32). */
int  fcn_act_fwd_f32(const float* x, float* y, float* keep, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                     int keep_cstride, int mode, const float* param, int param_shared, fcn_stream_t s);
/* inference twin: x and y hold halves (groups of 8), param stays float32, arithmetic in float32, one rounding to half; no keep */
int  fcn_act_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset, int mode,
                     const float* param, int param_shared, fcn_stream_t s);
/* PReLU: ref is the layer's INPUT x (the kept copy where the layer ran in place), dx (+)= x > 0 ? dy : param[c] * dy.  TanH: ref is the
 * layer's OUTPUT y, dx (+)= dy * (1 - y * y).  Bias: ref is NULL (its stride and offset are ignored), dx (+)= dy.  accumulate 1 adds
 * into dx; dx may be dy when accumulate is 0. */
int  fcn_act_bwd_data_f32(const float* dy, const float* ref, float* dx, int pixels, int C, int dy_cstride, int dy_coffset, int ref_cstride,
                          int ref_coffset, int dx_cstride, int dx_coffset, int mode, const float* param, int param_shared, int accumulate,
                          fcn_stream_t s);
/* PReLU: dparam[c] = sum over the pixels of dy * x * [x <= 0].  Bias: dparam[c] = sum of dy (x may be NULL).  With param_shared ONE value:
 * the per-channel sums folded over the channels in ascending order.  The result is OVERWRITTEN (as fcn_batchnorm_bwd_reduce_f32's sums
 * are).  No atomics: one workgroup folds a slab of pixels, the partial sums lie in d_workspace (fcn_act_workspace_bytes(pixels, C) bytes)
 * and a second launch folds them per channel in a fixed order (lane l of a wave folds slabs l, l + 64, .. ascending, then the lanes fold
 * by halves); the same call gives the same bits.  TanH has no parameter: FCN_E_ARG. */
int  fcn_act_bwd_param_f32(const float* dy, const float* x, float* dparam, int pixels, int C, int dy_cstride, int dy_coffset, int x_cstride,
                           int x_coffset, int mode, int param_shared, void* d_workspace, fcn_stream_t s);
size_t fcn_act_workspace_bytes(int pixels, int C);

/* ---- One-bottom activations without a learned parameter (Caffe ELULayer, ClipLayer - with 0 and 6 the MobileNet forks' ReLU6 -,
 *      AbsValLayer, BNLLLayer, SwishLayer) on NHWC views (csrc/neuron.hip).  Views, groups and pad channels follow fcn_act_*: a lane owns
 *      one 16-byte channel group of a pixel (4 floats / 8 halves), whole groups are LOADED (strides and offsets are multiples of the
 *      group), only channels coffset .. coffset + C - 1 are ever written.  `a` is alpha (ELU), beta (Swish) or lo (Clip), `b` is hi
 *      (Clip); both are ignored by the other modes.  Float32 arithmetic in both element types (expm1f / log1pf, not expf - 1).
 *      Contract of all three: null operands, non-positive extents, an unknown mode, a slice outside its pixel, a < 0 for ELU, a >= b
 *      for Clip FCN_E_ARG; a stride or offset that is no multiple of the group, x / y / keep / dy / ref / dx off 16 bytes FCN_E_ALIGN.
 *      Every check precedes the first HIP call; all launches are capturable.  No LDS, no atomics, one writer per element: the same
 *      call gives the same bits. ---- */
enum { FCN_NEURON_ELU = 0, FCN_NEURON_CLIP = 1, FCN_NEURON_ABSVAL = 2, FCN_NEURON_BNLL = 3, FCN_NEURON_SWISH = 4 };
/* ELU: y = x > 0 ? x : a * expm1(x).  Clip: y = min(max(x, a), b).  AbsVal: y = |x|.  BNLL: y = x > 0 ? x + log1p(exp(-x)) : log1p(exp(x)).
 * Swish: y = x / (1 + exp(-a x)).  y may be x.  keep may be NULL; otherwise it is a buffer of its own, keep_cstride >= C floats per pixel
 * (a multiple of 4) with the view's channels at 0, and receives x unchanged in the same launch (the input of an in-place Swish for its
 * backward pass; laid out as fcn_act_fwd_f32's keep). */
int  fcn_neuron_fwd_f32(const float* x, float* y, float* keep, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                        int keep_cstride, int mode, float a, float b, fcn_stream_t s);
/* inference twin: x and y hold halves (groups of 8), arithmetic in float32, one rounding to half; no keep.  A last, partial group is
 * stored as 32-bit pairs and, where C is odd, one half: the pad half that shares its word is not written. */
int  fcn_neuron_fwd_f16(const void* x, void* y, int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset, int mode, float a,
                        float b, fcn_stream_t s);
/* ref is the layer's OUTPUT y for ELU (dx (+)= dy * (y > 0 ? 1 : y + a)), Clip (dy * [a < y < b], both strict) and BNLL (dy * -expm1(-y)),
 * and its INPUT x for AbsVal (dy * sign(x), sign(0) = 0) and Swish (dy * (a y + s (1 - a y)), s = sigmoid(a x) and y = x s recomputed; in
 * place: the kept copy).  accumulate 1 adds into dx; dx may be dy when accumulate is 0. */
int  fcn_neuron_bwd_f32(const float* dy, const float* ref, float* dx, int pixels, int C, int dy_cstride, int dy_coffset, int ref_cstride,
                        int ref_coffset, int dx_cstride, int dx_coffset, int mode, float a, float b, int accumulate, fcn_stream_t s);

/* ---- Channel shuffle (the ShuffleChannel layer of the ShuffleNet ports) on NHWC views (csrc/shuffle.hip).  With n = C / group, for every
 *      pixel y[j * group + i] (+)= x[i * n + j], 0 <= i < group, 0 <= j < n: values are moved, never computed (accumulate's add apart).
 *      The inverse permutation is the same call with group C / group - the layer's data gradient.  group 1 and group C are the identity.
 *      Views and groups follow fcn_act_*: a lane owns one 16-byte channel group of a pixel of y (4 floats / 8 halves), gathers its source
 *      channels from the same pixel of x one by one and stores the group whole; a last, partial group is stored in pieces.  Only channels
 *      x_coffset .. x_coffset + C - 1 of x are read and only channels y_coffset .. y_coffset + C - 1 of y are written.
 *      Contract of both: null operands, non-positive extents, group < 1 or C % group != 0, a slice outside its pixel FCN_E_ARG; a stride or
 *      offset that is no multiple of the 16-byte group, x / y off 16 bytes FCN_E_ALIGN; windows of x and y whose byte ranges (first to last
 *      element) intersect FCN_E_ARG - the layer cannot run in place.  Every check precedes the first HIP call; both launches are
 *      capturable.  No LDS, no atomics, one writer per element: the same call gives the same bits. ---- */
/* accumulate 1 adds into y (a gradient view that already holds one); 0 overwrites. */
int  fcn_shuffle_channel_f32(const float* x, float* y, int pixels, int C, int group, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                             int accumulate, fcn_stream_t s);
/* inference twin: x and y hold halves (groups of 8); no accumulate.  A last, partial group is stored as 32-bit pairs and, where C is odd,
 * one half: the pad half that shares its word is not written. */
int  fcn_shuffle_channel_f16(const void* x, void* y, int pixels, int C, int group, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                             fcn_stream_t s);

/* ---- SSD detection head (Caffe-SSD's Permute + Flatten + Concat, Normalize and DetectionOutput; csrc/ssd.hip).  Float32, inference.
 *      Common contract: every output element has exactly one writer lane (no float atomics anywhere), so a second launch on the same
 *      inputs gives the same bytes; nothing outside the named outputs and the workspace is written; every refusal is made on the host
 *      before the first HIP call (null pointers, non-positive extents, ranges that leave their row or pixel FCN_E_ARG; pointers off their
 *      alignment FCN_E_ALIGN; extents past 2^31 elements and sizes beyond a kernel's plan FCN_E_UNSUPPORTED); all launches are capturable.
 *      The file is compiled without fused multiply-add contraction: a rebuild does not move a decision of the NMS. ---- */
#define FCN_SSD_MAX_HEADS 16
typedef struct fcn_ssd_head {
    const float* src;          /* channel 0 of pixel 0 of image 0 of the head's NHWC buffer                                      */
    int32_t pixels;            /* H * W per image                                                                                */
    int32_t C;                 /* real channels per pixel                                                                        */
    int32_t cstride;           /* floats per pixel in src                                                                        */
    int32_t coffset;           /* the head's first channel inside a pixel                                                        */
    int32_t dst_col;           /* column of a destination row where the head's pixels * C floats start (any value, odd included) */
    int32_t reserved;          /* 0                                                                                              */
} fcn_ssd_head;
/* Permute(0,2,3,1) + Flatten + Concat(axis 1) of up to FCN_SSD_MAX_HEADS heads in ONE launch:
 *   dst[n * dst_rstride + dst_col + p * C + c] = src[(n * pixels + p) * cstride + coffset + c]      for every head, n < N, p < pixels, c < C.
 * A head whose source runs and destination runs are all 16-byte aligned (C, cstride, coffset, dst_col, dst_rstride multiples of 4, both
 * pointers on 16 bytes) moves 16 bytes per lane, any other head one float per lane.  Pad channels of a source pixel are never read;
 * columns of dst outside the heads' ranges are never written.  Heads whose column ranges overlap, or leave dst_cols, are FCN_E_ARG. */
int  fcn_ssd_gather_f32(const fcn_ssd_head* h_heads, int n_heads, int N, float* dst, int dst_rstride, int dst_cols, fcn_stream_t s);
/* Normalize (across_spatial: false): y[c] = scale[c] * (x[c] / sqrt(sum_c x[c]^2 + eps)) per pixel; channel_shared: scale[0] for every c.
 * One wave per pixel.  The sum is taken in a fixed order: lane l adds x[c]^2 for c = l, l + 64, l + 128, .. ascending, then the 64 lanes
 * fold by halves (partner lane ^ 32, ^ 16, .. ^ 1).  Pad channels of x are never read; channels C .. r4(C) - 1 of the y view are written
 * as zeros (y_cstride >= y_coffset + r4(C)).  y may be x. */
int  fcn_normalize_fwd_f32(const float* x, float* y, const float* scale, int pixels, int C, int x_cstride, int x_coffset, int y_cstride,
                           int y_coffset, int channel_shared, float eps, fcn_stream_t s);
/* DetectionOutput (share_location: true, eta 1).  loc: N rows of P * 4 floats, conf: N rows of P * num_classes floats (row strides in
 * floats), priors: P * 4 corners followed by P * 4 variances, as a PriorBox top lies in memory.  The order of steps is the contract:
 *   1. decode every prior once per image.  FCN_CODE_CENTER_SIZE: cx = v0 l0 pw + pcx, cy = v1 l1 ph + pcy, w = exp(v2 l2) pw,
 *      h = exp(v3 l3) ph, corners c -+ size / 2; FCN_CODE_CORNER: corner_i = prior_i + v_i l_i; v = 1 under variance_encoded.  No clipping.
 *   2. per image and class c != background: the priors with conf > conf_threshold (strictly), by score descending, ties by prior index
 *      ascending, cut to top_k when top_k > -1.  Scores and threshold are any floats (logits, Caffe's default threshold -FLT_MAX: every
 *      prior of a class goes in); -0 and +0 are one score, a NaN score is above no threshold.
 *   3. greedy NMS in that order: a candidate is kept iff its Jaccard overlap with every box kept so far is <= nms_threshold.  The overlap
 *      is 0 when the boxes do not intersect, else inter / (a1 + a2 - inter); a box with xmax < xmin or ymax < ymin has area 0; no +1.
 *   4. per image, when keep_top_k > -1 and more survive: the keep_top_k highest scores; ties by label ascending, then prior index
 *      ascending (Caffe's std::sort leaves them unspecified; this order is fixed here).
 *   5. rows [image, label, score, xmin, ymin, xmax, ymax] by image ascending, label ascending and within a label in NMS order, into
 *      out_rows; their number into *out_count.  Rows at and past the count are not written.
 * One workgroup per (image, class) selects (compaction, ranking of the 64-bit keys (score bits, ~index) through LDS tiles) and sweeps;
 * one per image cuts and writes.  top_k (or P when top_k is -1) above FCN_DETOUT_MAX_TOPK and products past 2^31 are FCN_E_UNSUPPORTED;
 * `capacity` rows below what N images can yield is FCN_E_CAPACITY; a workspace below fcn_detection_output_workspace_bytes() FCN_E_ARG,
 * off 16 bytes FCN_E_ALIGN.  The size query returns 0 for parameters the launch would refuse. */
#define FCN_DETOUT_MAX_TOPK 1024
#define FCN_CODE_CORNER 1
#define FCN_CODE_CENTER_SIZE 2
typedef struct fcn_detout_params {
    int32_t N, P, num_classes, background;       /* background: label that is never emitted (-1: none)      */
    int32_t code_type, variance_encoded;
    int32_t top_k, keep_top_k;                   /* -1: no cut                                             */
    float conf_threshold, nms_threshold;
    int32_t loc_rstride, conf_rstride;           /* floats between the rows of two images                  */
    int32_t capacity;                            /* rows that out_rows holds                               */
    int32_t reserved;                            /* 0                                                      */
} fcn_detout_params;
size_t fcn_detection_output_workspace_bytes(const fcn_detout_params* h_params);
int  fcn_detection_output_f32(const float* loc, const float* conf, const float* priors, const fcn_detout_params* h_params, float* out_rows,
                              int32_t* out_count, void* d_workspace, size_t workspace_bytes, fcn_stream_t s);

/* ---- Region stage of the two-stage detectors (Faster R-CNN / R-FCN: the RPN's two-class softmax, Proposal, ROIPooling, PSROIPooling;
 *      csrc/region.hip).  Float32, inference.  The common contract of the SSD head above holds: one writer lane per output element, no
 *      atomics at all, a second launch on the same inputs gives the same bytes, every refusal is made on the host before the first HIP
 *      call, all launches are capturable, the file is compiled without fused multiply-add contraction.  Blobs are NHWC: a pixel is
 *      `cstride` floats of which the blob's channels start at `coffset`; channels C .. r4(C) - 1 of every top are written as zeros. ---- */
/* The RPN softmax, Reshape(0, 2, -1, 0) -> Softmax(axis 1) -> Reshape(0, 2A, -1, 0) of an (N, 2A, H, W) blob, in one launch: at every
 * pixel and for every a < A the pair (x[a], x[a + A]) is normalised: m = max of the two, e = exp(x - m), y = e / (e_a + e_{a+A}).
 * One lane per (pixel, a).  y may be x. */
int  fcn_pair_softmax_f32(const float* x, float* y, int pixels, int A, int x_cstride, int x_coffset, int y_cstride, int y_coffset, fcn_stream_t s);
/* Proposal (py-faster-rcnn's rpn/proposal_layer.py at TEST settings), one image.  scores: H x W pixels of 2A channels (a < A background,
 * A + a foreground), deltas: H x W pixels of 4A channels (4a .. 4a + 3: dx, dy, dw, dh of anchor a), im_info: 3 floats on the device
 * (height, width, scale).  Candidate i = (y W + x) A + a is anchors[a] shifted by (x, y) * feat_stride.  The order of steps is the contract:
 *   1. decode: w = x2 - x1 + 1, cx = x1 + 0.5 w, pcx = dx w + cx, pw = exp(dw) w, box (pcx - 0.5 pw, .., pcx + 0.5 pw, ..); y likewise.
 *   2. clip x to [0, im_w - 1], y to [0, im_h - 1].
 *   3. a candidate stays iff x2 - x1 + 1 >= min_size * im_scale and the same for y (a NaN score or corner is no candidate).  The corners
 *      are asked for a NaN as step 1 leaves them, before the clip, so the rule holds whatever min_size is, 0 included.  Every other float
 *      is a score: the infinities and the denormals order as floats do, -0 and +0 are one score.
 *   4. order by foreground score descending, TIES BY CANDIDATE INDEX ASCENDING (numpy's argsort()[::-1] leaves them unspecified; this order
 *      is fixed here); the first pre_nms_topn go on.
 *   5. greedy NMS in that order with the +1 extents: area (x2 - x1 + 1)(y2 - y1 + 1), intersection extents max(0, min(x2) - max(x1) + 1),
 *      a later box is suppressed iff inter / (a_i + a_j - inter) > nms_thresh.  nms_thresh is any float but a NaN: at 1 or above nothing is
 *      suppressed, below 0 every later box is, boxes that do not meet included (their overlap is 0).
 *   6. the first post_nms_topn survivors are the rows [0, x1, y1, x2, y2] of rois (and their scores the rows of top_scores, which may be
 *      NULL); their number goes to *out_count; rows at and past the count, and the pad channels 5 .. 7 (1 .. 3), are written as ZEROS on
 *      every call: all post_nms_topn rows are defined.
 * Five launches: decode (a key per candidate: score bits, ~index, or 0 for a dropped one - nothing is compacted), rank (a workgroup per
 * 256 candidates and eighth of the keys counts the keys above its own through LDS tiles), place (the eight counts summed are the place
 * in the order), the suppression bit matrix (a wave per 64 x 64 block), one wave that sweeps it a word at a time and writes the rows.  More than FCN_PROPOSAL_MAX_ANCHORS anchors, H * W * A above FCN_PROPOSAL_MAX_CANDIDATES, min(pre_nms_topn, H * W * A)
 * or post_nms_topn above FCN_PROPOSAL_MAX_PRE_NMS are FCN_E_UNSUPPORTED; a workspace below fcn_proposal_workspace_bytes() FCN_E_ARG, off
 * 16 bytes FCN_E_ALIGN.  The size query returns 0 for parameters the launch would refuse. */
#define FCN_PROPOSAL_MAX_ANCHORS 32
#define FCN_PROPOSAL_MAX_CANDIDATES 65536
#define FCN_PROPOSAL_MAX_PRE_NMS 6144
typedef struct fcn_proposal_params {
    int32_t H, W, A, feat_stride;
    int32_t pre_nms_topn, post_nms_topn;
    float min_size, nms_thresh;
    int32_t score_cstride, score_coffset;        /* floats per pixel of the bottoms, first channel inside a pixel     */
    int32_t delta_cstride, delta_coffset;
    int32_t rois_cstride, rois_coffset;          /* rois_cstride >= rois_coffset + 8                                  */
    int32_t top_score_cstride, top_score_coffset;/* 0, 0 without a scores top; else cstride >= coffset + 4            */
    float anchors[4 * FCN_PROPOSAL_MAX_ANCHORS]; /* x1, y1, x2, y2 of each base anchor                                */
} fcn_proposal_params;
size_t fcn_proposal_workspace_bytes(const fcn_proposal_params* h_params);
int  fcn_proposal_f32(const float* scores, const float* deltas, const float* im_info, const fcn_proposal_params* h_params, float* rois,
                      float* top_scores, int32_t* out_count, void* d_workspace, size_t workspace_bytes, fcn_stream_t s);
/* ROIPooling.  x: N images of H x W pixels; rois: R rows [b, x1, y1, x2, y2] (row stride rois_cstride); y: R images of pooled_h x pooled_w
 * pixels of C channels.  Per roi: start = round(x * spatial_scale) (halves away from zero), roi_w = max(end_w - start_w + 1, 1),
 * bin_w = (float)roi_w / pooled_w; bin (ph, pw) covers rows floor(ph bin_h) + start_h .. ceil((ph + 1) bin_h) + start_h (exclusive), both
 * clipped to [0, H], columns likewise; the value is the maximum over the bin of image b (the first maximum in raster order; a NaN never
 * wins), 0 for an empty bin or an image index outside [0, N).  argmax (NULL, or R * pooled_h * pooled_w * C dense int32 in the top's
 * order): h * W + w of the maximum, -1 for an empty bin.  One wave per (roi, bin), lanes over channels. */
int  fcn_roi_pool_fwd_f32(const float* x, const float* rois, float* y, int32_t* argmax, int N, int H, int W, int C, int x_cstride, int x_coffset,
                          int R, int rois_cstride, int rois_coffset, int pooled_h, int pooled_w, float spatial_scale, int y_cstride, int y_coffset,
                          fcn_stream_t s);
/* PSROIPooling (R-FCN).  x has C = output_dim * group_size^2 channels (anything else is FCN_E_ARG); y: R images of group_size x group_size
 * pixels of output_dim channels.  start_w = round(x1) * spatial_scale, end_w = (round(x2) + 1) * spatial_scale, roi_w = max(end_w - start_w,
 * 0.1), bin_w = roi_w / group_size, wstart = floor(pw bin_w + start_w), wend = ceil((pw + 1) bin_w + start_w), both clipped to [0, W]; rows
 * likewise.  Top channel ct of bin (ph, pw) is the mean of input channel (ct * group_size + ph) * group_size + pw over the bin: the sum
 * in raster order divided by the bin's pixel count; 0 for an empty bin or an image index outside [0, N). */
int  fcn_psroi_pool_fwd_f32(const float* x, const float* rois, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int R,
                            int rois_cstride, int rois_coffset, int output_dim, int group_size, float spatial_scale, int y_cstride, int y_coffset,
                            fcn_stream_t s);

/* ---- data-parallel exchange (new capability; the reference trains with --gpu=0 only, train/train.sh:26):
 *      sum of the flat gradient buffer over all ranks with RCCL on the caller's stream ---- */
int  fcn_comm_unique_id(char* h_id128);                                    /* rank 0: ncclGetUniqueId (128 bytes)   */
int  fcn_comm_init(fcn_comm_t* comm, const char* h_id128, int world, int rank);
int  fcn_comm_allreduce_sum_f32(fcn_comm_t comm, float* buf, size_t count, fcn_stream_t s);
int  fcn_comm_destroy(fcn_comm_t comm);

/* ---- ArgMax (Caffe's ArgMaxLayer over the channel axis), alone and fused behind Interp and / or Softmax (csrc/argmax.hip).  x is a
 *      (pixels, C, x_cstride, x_coffset) NHWC view of float32 or halves; y is ALWAYS float32, as Caffe's top is: top_k channels per pixel
 *      (2 * top_k with FCN_ARGMAX_PAIRS) at y_coffset of y_cstride.  Caffe sorts (value, index) pairs with std::greater: rank 0 is the
 *      largest value, and of equal values the LARGER INDEX comes first.  Only channels x_coffset .. x_coffset + C - 1 are compared: pad
 *      channels and neighbouring windows may be loaded (inside the pixel's stride) and never win.  A NaN never takes a rank.  No atomics:
 *      the same call gives the same bits; every launch can be captured.  Two launch shapes: a lane per pixel over the window's 16-byte
 *      segments (segmentation tails: few channels, many pixels), and a wave per pixel with a fixed butterfly over (value, index) pairs
 *      (classifier rows).  The wave form runs where a pixel's window holds more than FCN_ARGMAX_WAVE_BYTES bytes, and where at least
 *      FCN_ARGMAX_WAVE_MIN_C channels meet at most FCN_ARGMAX_WAVE_PIXELS pixels (every pixel's wave resident at once: 256 CUs x 32).
 *      Contract, checked before the first HIP call: null pointers, non-positive extents, top_k < 1 or > C, a window outside its pixel,
 *      unknown flags or VALUES together with PAIRS FCN_E_ARG; top_k > FCN_ARGMAX_MAX_TOPK FCN_E_UNSUPPORTED; alignment as
 *      fcn_interp_fwd_*: float32 x and y on 4-byte pointers with any stride (16-byte loads where x allows), half x on a 16-byte pointer
 *      with stride and offset in multiples of 8 halves and y on one with multiples of 4 floats, else FCN_E_ALIGN.  Floor: the bytes of x. ---- */
#define FCN_ARGMAX_MAX_TOPK 32
#define FCN_ARGMAX_WAVE_BYTES  512   /* a window above this many bytes (128 floats, 256 halves): a wave per pixel */
#define FCN_ARGMAX_WAVE_PIXELS 8192  /* up to this many pixels ...                                                  */
#define FCN_ARGMAX_WAVE_MIN_C  32    /* ... of at least this many channels: a wave per pixel as well                */
#define FCN_ARGMAX_VALUES  1   /* y holds the k largest values, not their indices (Caffe: axis set + out_max_val) */
#define FCN_ARGMAX_PAIRS   2   /* y holds k indices, then k values (Caffe: no axis + out_max_val) */
#define FCN_ARGMAX_SOFTMAX 4   /* x holds the scores in front of a fused Softmax: values are probabilities, indices unchanged */
int  fcn_argmax_fwd_f32(const float* x, float* y, int pixels, int C, int x_cstride, int x_coffset, int top_k, int y_cstride, int y_coffset,
                        int flags, fcn_stream_t s);
int  fcn_argmax_fwd_f16(const void* x, float* y, int pixels, int C, int x_cstride, int x_coffset, int top_k, int y_cstride, int y_coffset,
                        int flags, fcn_stream_t s);
/* Interp (the geometry and integer cell arithmetic of fcn_interp_fwd_*: cell = num / (n2 - 1), weight = float(num % (n2 - 1)) /
 * float(n2 - 1), num = o (n1 - 1); the blend in float32 without contraction) and ArgMax in one pass, a lane per output pixel: the
 * resampled map is never written.  top_k == 1: y takes one float per pixel (index, or value with VALUES), or two (PAIRS: index, value).
 * Under FCN_ARGMAX_SOFTMAX the value is the probability 1 / sum exp(v - max) over the blended scores.  Contract of fcn_interp_fwd_*
 * (the half form as with out_f32 1) plus the flags'; 2^31 output pixels or more FCN_E_UNSUPPORTED. */
int  fcn_interp_argmax_fwd_f32(const float* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                               int OH, int OW, int y_cstride, int y_coffset, int flags, fcn_stream_t s);
int  fcn_interp_argmax_fwd_f16(const void* x, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int pad_beg, int pad_end,
                               int OH, int OW, int y_cstride, int y_coffset, int flags, fcn_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* FCNHIP_H_ */
