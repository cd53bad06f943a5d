// The region stage of the two-stage detectors for gfx950: the RPN's two-class softmax, Proposal (decode, clip, size filter, order,
// greedy NMS, the rows and their count), ROIPooling and PSROIPooling.  include/fcnhip.h states the contract.
//
// Every output element has one writer lane and there is no atomic in this file: a candidate's key lies at the candidate's own index
// (a filtered candidate has the key 0, below every real key), so nothing has to be compacted.  Steps that hand data from one workgroup
// to another are separate launches.  The same inputs give the same bytes.
#include "common.h"

#include <float.h>

using namespace fcn;

namespace {

typedef float V4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

inline bool aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }
inline long long r4ll(long long v) { return (v + 3) / 4 * 4; }
inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// ---------------------------------------------------------------------------------------------------------------- pair softmax
__global__ __launch_bounds__(256) void pair_softmax_kernel(const float* x, float* y, long long pixels, int A, int x_cstride, int x_coffset,
                                                           int y_cstride, int y_coffset) {
    const long long total = pixels * A;
    const int C = 2 * A, C4 = (C + 3) / 4 * 4;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long pix = t / A;
        const int a = (int)(t - pix * A);
        const float* xp = x + (size_t)pix * x_cstride + x_coffset;
        float* yp = y + (size_t)pix * y_cstride + y_coffset;
        const float b = xp[a], f = xp[a + A];
        const float m = fmaxf(b, f);
        const float eb = expf(b - m), ef = expf(f - m);
        const float sum = eb + ef;
        yp[a] = eb / sum;
        yp[a + A] = ef / sum;
        if (a == 0)
            for (int c = C; c < C4; ++c) yp[c] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- proposal
constexpr int RANK_SLICES = 8;       // the ranking pass splits the keys it counts over this many workgroups per 256 candidates
constexpr int RANK_TILE = 2048;      // keys per LDS tile of the ranking pass (16 KB)

struct PropPlan {
    fcn_proposal_params p;
    int M;                       // candidates: H * W * A
    int K;                       // boxes that go into the NMS at most: min(pre_nms_topn, M)
    int words;                   // 64-bit words of a row of the suppression matrix: ceil(K / 64)
    // workspace, byte offsets (each a multiple of 16)
    size_t off_boxes;            // M float4: the decoded, clipped boxes
    size_t off_keys;             // M u64: (score bits, ~index), or 0 for a candidate the size filter dropped
    size_t off_sbox;             // K float4: the boxes in order
    size_t off_sidx;             // K int: the candidates in order, -1 past the last one
    size_t off_sscore;           // K float: their scores
    size_t off_mask;             // K * words u64: bit j of row i: box i suppresses the later box j
    size_t off_part;             // RANK_SLICES * M int: how many keys of one slice of the candidates are greater than a candidate's
    size_t bytes;
};

int prop_plan(const fcn_proposal_params* hp, PropPlan* d) {
    FCN_REQUIRE(hp, FCN_E_ARG, "proposal: null parameters");
    const fcn_proposal_params& p = *hp;
    FCN_REQUIRE(p.H > 0 && p.W > 0 && p.A > 0 && p.pre_nms_topn > 0 && p.post_nms_topn > 0, FCN_E_ARG,
                "proposal: non-positive extent (H %d, W %d, anchors %d, pre_nms_topn %d, post_nms_topn %d)", p.H, p.W, p.A, p.pre_nms_topn,
                p.post_nms_topn);
    FCN_REQUIRE(p.A <= FCN_PROPOSAL_MAX_ANCHORS, FCN_E_UNSUPPORTED, "proposal: %d anchors exceed %d", p.A, FCN_PROPOSAL_MAX_ANCHORS);
    const long long M = (long long)p.H * p.W * p.A;
    FCN_REQUIRE(M <= FCN_PROPOSAL_MAX_CANDIDATES, FCN_E_UNSUPPORTED, "proposal: %lld candidates (%d x %d x %d anchors) exceed %d", M, p.H, p.W,
                p.A, FCN_PROPOSAL_MAX_CANDIDATES);
    const long long K = p.pre_nms_topn < M ? p.pre_nms_topn : M;
    FCN_REQUIRE(K <= FCN_PROPOSAL_MAX_PRE_NMS, FCN_E_UNSUPPORTED, "proposal: %lld boxes into the NMS (pre_nms_topn %d over %lld candidates) exceed %d",
                K, p.pre_nms_topn, M, FCN_PROPOSAL_MAX_PRE_NMS);
    FCN_REQUIRE(p.post_nms_topn <= FCN_PROPOSAL_MAX_PRE_NMS, FCN_E_UNSUPPORTED, "proposal: post_nms_topn %d exceeds %d", p.post_nms_topn,
                FCN_PROPOSAL_MAX_PRE_NMS);
    FCN_REQUIRE(p.feat_stride > 0, FCN_E_ARG, "proposal: feat_stride %d", p.feat_stride);
    FCN_REQUIRE(p.min_size >= 0.f && p.nms_thresh == p.nms_thresh, FCN_E_ARG, "proposal: min_size is negative or a threshold is NaN");
    FCN_REQUIRE(p.score_coffset >= 0 && p.delta_coffset >= 0 && (long long)p.score_cstride >= p.score_coffset + 2ll * p.A &&
                    (long long)p.delta_cstride >= p.delta_coffset + 4ll * p.A, FCN_E_ARG, "proposal: a bottom's channels leave its pixel");
    FCN_REQUIRE(p.rois_coffset >= 0 && p.rois_cstride >= p.rois_coffset + 8, FCN_E_ARG,
                "proposal: the rois need room for 8 channels (5 and their pad), have %d + %d", p.rois_coffset, p.rois_cstride);
    FCN_REQUIRE(p.top_score_coffset >= 0 && (p.top_score_cstride == 0 || p.top_score_cstride >= p.top_score_coffset + 4), FCN_E_ARG,
                "proposal: the scores top needs room for 4 channels (1 and its pad)");
    const long long two31 = 1ll << 31;
    FCN_REQUIRE((long long)p.H * p.W * p.score_cstride < two31 && (long long)p.H * p.W * p.delta_cstride < two31 &&
                    (long long)p.post_nms_topn * p.rois_cstride < two31 && (long long)p.post_nms_topn * p.top_score_cstride < two31,
                FCN_E_UNSUPPORTED, "proposal: views past 2^31 elements");
    d->p = p;
    d->M = (int)M;
    d->K = (int)K;
    d->words = (int)((K + 63) / 64);
    size_t o = 0;
    d->off_boxes = o;   o += up16((size_t)M * 16);
    d->off_keys = o;    o += up16((size_t)M * 8);
    d->off_sbox = o;    o += up16((size_t)K * 16);
    d->off_sidx = o;    o += up16((size_t)K * 4);
    d->off_sscore = o;  o += up16((size_t)K * 4);
    d->off_mask = o;    o += up16((size_t)K * d->words * 8);
    d->off_part = o;    o += up16((size_t)RANK_SLICES * M * 4);
    d->bytes = o;
    return 0;
}

// a float as an unsigned whose order is the float's (no NaN arrives here: a NaN score is no candidate)
__device__ inline unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f + 0.f);      // (-0 + 0 = +0: the two zeros are one score)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// steps 2 to 4 for every candidate; marks the order's K places as empty
__global__ __launch_bounds__(256) void prop_decode_kernel(const float* __restrict__ scores, const float* __restrict__ deltas,
                                                          const float* __restrict__ im_info, V4* __restrict__ boxes, u64* __restrict__ keys,
                                                          int* __restrict__ sidx, PropPlan d) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < d.K) sidx[t] = -1;
    if (t >= d.M) return;
    const int A = d.p.A, W = d.p.W;
    const int pix = t / A, a = t - pix * A;
    const int y = pix / W, x = pix - y * W;
    const float im_h = im_info[0], im_w = im_info[1], im_scale = im_info[2];
    const float sx = (float)(x * d.p.feat_stride), sy = (float)(y * d.p.feat_stride);
    const float ax1 = d.p.anchors[4 * a] + sx, ay1 = d.p.anchors[4 * a + 1] + sy;
    const float ax2 = d.p.anchors[4 * a + 2] + sx, ay2 = d.p.anchors[4 * a + 3] + sy;
    const float* dl = deltas + (size_t)pix * d.p.delta_cstride + d.p.delta_coffset + 4 * a;
    const float w = ax2 - ax1 + 1.f, h = ay2 - ay1 + 1.f;
    const float cx = ax1 + 0.5f * w, cy = ay1 + 0.5f * h;
    const float pcx = dl[0] * w + cx, pcy = dl[1] * h + cy;
    const float pw = expf(dl[2]) * w, ph = expf(dl[3]) * h;
    const float x1 = pcx - 0.5f * pw, y1 = pcy - 0.5f * ph, x2 = pcx + 0.5f * pw, y2 = pcy + 0.5f * ph;
    V4 b;
    b.x = fminf(fmaxf(x1, 0.f), im_w - 1.f);
    b.y = fminf(fmaxf(y1, 0.f), im_h - 1.f);
    b.z = fminf(fmaxf(x2, 0.f), im_w - 1.f);
    b.w = fminf(fmaxf(y2, 0.f), im_h - 1.f);
    boxes[t] = b;
    const float sc = scores[(size_t)pix * d.p.score_cstride + d.p.score_coffset + A + a];
    const float ms = d.p.min_size * im_scale;
    // fmaxf / fminf return their other operand for a NaN: the clip turns a NaN corner into 0, a box one pixel wide that a min_size of
    // 1 or less lets through.  So the corners are asked before the clip.
    const bool number = x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2 && sc == sc;
    const bool ok = number && (b.z - b.x + 1.f >= ms) && (b.w - b.y + 1.f >= ms);
    keys[t] = ok ? (((u64)ordered_bits(sc) << 32) | (u64)(0xFFFFFFFFu - (unsigned)t)) : 0ull;
}

// step 5, first half: how many keys are greater than a candidate's own, counted slice by slice: workgroup (x, y) streams slice y of the
// keys through LDS for the 256 candidates of block x.  The slices' counts are summed by the next launch: no atomic.
__global__ __launch_bounds__(256) void prop_rank_kernel(const u64* __restrict__ keys, int* __restrict__ part, PropPlan d) {
    __shared__ u64 tile[RANK_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const u64 mine = i < d.M ? keys[i] : 0ull;
    const bool valid = mine != 0ull;
    if (!__syncthreads_or(valid ? 1 : 0)) return;      // (the place pass never reads the counts of a dropped candidate)
    const int per = (d.M + RANK_SLICES - 1) / RANK_SLICES;
    const int lo = blockIdx.y * per, hi = min(d.M, lo + per);
    int rank = 0;
    for (int base = lo; base < hi; base += RANK_TILE) {
        const int cnt = min(RANK_TILE, hi - base);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += 256) tile[j] = keys[base + j];
        __syncthreads();
        if (valid) {
            int r = 0;
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) r += tile[j] > mine ? 1 : 0;
            rank += r;
        }
    }
    if (valid) part[(size_t)blockIdx.y * d.M + i] = rank;
}

// step 5, second half: the sum of a candidate's counts is its place in the order; the first K places take box, index and score
__global__ __launch_bounds__(256) void prop_place_kernel(const float* __restrict__ scores, const V4* __restrict__ boxes, const u64* __restrict__ keys,
                                                         const int* __restrict__ part, V4* __restrict__ sbox, int* __restrict__ sidx,
                                                         float* __restrict__ sscore, PropPlan d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.M || keys[i] == 0ull) return;
    int rank = 0;
    for (int s = 0; s < RANK_SLICES; ++s) rank += part[(size_t)s * d.M + i];
    if (rank < d.K) {
        const int pix = i / d.p.A, a = i - pix * d.p.A;
        sbox[rank] = boxes[i];
        sidx[rank] = i;
        sscore[rank] = scores[(size_t)pix * d.p.score_cstride + d.p.score_coffset + d.p.A + a];
    }
}

__device__ inline float prop_area(const V4 b) { return (b.z - b.x + 1.f) * (b.w - b.y + 1.f); }

// step 6, first half: one wave per 64 x 64 block of the suppression matrix; lane l owns row 64 * blockIdx.y + l.
// Bit j of word blockIdx.x of row i is set iff j > i, both places hold a box and their overlap exceeds the threshold.
__global__ __launch_bounds__(64) void prop_mask_kernel(const V4* __restrict__ sbox, const int* __restrict__ sidx, u64* __restrict__ mask, PropPlan d) {
    __shared__ V4 s_col[64];
    __shared__ int s_ok[64];
    const int lane = threadIdx.x;
    const int cb = blockIdx.x, rb = blockIdx.y;
    const int i = rb * 64 + lane, jc = cb * 64 + lane;
    if (cb < rb) {      // below the diagonal nothing is later
        if (i < d.K) mask[(size_t)i * d.words + cb] = 0ull;
        return;
    }
    const bool col_ok = jc < d.K && sidx[jc] >= 0;
    s_ok[lane] = col_ok ? 1 : 0;
    if (col_ok) s_col[lane] = sbox[jc];
    __syncthreads();
    if (i >= d.K) return;
    u64 bits = 0ull;
    if (sidx[i] >= 0) {
        const V4 bi = sbox[i];
        const float ai = prop_area(bi);
        for (int j = 0; j < 64; ++j) {
            if (!s_ok[j] || cb * 64 + j <= i) continue;
            const V4 bj = s_col[j];
            const float iw = fmaxf(0.f, fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x) + 1.f);
            const float ih = fmaxf(0.f, fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y) + 1.f);
            const float inter = iw * ih;
            const float ov = inter / (ai + prop_area(bj) - inter);
            if (ov > d.p.nms_thresh) bits |= 1ull << j;
        }
    }
    mask[(size_t)i * d.words + cb] = bits;
}

static_assert((FCN_PROPOSAL_MAX_PRE_NMS + 63) / 64 <= 128, "the sweep keeps the set of suppressed places in two words a lane");

// step 6, second half, and step 7: one wave walks the order 64 places (one word) at a time.  The set of suppressed places lives in
// registers - lane l holds words l and l + 64 - and within a word only the 64 x 64 diagonal block of the matrix decides, so a word costs
// one load of that block (lane l: box 64 w + l), a chain of at most 64 register steps, and one batch of independent row loads for the
// boxes it kept: two memory round trips a word, not one per kept box.  Then the rows.
__global__ __launch_bounds__(64) void prop_sweep_kernel(const V4* __restrict__ sbox, const int* __restrict__ sidx, const float* __restrict__ sscore,
                                                        const u64* __restrict__ mask, float* __restrict__ rois, float* __restrict__ top_scores,
                                                        int* __restrict__ out_count, PropPlan d) {
    __shared__ int s_kept[FCN_PROPOSAL_MAX_PRE_NMS];
    const int lane = threadIdx.x;
    const int R = d.p.post_nms_topn, words = d.words;
    // the places that hold a box are the first k of the order
    int k = 0;
    for (int i = lane; i < d.K; i += 64) k += sidx[i] >= 0 ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) k += __shfl_xor(k, off, 64);
    u64 r0 = 0ull, r1 = 0ull;
    int nkept = 0;
    for (int w = 0; w * 64 < k && nkept < R; ++w) {      // (every condition below is the same in all lanes)
        const int left = k - w * 64, mine = w * 64 + lane;
        const u64 valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        const u64 diag = mine < k ? mask[(size_t)mine * words + w] : 0ull;
        u64 rem = __shfl(w < 64 ? r0 : r1, w & 63, 64);
        u64 avail = ~rem & valid, keptbits = 0ull;
        const int before = nkept;
        while (avail && nkept < R) {      // the lowest place nothing has suppressed is kept and suppresses within the word
            const int b = __ffsll((long long)avail) - 1;
            keptbits |= 1ull << b;
            ++nkept;
            rem |= __shfl(diag, b, 64);
            avail = b == 63 ? 0ull : (~rem & valid & ~((2ull << b) - 1ull));
        }
        if ((keptbits >> lane) & 1ull) s_kept[before + __popcll(keptbits & ((1ull << lane) - 1ull))] = mine;
        // the kept boxes' rows into the set, four rows a round so that their loads are in flight together
        u64 bits = keptbits;
        while (bits) {
            u64 a0 = 0ull, a1 = 0ull;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = bits ? __ffsll((long long)bits) - 1 : -1;
                bits &= bits - 1ull;      // (0 stays 0)
                const u64* row = mask + (size_t)(w * 64 + (b < 0 ? 0 : b)) * words;
                a0 |= (b >= 0 && lane < words) ? row[lane] : 0ull;
                a1 |= (b >= 0 && lane + 64 < words) ? row[lane + 64] : 0ull;
            }
            r0 |= a0;
            r1 |= a1;
        }
    }
    __syncthreads();
    if (lane == 0) *out_count = nkept;
    for (int r = lane; r < R; r += 64) {
        float* row = rois + (size_t)r * d.p.rois_cstride + d.p.rois_coffset;
        V4 b = {0.f, 0.f, 0.f, 0.f};
        float sc = 0.f;
        if (r < nkept) {
            b = sbox[s_kept[r]];
            sc = sscore[s_kept[r]];
        }
        row[0] = 0.f;
        row[1] = b.x;
        row[2] = b.y;
        row[3] = b.z;
        row[4] = b.w;
        row[5] = 0.f;
        row[6] = 0.f;
        row[7] = 0.f;
        if (top_scores) {
            float* srow = top_scores + (size_t)r * d.p.top_score_cstride + d.p.top_score_coffset;
            srow[0] = sc;
            srow[1] = 0.f;
            srow[2] = 0.f;
            srow[3] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- poolings
struct PoolArgs {
    int N, H, W, C, x_cstride, x_coffset;
    int R, rois_cstride, rois_coffset;
    int PH, PW, y_cstride, y_coffset;
    float scale;
};

// a float to an int, saturated (a NaN becomes the lower bound): the bounds lie far outside any feature map and inside int's range
__device__ inline int sat_int(float v) { return (int)fminf(fmaxf(v, -1.0e8f), 1.0e8f); }
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one wave per (roi, bin), four per workgroup; lanes over channels
__global__ __launch_bounds__(256) void roi_pool_kernel(const float* __restrict__ x, const float* __restrict__ rois, float* __restrict__ y,
                                                       int* __restrict__ argmax, PoolArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long bins = (long long)a.R * a.PH * a.PW;
    const int C4 = (a.C + 3) / 4 * 4;
    for (long long bin = (long long)blockIdx.x * 4 + wave; bin < bins; bin += (long long)gridDim.x * 4) {
        const int r = (int)(bin / (a.PH * a.PW)), q = (int)(bin - (long long)r * a.PH * a.PW);
        const int ph = q / a.PW, pw = q - ph * a.PW;
        const float* roi = rois + (size_t)r * a.rois_cstride + a.rois_coffset;
        const int n = sat_int(roi[0]);
        const int sw = sat_int(roundf(roi[1] * a.scale)), sh = sat_int(roundf(roi[2] * a.scale));
        const int ew = sat_int(roundf(roi[3] * a.scale)), eh = sat_int(roundf(roi[4] * a.scale));
        const int roi_w = max(ew - sw + 1, 1), roi_h = max(eh - sh + 1, 1);
        const float bin_h = (float)roi_h / (float)a.PH, bin_w = (float)roi_w / (float)a.PW;
        const int hs = clampi(sat_int(floorf((float)ph * bin_h)) + sh, 0, a.H), he = clampi(sat_int(ceilf((float)(ph + 1) * bin_h)) + sh, 0, a.H);
        const int ws = clampi(sat_int(floorf((float)pw * bin_w)) + sw, 0, a.W), we = clampi(sat_int(ceilf((float)(pw + 1) * bin_w)) + sw, 0, a.W);
        const bool empty = he <= hs || we <= ws || n < 0 || n >= a.N;
        float* yp = y + (size_t)bin * a.y_cstride + a.y_coffset;
        int* ap = argmax ? argmax + (size_t)bin * a.C : nullptr;
        for (int c = lane; c < C4; c += 64) {
            if (c >= a.C) {
                yp[c] = 0.f;
                continue;
            }
            float m = empty ? 0.f : -FLT_MAX;
            int at = -1;
            if (!empty) {
                const float* xp = x + (size_t)n * a.H * a.W * a.x_cstride + a.x_coffset + c;
                for (int h = hs; h < he; ++h)
                    for (int w = ws; w < we; ++w) {
                        const float v = xp[(size_t)(h * a.W + w) * a.x_cstride];
                        if (v > m) {
                            m = v;
                            at = h * a.W + w;
                        }
                    }
            }
            yp[c] = m;
            if (ap) ap[c] = at;
        }
    }
}

// one wave per (roi, bin), four per workgroup; lanes over the top's channels
__global__ __launch_bounds__(256) void psroi_pool_kernel(const float* __restrict__ x, const float* __restrict__ rois, float* __restrict__ y,
                                                         PoolArgs a, int OD) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = a.PH;
    const long long bins = (long long)a.R * G * G;
    const int C4 = (OD + 3) / 4 * 4;
    for (long long bin = (long long)blockIdx.x * 4 + wave; bin < bins; bin += (long long)gridDim.x * 4) {
        const int r = (int)(bin / (G * G)), q = (int)(bin - (long long)r * G * G);
        const int ph = q / G, pw = q - ph * G;
        const float* roi = rois + (size_t)r * a.rois_cstride + a.rois_coffset;
        const int n = sat_int(roi[0]);
        const float sw = roundf(roi[1]) * a.scale, sh = roundf(roi[2]) * a.scale;
        const float ew = (roundf(roi[3]) + 1.f) * a.scale, eh = (roundf(roi[4]) + 1.f) * a.scale;
        const float roi_w = fmaxf(ew - sw, 0.1f), roi_h = fmaxf(eh - sh, 0.1f);
        const float bin_h = roi_h / (float)G, bin_w = roi_w / (float)G;
        const int hs = clampi(sat_int(floorf((float)ph * bin_h + sh)), 0, a.H), he = clampi(sat_int(ceilf((float)(ph + 1) * bin_h + sh)), 0, a.H);
        const int ws = clampi(sat_int(floorf((float)pw * bin_w + sw)), 0, a.W), we = clampi(sat_int(ceilf((float)(pw + 1) * bin_w + sw)), 0, a.W);
        const bool empty = he <= hs || we <= ws || n < 0 || n >= a.N;
        const float area = (float)((he - hs) * (we - ws));
        float* yp = y + (size_t)bin * a.y_cstride + a.y_coffset;
        for (int ct = lane; ct < C4; ct += 64) {
            float sum = 0.f;
            if (ct < OD && !empty) {
                const float* xp = x + (size_t)n * a.H * a.W * a.x_cstride + a.x_coffset + (ct * G + ph) * G + pw;
                for (int h = hs; h < he; ++h)
                    for (int w = ws; w < we; ++w) sum = sum + xp[(size_t)(h * a.W + w) * a.x_cstride];
                sum = sum / area;
            }
            yp[ct] = sum;
        }
    }
}

int pool_args(const char* who, const float* x, const float* rois, const float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int R,
              int rois_cstride, int rois_coffset, int PH, int PW, int topC, float scale, int y_cstride, int y_coffset, PoolArgs* a) {
    FCN_REQUIRE(x && rois && y, FCN_E_ARG, "%s: null pointer", who);
    FCN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && R > 0, FCN_E_ARG, "%s: non-positive extent (N %d, H %d, W %d, C %d, rois %d)", who, N, H, W, C, R);
    FCN_REQUIRE(PH >= 1 && PW >= 1, FCN_E_ARG, "%s: pooled grid %d x %d", who, PH, PW);
    FCN_REQUIRE(scale > 0.f, FCN_E_ARG, "%s: spatial_scale %g is not positive", who, (double)scale);
    FCN_REQUIRE(x_coffset >= 0 && x_cstride >= x_coffset + C, FCN_E_ARG, "%s: channels %d + %d leave the pixel of %d", who, x_coffset, C, x_cstride);
    FCN_REQUIRE(rois_coffset >= 0 && rois_cstride >= rois_coffset + 5, FCN_E_ARG, "%s: a roi row of %d + 5 floats leaves its stride %d", who,
                rois_coffset, rois_cstride);
    FCN_REQUIRE(y_coffset >= 0 && (long long)y_cstride >= y_coffset + r4ll(topC), FCN_E_ARG, "%s: the top needs room for %lld channels", who,
                r4ll(topC));
    FCN_REQUIRE(aligned(x, 4) && aligned(rois, 4) && aligned(y, 4), FCN_E_ALIGN, "%s: a pointer off 4 bytes", who);
    const long long two31 = 1ll << 31;
    FCN_REQUIRE((long long)N * H * W * x_cstride < two31 && (long long)R * PH * PW * y_cstride < two31 && (long long)R * rois_cstride < two31 &&
                    (long long)R * PH * PW * C < two31, FCN_E_UNSUPPORTED, "%s: views past 2^31 elements", who);
    a->N = N, a->H = H, a->W = W, a->C = C, a->x_cstride = x_cstride, a->x_coffset = x_coffset;
    a->R = R, a->rois_cstride = rois_cstride, a->rois_coffset = rois_coffset;
    a->PH = PH, a->PW = PW, a->y_cstride = y_cstride, a->y_coffset = y_coffset, a->scale = scale;
    return 0;
}

}  // namespace

extern "C" {

int fcn_pair_softmax_f32(const float* x, float* y, int pixels, int A, int x_cstride, int x_coffset, int y_cstride, int y_coffset, fcn_stream_t s) {
    FCN_REQUIRE(x && y && pixels > 0 && A > 0, FCN_E_ARG, "pair_softmax: null pointer or non-positive extent");
    FCN_REQUIRE(x_coffset >= 0 && y_coffset >= 0 && (long long)x_cstride >= x_coffset + 2ll * A && (long long)y_cstride >= y_coffset + r4ll(2ll * A),
                FCN_E_ARG, "pair_softmax: slice out of range (the top needs room for %lld channels)", r4ll(2ll * A));
    FCN_REQUIRE(aligned(x, 4) && aligned(y, 4), FCN_E_ALIGN, "pair_softmax: a pointer off 4 bytes");
    FCN_REQUIRE((long long)pixels * x_cstride < (1ll << 31) && (long long)pixels * y_cstride < (1ll << 31), FCN_E_UNSUPPORTED,
                "pair_softmax: views past 2^31 elements");
    hipLaunchKernelGGL(pair_softmax_kernel, dim3(stream_grid((long long)pixels * A, 256)), dim3(256), 0, as_stream(s), x, y, (long long)pixels, A,
                       x_cstride, x_coffset, y_cstride, y_coffset);
    FCN_LAUNCH_CHECK("pair_softmax");
    return 0;
}

size_t fcn_proposal_workspace_bytes(const fcn_proposal_params* h_params) {
    PropPlan d;
    if (prop_plan(h_params, &d)) return 0;
    return d.bytes;
}

int fcn_proposal_f32(const float* scores, const float* deltas, const float* im_info, const fcn_proposal_params* h_params, float* rois,
                     float* top_scores, int32_t* out_count, void* d_workspace, size_t workspace_bytes, fcn_stream_t s) {
    PropPlan d;
    if (int rc = prop_plan(h_params, &d)) return rc;
    FCN_REQUIRE(scores && deltas && im_info && rois && out_count && d_workspace, FCN_E_ARG, "proposal: null pointer");
    FCN_REQUIRE(!top_scores || d.p.top_score_cstride >= d.p.top_score_coffset + 4, FCN_E_ARG, "proposal: a scores top without a stride");
    FCN_REQUIRE(workspace_bytes >= d.bytes, FCN_E_ARG, "proposal: workspace of %zu bytes, %zu needed", workspace_bytes, d.bytes);
    FCN_REQUIRE(aligned(d_workspace, 16), FCN_E_ALIGN, "proposal: workspace off 16 bytes");
    FCN_REQUIRE(aligned(scores, 4) && aligned(deltas, 4) && aligned(im_info, 4) && aligned(rois, 4) && aligned(top_scores, 4) && aligned(out_count, 4),
                FCN_E_ALIGN, "proposal: a pointer off 4 bytes");
    char* ws = static_cast<char*>(d_workspace);
    V4* boxes = reinterpret_cast<V4*>(ws + d.off_boxes);
    u64* keys = reinterpret_cast<u64*>(ws + d.off_keys);
    V4* sbox = reinterpret_cast<V4*>(ws + d.off_sbox);
    int* sidx = reinterpret_cast<int*>(ws + d.off_sidx);
    float* sscore = reinterpret_cast<float*>(ws + d.off_sscore);
    u64* mask = reinterpret_cast<u64*>(ws + d.off_mask);
    int* part = reinterpret_cast<int*>(ws + d.off_part);
    hipStream_t st = as_stream(s);
    const int blocks = cdiv(d.M, 256);
    hipLaunchKernelGGL(prop_decode_kernel, dim3(blocks), dim3(256), 0, st, scores, deltas, im_info, boxes, keys, sidx, d);
    FCN_LAUNCH_CHECK("proposal decode");
    hipLaunchKernelGGL(prop_rank_kernel, dim3(blocks, RANK_SLICES), dim3(256), 0, st, keys, part, d);
    FCN_LAUNCH_CHECK("proposal rank");
    hipLaunchKernelGGL(prop_place_kernel, dim3(blocks), dim3(256), 0, st, scores, boxes, keys, part, sbox, sidx, sscore, d);
    FCN_LAUNCH_CHECK("proposal place");
    hipLaunchKernelGGL(prop_mask_kernel, dim3(d.words, d.words), dim3(64), 0, st, sbox, sidx, mask, d);
    FCN_LAUNCH_CHECK("proposal mask");
    hipLaunchKernelGGL(prop_sweep_kernel, dim3(1), dim3(64), 0, st, sbox, sidx, sscore, mask, rois, top_scores, out_count, d);
    FCN_LAUNCH_CHECK("proposal sweep");
    return 0;
}

int fcn_roi_pool_fwd_f32(const float* x, const float* rois, float* y, int32_t* argmax, int N, int H, int W, int C, int x_cstride, int x_coffset,
                         int R, int rois_cstride, int rois_coffset, int pooled_h, int pooled_w, float spatial_scale, int y_cstride, int y_coffset,
                         fcn_stream_t s) {
    PoolArgs a;
    if (int rc = pool_args("roi_pool", x, rois, y, N, H, W, C, x_cstride, x_coffset, R, rois_cstride, rois_coffset, pooled_h, pooled_w, C,
                           spatial_scale, y_cstride, y_coffset, &a))
        return rc;
    FCN_REQUIRE(aligned(argmax, 4), FCN_E_ALIGN, "roi_pool: argmax off 4 bytes");
    hipLaunchKernelGGL(roi_pool_kernel, dim3(stream_grid((long long)R * pooled_h * pooled_w, 4)), dim3(256), 0, as_stream(s), x, rois, y, argmax, a);
    FCN_LAUNCH_CHECK("roi_pool");
    return 0;
}

int fcn_psroi_pool_fwd_f32(const float* x, const float* rois, float* y, int N, int H, int W, int C, int x_cstride, int x_coffset, int R,
                           int rois_cstride, int rois_coffset, int output_dim, int group_size, float spatial_scale, int y_cstride, int y_coffset,
                           fcn_stream_t s) {
    FCN_REQUIRE(output_dim > 0 && group_size >= 1, FCN_E_ARG, "psroi_pool: output_dim %d, group_size %d", output_dim, group_size);
    FCN_REQUIRE((long long)output_dim * group_size * group_size == C, FCN_E_ARG, "psroi_pool: %d channels, output_dim %d x group_size %d^2 needs %lld", C,
                output_dim, group_size, (long long)output_dim * group_size * group_size);
    PoolArgs a;
    if (int rc = pool_args("psroi_pool", x, rois, y, N, H, W, C, x_cstride, x_coffset, R, rois_cstride, rois_coffset, group_size, group_size, output_dim,
                           spatial_scale, y_cstride, y_coffset, &a))
        return rc;
    hipLaunchKernelGGL(psroi_pool_kernel, dim3(stream_grid((long long)R * group_size * group_size, 4)), dim3(256), 0, as_stream(s), x, rois, y, a,
                       output_dim);
    FCN_LAUNCH_CHECK("psroi_pool");
    return 0;
}

}  // extern "C"
