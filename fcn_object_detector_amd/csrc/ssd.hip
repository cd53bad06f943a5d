// The SSD detection head for gfx950: the gather that stands for Permute + Flatten + Concat, Normalize, and DetectionOutput
// (decode, per-class selection and greedy NMS, the per-image cut, the rows).  include/fcnhip.h states the contract.
//
// Every output element has one writer lane and no float is ever accumulated through an atomic, so the same inputs give the same
// bytes.  The one atomic below is an integer slot counter in LDS: it decides where a candidate's key lies in the workspace, never
// what comes out - the keys are distinct (the prior index is part of them) and every later step ranks them by value.
#include "common.h"

using namespace fcn;

namespace {

typedef float V4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

inline bool aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }
inline long long r4ll(long long v) { return (v + 3) / 4 * 4; }

// ---------------------------------------------------------------------------------------------------------------- gather
struct GatherArgs {
    fcn_ssd_head h[FCN_SSD_MAX_HEADS];
};

// grid: (blocks over one image of the largest head, head, image).  vec_mask bit i: head i moves 16 bytes per lane.
__global__ __launch_bounds__(256) void ssd_gather_kernel(float* __restrict__ dst, int dst_rstride, unsigned vec_mask, GatherArgs a) {
    const fcn_ssd_head h = a.h[blockIdx.y];
    const unsigned n = blockIdx.z;
    const float* __restrict__ src = h.src + ((size_t)n * h.pixels) * h.cstride + h.coffset;
    float* __restrict__ d = dst + (size_t)n * dst_rstride + h.dst_col;
    const unsigned C = (unsigned)h.C, cs = (unsigned)h.cstride;
    if ((vec_mask >> blockIdx.y) & 1u) {
        const unsigned per = C / 4, total = (unsigned)h.pixels * per;
        for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
            const unsigned p = t / per, c = (t - p * per) * 4;
            *reinterpret_cast<V4*>(d + (size_t)p * C + c) = *reinterpret_cast<const V4*>(src + (size_t)p * cs + c);
        }
    } else {
        const unsigned total = (unsigned)h.pixels * C;
        for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
            const unsigned p = t / C, c = t - p * C;
            d[t] = src[(size_t)p * cs + c];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- normalize
// one wave per pixel, four pixels per workgroup
__global__ __launch_bounds__(256) void normalize_kernel(const float* x, float* y, const float* __restrict__ scale,
                                                        int pixels, int C, int x_cstride, int x_coffset, int y_cstride, int y_coffset,
                                                        int shared, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = (C + 3) / 4 * 4;
    for (long long pix = (long long)blockIdx.x * 4 + wave; pix < pixels; pix += (long long)gridDim.x * 4) {
        const float* xp = x + (size_t)pix * x_cstride + x_coffset;
        float* yp = y + (size_t)pix * y_cstride + y_coffset;
        float sum = 0.f;
        for (int c = lane; c < C; c += 64) sum = sum + xp[c] * xp[c];
        for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_xor(sum, off, 64);
        const float norm = sqrtf(sum + eps);
        for (int c = lane; c < C4; c += 64) yp[c] = c < C ? (xp[c] / norm) * scale[shared ? 0 : c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- detection output
struct DetPlan {
    fcn_detout_params p;
    int kmax;                    // candidates per (image, class) that go into the NMS: min(top_k, P), or P
    // workspace, byte offsets (each a multiple of 16)
    size_t off_boxes;            // N * P float4: the decoded boxes
    size_t off_keys;             // N * classes * P u64: candidate keys of one (image, class), in no particular order
    size_t off_kept;             // N * classes * kmax int: prior indices that survive the NMS, in NMS order
    size_t off_kept_n;           // N * classes int: how many
    size_t off_ckey;             // N * classes * kmax u64: per image, the survivors' keys (score bits, ~(label * P + prior)) in row order
    size_t off_centry;           // N * classes * kmax int: per image, the survivors' label * kmax + position, in row order
    size_t off_flag;             // N * classes * kmax int: 1 where the survivor passes the keep_top_k cut
    size_t off_total;            // N int: survivors per image before the cut
    size_t off_img_n;            // N int: rows per image
    size_t off_cpref;            // N * classes int: per image, where each class's survivors start in row order
    size_t bytes;
};

inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// the checks of the size query and the launch; returns 0 and fills `d`, or the code (the text is set)
int det_plan(const fcn_detout_params* hp, DetPlan* d) {
    FCN_REQUIRE(hp, FCN_E_ARG, "detection_output: null parameters");
    const fcn_detout_params& p = *hp;
    FCN_REQUIRE(p.N > 0 && p.P > 0 && p.num_classes > 0, FCN_E_ARG, "detection_output: non-positive extent (N %d, P %d, classes %d)", p.N, p.P,
                p.num_classes);
    FCN_REQUIRE(p.background >= -1 && p.background < p.num_classes, FCN_E_ARG, "detection_output: background label %d outside %d classes",
                p.background, p.num_classes);
    FCN_REQUIRE(p.code_type == FCN_CODE_CORNER || p.code_type == FCN_CODE_CENTER_SIZE, FCN_E_UNSUPPORTED,
                "detection_output: code type %d (CORNER and CENTER_SIZE only)", p.code_type);
    FCN_REQUIRE((p.top_k == -1 || p.top_k > 0) && (p.keep_top_k == -1 || p.keep_top_k > 0), FCN_E_ARG,
                "detection_output: top_k %d / keep_top_k %d (positive, or -1)", p.top_k, p.keep_top_k);
    FCN_REQUIRE(p.nms_threshold == p.nms_threshold && p.conf_threshold == p.conf_threshold, FCN_E_ARG, "detection_output: a threshold is NaN");
    FCN_REQUIRE(p.loc_rstride >= 0 && p.conf_rstride >= 0 && (long long)p.loc_rstride >= 4ll * p.P * (p.N > 1) &&
                    (long long)p.conf_rstride >= (long long)p.P * p.num_classes * (p.N > 1), FCN_E_ARG,
                "detection_output: row strides %d / %d below the rows' widths", p.loc_rstride, p.conf_rstride);
    const long long kmax = p.top_k > -1 ? (p.top_k < p.P ? p.top_k : p.P) : p.P;
    FCN_REQUIRE(kmax <= FCN_DETOUT_MAX_TOPK, FCN_E_UNSUPPORTED, "detection_output: %lld candidates per class (top_k %d, %d priors) exceed %d",
                kmax, p.top_k, p.P, FCN_DETOUT_MAX_TOPK);
    const long long two31 = 1ll << 31;
    FCN_REQUIRE((long long)p.N * p.num_classes * p.P < two31 && (long long)p.N * p.loc_rstride < two31 && (long long)p.N * p.conf_rstride < two31 &&
                    (long long)p.N * p.num_classes * kmax < two31 && 7ll * p.capacity < two31 && (long long)p.N * p.P * 4 < two31,
                FCN_E_UNSUPPORTED, "detection_output: extents past 2^31 elements");
    FCN_REQUIRE(p.N <= 65535 && p.num_classes <= 65535, FCN_E_UNSUPPORTED, "detection_output: more than 65535 images or classes");
    const long long fg = p.num_classes - (p.background >= 0 ? 1 : 0);
    long long per_image = fg * kmax;
    if (p.keep_top_k > -1 && p.keep_top_k < per_image) per_image = p.keep_top_k;
    FCN_REQUIRE(p.capacity >= 0, FCN_E_ARG, "detection_output: negative capacity");
    FCN_REQUIRE((long long)p.capacity >= p.N * per_image, FCN_E_CAPACITY, "detection_output: capacity %d rows, %d images can yield %lld each",
                p.capacity, p.N, per_image);
    d->p = p;
    d->kmax = (int)kmax;
    const size_t nck = (size_t)p.N * p.num_classes * kmax, nc = (size_t)p.N * p.num_classes;
    size_t o = 0;
    d->off_boxes = o;   o += up16((size_t)p.N * p.P * 16);
    d->off_keys = o;    o += up16(nc * p.P * 8);
    d->off_kept = o;    o += up16(nck * 4);
    d->off_kept_n = o;  o += up16(nc * 4);
    d->off_ckey = o;    o += up16(nck * 8);
    d->off_centry = o;  o += up16(nck * 4);
    d->off_flag = o;    o += up16(nck * 4);
    d->off_total = o;   o += up16((size_t)p.N * 4);
    d->off_img_n = o;   o += up16((size_t)p.N * 4);
    d->off_cpref = o;   o += up16(nc * 4);
    d->bytes = o;
    return 0;
}

// a float as an unsigned whose order is the float's (no NaN arrives here: a NaN score is no candidate)
__device__ inline unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f + 0.f);      // (-0 + 0 = +0: the two zeros are one score)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float box_area(const V4 b) { return (b.z < b.x || b.w < b.y) ? 0.f : (b.z - b.x) * (b.w - b.y); }

__device__ inline float jaccard(const V4 a, const V4 b) {
    if (b.x > a.z || b.z < a.x || b.y > a.w || b.w < a.y) return 0.f;
    const float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x), ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    const float inter = iw * ih;
    if (!(iw > 0.f && ih > 0.f)) return 0.f;
    return inter / (box_area(a) + box_area(b) - inter);
}

// exclusive prefix sum of one int per thread over the 256 threads of a workgroup; *total = the sum.  `s`: 256 ints of LDS.
__device__ inline int block_scan_excl(int v, int* s, int* total) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void det_decode_kernel(const float* __restrict__ loc, const float* __restrict__ priors, V4* __restrict__ boxes,
                                                         int N, int P, int loc_rstride, int code, int var_encoded) {
    const long long total = (long long)N * P;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(t / P), p = (int)(t - (long long)n * P);
        const float* l = loc + (size_t)n * loc_rstride + (size_t)p * 4;
        const float* pb = priors + (size_t)p * 4;
        const float* pv = priors + (size_t)P * 4 + (size_t)p * 4;
        const float v0 = var_encoded ? 1.f : pv[0], v1 = var_encoded ? 1.f : pv[1], v2 = var_encoded ? 1.f : pv[2], v3 = var_encoded ? 1.f : pv[3];
        V4 b;
        if (code == FCN_CODE_CORNER) {
            b.x = pb[0] + v0 * l[0];
            b.y = pb[1] + v1 * l[1];
            b.z = pb[2] + v2 * l[2];
            b.w = pb[3] + v3 * l[3];
        } else {
            const float pw = pb[2] - pb[0], ph = pb[3] - pb[1];
            const float pcx = (pb[0] + pb[2]) / 2.f, pcy = (pb[1] + pb[3]) / 2.f;
            const float cx = v0 * l[0] * pw + pcx, cy = v1 * l[1] * ph + pcy;
            const float w = expf(v2 * l[2]) * pw, h = expf(v3 * l[3]) * ph;
            b.x = cx - w / 2.f;
            b.y = cy - h / 2.f;
            b.z = cx + w / 2.f;
            b.w = cy + h / 2.f;
        }
        boxes[t] = b;
    }
}

constexpr int DET_TILE = 1024;      // keys per LDS tile of a ranking pass; also FCN_DETOUT_MAX_TOPK
static_assert(DET_TILE == FCN_DETOUT_MAX_TOPK, "the sorted candidates of a class fill one tile");

// rank of `mine` among keys[0 .. m): how many are greater.  All 256 threads call it together (`valid` says whether this thread has a
// key); the keys pass through `tile` (DET_TILE u64 of LDS).
__device__ inline int rank_among(const u64* __restrict__ keys, int m, u64 mine, bool valid, u64* tile) {
    int rank = 0;
    for (int base = 0; base < m; base += DET_TILE) {
        const int cnt = min(DET_TILE, m - base);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += 256) tile[j] = keys[base + j];
        __syncthreads();
        if (valid)
            for (int j = 0; j < cnt; ++j) rank += tile[j] > mine ? 1 : 0;
    }
    return rank;
}

// grid (class, image): steps 2 and 3 for one class of one image
__global__ __launch_bounds__(256) void det_select_nms_kernel(const float* __restrict__ conf, const V4* __restrict__ boxes, u64* __restrict__ keys_all,
                                                             int* __restrict__ kept_all, int* __restrict__ kept_n, DetPlan d) {
    __shared__ u64 s_sorted[DET_TILE];
    __shared__ u64 s_tile[DET_TILE];
    __shared__ V4 s_box[DET_TILE];
    __shared__ int s_sup[DET_TILE];
    __shared__ int s_scan[256];
    __shared__ int s_m;
    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int P = d.p.P, NC = d.p.num_classes, kmax = d.kmax;
    const size_t nc = (size_t)n * NC + c;
    if (c == d.p.background) {
        if (tid == 0) kept_n[nc] = 0;
        return;
    }
    u64* keys = keys_all + nc * P;
    int* kept = kept_all + nc * kmax;
    if (tid == 0) s_m = 0;
    __syncthreads();
    const float* cf = conf + (size_t)n * d.p.conf_rstride + c;
    for (int p = tid; p < P; p += 256) {
        const float sc = cf[(size_t)p * NC];
        if (sc > d.p.conf_threshold) {
            const int slot = atomicAdd(&s_m, 1);
            keys[slot] = ((u64)ordered_bits(sc) << 32) | (u64)(0xFFFFFFFFu - (unsigned)p);
        }
    }
    __syncthreads();
    const int m = s_m;
    const int k = min(m, kmax);
    // the k greatest keys, in order, into LDS: a key's rank is its place
    for (int base = 0; base < m; base += 256) {
        const int i = base + tid;
        const bool valid = i < m;
        const u64 mine = valid ? keys[i] : 0ull;
        const int rank = rank_among(keys, m, mine, valid, s_tile);
        if (valid && rank < k) s_sorted[rank] = mine;
    }
    __syncthreads();
    for (int i = tid; i < k; i += 256) {
        const unsigned p = 0xFFFFFFFFu - (unsigned)(s_sorted[i] & 0xFFFFFFFFull);
        s_box[i] = boxes[(size_t)n * P + p];
        s_sup[i] = 0;
    }
    // the greedy sweep: candidate i, unless an earlier kept box suppressed it, is kept and suppresses every later one it overlaps
    for (int i = 0; i < k; ++i) {
        __syncthreads();
        if (s_sup[i]) continue;
        const V4 bi = s_box[i];
        for (int j = i + 1 + tid; j < k; j += 256)
            if (!s_sup[j] && jaccard(bi, s_box[j]) > d.p.nms_threshold) s_sup[j] = 1;
    }
    __syncthreads();
    // survivors in order: thread t owns candidates 4t .. 4t + 3
    int mine[4], cnt = 0;
    for (int e = 0; e < 4; ++e) {
        const int i = tid * 4 + e;
        mine[e] = (i < k && !s_sup[i]) ? 1 : 0;
        cnt += mine[e];
    }
    int total;
    int pos = block_scan_excl(cnt, s_scan, &total);
    for (int e = 0; e < 4; ++e)
        if (mine[e]) kept[pos++] = (int)(0xFFFFFFFFu - (unsigned)(s_sorted[tid * 4 + e] & 0xFFFFFFFFull));
    if (tid == 0) kept_n[nc] = total;
}

// grid (image): step 4.  Lists the image's survivors in row order (label, then NMS order), ranks them when the cut applies.
__global__ __launch_bounds__(256) void det_keep_kernel(const float* __restrict__ conf, const int* __restrict__ kept_all, const int* __restrict__ kept_n,
                                                       u64* __restrict__ ckey_all, int* __restrict__ centry_all, int* __restrict__ flag_all,
                                                       int* __restrict__ total_all, int* __restrict__ img_n, int* __restrict__ cpref_all, DetPlan d) {
    __shared__ u64 s_tile[DET_TILE];
    __shared__ int s_scan[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int P = d.p.P, NC = d.p.num_classes, kmax = d.kmax;
    const size_t per = (size_t)NC * kmax;
    u64* ckey = ckey_all + n * per;
    int* centry = centry_all + n * per;
    int* flag = flag_all + n * per;
    const int* kn = kept_n + (size_t)n * NC;
    const int* kept = kept_all + n * per;
    // where each class's survivors start in row order: one scan over the classes' counts, not over the classes' capacities
    int* cpref = cpref_all + (size_t)n * NC;
    int t_total = 0;
    for (int base = 0; base < NC; base += 256) {
        const int c = base + tid;
        const int v = c < NC ? kn[c] : 0;
        int chunk;
        const int ex = t_total + block_scan_excl(v, s_scan, &chunk);
        if (c < NC) cpref[c] = ex;
        t_total += chunk;
    }
    __syncthreads();
    for (size_t e = tid; e < per; e += 256) {
        const int c = (int)(e / kmax), pos = (int)(e - (size_t)c * kmax);
        if (pos < kn[c]) {
            const int at = cpref[c] + pos;
            const int p = kept[e];
            const float sc = conf[(size_t)n * d.p.conf_rstride + (size_t)p * NC + c];
            ckey[at] = ((u64)ordered_bits(sc) << 32) | (u64)(0xFFFFFFFFu - (unsigned)(c * P + p));
            centry[at] = (int)e;
        }
    }
    __syncthreads();
    const bool cut = d.p.keep_top_k > -1 && t_total > d.p.keep_top_k;
    for (int base = 0; base < t_total; base += 256) {
        const int i = base + tid;
        const bool valid = i < t_total;
        int keep = 1;
        if (cut) {
            const u64 mine = valid ? ckey[i] : 0ull;
            keep = rank_among(ckey, t_total, mine, valid, s_tile) < d.p.keep_top_k ? 1 : 0;
        }
        if (valid) flag[i] = keep;
    }
    if (tid == 0) {
        total_all[n] = t_total;
        img_n[n] = cut ? d.p.keep_top_k : t_total;
    }
}

// grid (image): step 5
__global__ __launch_bounds__(256) void det_rows_kernel(const float* __restrict__ conf, const V4* __restrict__ boxes, const int* __restrict__ kept_all,
                                                       const int* __restrict__ centry_all, const int* __restrict__ flag_all,
                                                       const int* __restrict__ total_all, const int* __restrict__ img_n, float* __restrict__ out_rows,
                                                       int* __restrict__ out_count, DetPlan d) {
    __shared__ int s_scan[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int P = d.p.P, NC = d.p.num_classes, kmax = d.kmax;
    const size_t per = (size_t)NC * kmax;
    int row = 0;
    for (int i = 0; i < n; ++i) row += img_n[i];
    if (n == 0 && tid == 0) {
        int all = 0;
        for (int i = 0; i < d.p.N; ++i) all += img_n[i];
        *out_count = all;
    }
    const int* centry = centry_all + n * per;
    const int* flag = flag_all + n * per;
    const int* kept = kept_all + n * per;
    const int t_total = total_all[n];
    for (int base = 0; base < t_total; base += 256) {
        const int i = base + tid;
        const int keep = (i < t_total && flag[i]) ? 1 : 0;
        int chunk;
        const int at = row + block_scan_excl(keep, s_scan, &chunk);
        if (keep && at < d.p.capacity) {
            const int e = centry[i], c = e / kmax, p = kept[e];
            const V4 b = boxes[(size_t)n * P + p];
            float* r = out_rows + (size_t)at * 7;
            r[0] = (float)n;
            r[1] = (float)c;
            r[2] = conf[(size_t)n * d.p.conf_rstride + (size_t)p * NC + c];
            r[3] = b.x;
            r[4] = b.y;
            r[5] = b.z;
            r[6] = b.w;
        }
        row += chunk;
    }
}

}  // namespace

extern "C" {

int fcn_ssd_gather_f32(const fcn_ssd_head* heads, int n_heads, int N, float* dst, int dst_rstride, int dst_cols, fcn_stream_t s) {
    FCN_REQUIRE(heads && dst && n_heads > 0 && N > 0 && dst_cols > 0, FCN_E_ARG, "ssd_gather: null pointer or non-positive extent");
    FCN_REQUIRE(n_heads <= FCN_SSD_MAX_HEADS, FCN_E_UNSUPPORTED, "ssd_gather: %d heads (at most %d a launch)", n_heads, FCN_SSD_MAX_HEADS);
    FCN_REQUIRE(N <= 65535, FCN_E_UNSUPPORTED, "ssd_gather: %d images (at most 65535)", N);
    FCN_REQUIRE(dst_rstride >= dst_cols, FCN_E_ARG, "ssd_gather: row stride %d below the row's %d columns", dst_rstride, dst_cols);
    FCN_REQUIRE(aligned(dst, 4), FCN_E_ALIGN, "ssd_gather: dst off 4 bytes");
    FCN_REQUIRE((long long)N * dst_rstride < (1ll << 31), FCN_E_UNSUPPORTED, "ssd_gather: destination past 2^31 elements");
    GatherArgs a;
    memset(&a, 0, sizeof(a));
    unsigned vec_mask = 0;
    long long most = 0;
    for (int i = 0; i < n_heads; ++i) {
        const fcn_ssd_head& h = heads[i];
        FCN_REQUIRE(h.src && h.pixels > 0 && h.C > 0, FCN_E_ARG, "ssd_gather: head %d: null source or non-positive extent", i);
        FCN_REQUIRE(h.coffset >= 0 && h.cstride >= h.coffset + h.C, FCN_E_ARG, "ssd_gather: head %d: channels %d + %d leave the pixel of %d", i,
                    h.coffset, h.C, h.cstride);
        FCN_REQUIRE(aligned(h.src, 4), FCN_E_ALIGN, "ssd_gather: head %d: source off 4 bytes", i);
        FCN_REQUIRE((long long)N * h.pixels * h.cstride < (1ll << 31) && (long long)h.pixels * h.C < (1ll << 31), FCN_E_UNSUPPORTED,
                    "ssd_gather: head %d past 2^31 elements", i);
        FCN_REQUIRE(h.dst_col >= 0 && (long long)h.dst_col + (long long)h.pixels * h.C <= dst_cols, FCN_E_ARG,
                    "ssd_gather: head %d: columns %d + %lld leave the row of %d", i, h.dst_col, (long long)h.pixels * h.C, dst_cols);
        for (int j = 0; j < i; ++j) {
            const long long a0 = h.dst_col, a1 = a0 + (long long)h.pixels * h.C;
            const long long b0 = heads[j].dst_col, b1 = b0 + (long long)heads[j].pixels * heads[j].C;
            FCN_REQUIRE(a1 <= b0 || b1 <= a0, FCN_E_ARG, "ssd_gather: heads %d and %d write the same columns", j, i);
        }
        a.h[i] = h;
        const bool vec = h.C % 4 == 0 && h.cstride % 4 == 0 && h.coffset % 4 == 0 && h.dst_col % 4 == 0 && dst_rstride % 4 == 0 &&
                         aligned(h.src, 16) && aligned(dst, 16);
        if (vec) vec_mask |= 1u << i;
        const long long work = (long long)h.pixels * (vec ? h.C / 4 : h.C);
        if (work > most) most = work;
    }
    hipLaunchKernelGGL(ssd_gather_kernel, dim3(stream_grid(most, 256), n_heads, N), dim3(256), 0, as_stream(s), dst, dst_rstride, vec_mask, a);
    FCN_LAUNCH_CHECK("ssd_gather");
    return 0;
}

int fcn_normalize_fwd_f32(const float* x, float* y, const float* scale, int pixels, int C, int x_cstride, int x_coffset, int y_cstride,
                          int y_coffset, int channel_shared, float eps, fcn_stream_t s) {
    FCN_REQUIRE(x && y && scale && pixels > 0 && C > 0, FCN_E_ARG, "normalize: null pointer or non-positive extent");
    FCN_REQUIRE(channel_shared == 0 || channel_shared == 1, FCN_E_ARG, "normalize: channel_shared must be 0 or 1");
    FCN_REQUIRE(eps >= 0.f, FCN_E_ARG, "normalize: eps %g is negative (or NaN)", (double)eps);
    FCN_REQUIRE(x_coffset >= 0 && y_coffset >= 0 && x_cstride >= x_coffset + C && (long long)y_cstride >= y_coffset + r4ll(C), FCN_E_ARG,
                "normalize: slice out of range (the top needs room for %lld channels)", r4ll(C));
    FCN_REQUIRE(aligned(x, 4) && aligned(y, 4) && aligned(scale, 4), FCN_E_ALIGN, "normalize: a pointer off 4 bytes");
    FCN_REQUIRE((long long)pixels * x_cstride < (1ll << 31) && (long long)pixels * y_cstride < (1ll << 31), FCN_E_UNSUPPORTED,
                "normalize: views past 2^31 elements");
    hipLaunchKernelGGL(normalize_kernel, dim3(stream_grid(pixels, 4)), dim3(256), 0, as_stream(s), x, y, scale, pixels, C, x_cstride, x_coffset,
                       y_cstride, y_coffset, channel_shared, eps);
    FCN_LAUNCH_CHECK("normalize");
    return 0;
}

size_t fcn_detection_output_workspace_bytes(const fcn_detout_params* h_params) {
    DetPlan d;
    if (det_plan(h_params, &d)) return 0;
    return d.bytes;
}

int fcn_detection_output_f32(const float* loc, const float* conf, const float* priors, const fcn_detout_params* h_params, float* out_rows,
                             int32_t* out_count, void* d_workspace, size_t workspace_bytes, fcn_stream_t s) {
    DetPlan d;
    if (int rc = det_plan(h_params, &d)) return rc;
    FCN_REQUIRE(loc && conf && priors && out_rows && out_count && d_workspace, FCN_E_ARG, "detection_output: null pointer");
    FCN_REQUIRE(workspace_bytes >= d.bytes, FCN_E_ARG, "detection_output: workspace of %zu bytes, %zu needed", workspace_bytes, d.bytes);
    FCN_REQUIRE(aligned(d_workspace, 16), FCN_E_ALIGN, "detection_output: workspace off 16 bytes");
    FCN_REQUIRE(aligned(loc, 4) && aligned(conf, 4) && aligned(priors, 4) && aligned(out_rows, 4) && aligned(out_count, 4), FCN_E_ALIGN,
                "detection_output: a pointer off 4 bytes");
    const fcn_detout_params& p = d.p;
    char* ws = static_cast<char*>(d_workspace);
    V4* boxes = reinterpret_cast<V4*>(ws + d.off_boxes);
    u64* keys = reinterpret_cast<u64*>(ws + d.off_keys);
    int* kept = reinterpret_cast<int*>(ws + d.off_kept);
    int* kept_n = reinterpret_cast<int*>(ws + d.off_kept_n);
    u64* ckey = reinterpret_cast<u64*>(ws + d.off_ckey);
    int* centry = reinterpret_cast<int*>(ws + d.off_centry);
    int* flag = reinterpret_cast<int*>(ws + d.off_flag);
    int* total = reinterpret_cast<int*>(ws + d.off_total);
    int* img_n = reinterpret_cast<int*>(ws + d.off_img_n);
    int* cpref = reinterpret_cast<int*>(ws + d.off_cpref);
    hipStream_t st = as_stream(s);
    hipLaunchKernelGGL(det_decode_kernel, dim3(stream_grid((long long)p.N * p.P, 256)), dim3(256), 0, st, loc, priors, boxes, p.N, p.P,
                       p.loc_rstride, p.code_type, p.variance_encoded ? 1 : 0);
    FCN_LAUNCH_CHECK("detection_output decode");
    hipLaunchKernelGGL(det_select_nms_kernel, dim3(p.num_classes, p.N), dim3(256), 0, st, conf, boxes, keys, kept, kept_n, d);
    FCN_LAUNCH_CHECK("detection_output select");
    hipLaunchKernelGGL(det_keep_kernel, dim3(p.N), dim3(256), 0, st, conf, kept, kept_n, ckey, centry, flag, total, img_n, cpref, d);
    FCN_LAUNCH_CHECK("detection_output keep");
    hipLaunchKernelGGL(det_rows_kernel, dim3(p.N), dim3(256), 0, st, conf, boxes, kept, centry, flag, total, img_n, out_rows, out_count, d);
    FCN_LAUNCH_CHECK("detection_output rows");
    return 0;
}

}  // extern "C"
