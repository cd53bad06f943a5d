// What interp.hip (Interp) and argmax.hip (Interp + ArgMax in one pass) share: the geometry of a resampling, the integer cell
// arithmetic of an output index, the blend, the 16-byte segment loads and the contract checks.  One copy, so the fused pass blends
// exactly what the Interp launch would have written.
#pragma once

#include "common.h"

namespace {

using namespace fcn;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

struct InterpGeom {
    int H, W, C;                     // the bottom's extents
    int off, He, We;                 // the effective input: rows / columns off .. off + He - 1 (off = -pad_beg)
    int OH, OW;
    int in_cstride, in_coffset;      // x / dX
    int out_cstride, out_coffset;    // y / dY
};

// output index o of n2 -> cell i0, its neighbour i1 and the neighbour's weight lam in an input of n1
__device__ inline void interp_pos(int o, int n1, int n2, int& i0, int& i1, float& lam) {
    if (n1 == 1 || n2 == 1) {
        i0 = i1 = 0;
        lam = 0.f;
        return;
    }
    const unsigned d = (unsigned)(n2 - 1), num = (unsigned)o * (unsigned)(n1 - 1);
    const unsigned q = num / d;
    i0 = (int)q;
    i1 = min(i0 + 1, n1 - 1);
    lam = (float)(num - q * d) / (float)d;
}

__device__ inline float blend(float p00, float p01, float p10, float p11, float lx, float ly) {
    const float top = lx == 0.f ? p00 : (1.f - lx) * p00 + lx * p01;
    const float bot = lx == 0.f ? p10 : (1.f - lx) * p10 + lx * p11;
    return ly == 0.f ? top : (1.f - ly) * top + ly * bot;
}

// one 16-byte segment (or one element) as floats
template <int E> __device__ inline void load_seg(const float* p, float* v) {
    if (E == 1) {
        v[0] = *p;
    } else {
        typedef float V __attribute__((ext_vector_type(4)));
        const V t = *reinterpret_cast<const V*>(p);
        for (int e = 0; e < 4; ++e) v[e] = t[e];
    }
}
template <int E> __device__ inline void load_seg(const _Float16* p, float* v) {
    if (E == 1) {
        v[0] = (float)*p;
    } else {
        typedef _Float16 V __attribute__((ext_vector_type(8)));
        const V t = *reinterpret_cast<const V*>(p);
        for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
    }
}

// the checks the entry points share; every one precedes the first HIP call.  out_C: channels of the output view (C for Interp and its
// adjoint, what an ArgMax writes per pixel for the fused pass).  in_e / out_e: elements per 16-byte segment that the strides and
// offsets of the two views must be multiples of (0: no such demand, the scalar path serves them).
inline int interp_check(const char* who, const void* in, const void* out, int N, int H, int W, int C, int in_cstride, int in_coffset, int pad_beg,
                        int pad_end, int OH, int OW, int out_C, int out_cstride, int out_coffset, int in_e, int out_e, InterpGeom* g) {
    FCN_REQUIRE(in && out && N > 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, FCN_E_ARG, "%s: null pointer or non-positive extent", who);
    FCN_REQUIRE(pad_beg <= 0 && pad_end <= 0, FCN_E_ARG, "%s: pad_beg %d / pad_end %d must not be positive (they crop)", who, pad_beg, pad_end);
    const long long He = (long long)H + pad_beg + pad_end, We = (long long)W + pad_beg + pad_end;
    FCN_REQUIRE(He >= 1 && We >= 1, FCN_E_ARG, "%s: pads %d / %d leave nothing of the %d x %d view", who, pad_beg, pad_end, H, W);
    FCN_REQUIRE(in_coffset >= 0 && out_coffset >= 0 && in_cstride >= in_coffset + C && out_cstride >= out_coffset + out_C, FCN_E_ARG,
                "%s: slice out of range", who);
    if (in_e)
        FCN_REQUIRE(in_cstride % in_e == 0 && in_coffset % in_e == 0 && aligned16(in), FCN_E_ALIGN,
                    "%s: input stride and offset must be multiples of %d elements, the pointer of 16 bytes", who, in_e);
    if (out_e)
        FCN_REQUIRE(out_cstride % out_e == 0 && out_coffset % out_e == 0 && aligned16(out), FCN_E_ALIGN,
                    "%s: output stride and offset must be multiples of %d elements, the pointer of 16 bytes", who, out_e);
    FCN_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, FCN_E_ALIGN,
                "%s: pointers must be multiples of 4 bytes", who);
    // what the kernels keep in 32 bits: a row's lanes, o * (n1 - 1), the row counts; (n2 - 1) must be exact as a float
    const long long lim = 1ll << 31;
    FCN_REQUIRE((long long)OH * He < lim && (long long)OW * We < lim && (long long)W * in_cstride < lim && (long long)OW * out_cstride < lim &&
                    (long long)N * H < lim && (long long)N * OH < lim && OH <= (1 << 24) && OW <= (1 << 24),
                FCN_E_UNSUPPORTED, "%s: a row or an axis past 2^31 lanes (or an output extent past 2^24)", who);
    *g = InterpGeom{H, W, C, -pad_beg, (int)He, (int)We, OH, OW, in_cstride, in_coffset, out_cstride, out_coffset};
    return 0;
}

}  // namespace
