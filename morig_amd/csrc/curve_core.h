// The per-element arithmetic of the motion-stage curves: the float32 correspondence distance of
// evaluate/eval_corr.py:17-21, the per-mesh normalisation of evaluate/eval_attn.py:21 and the comparison of one value against up to
// MORIG_CURVE_MAX_BINS float32 bins. Every operation is one float32 operation rounded to nearest, in the written order, never contracted
// into a fused multiply-add: that is what numpy computes on float32 arrays, and the counts are compared with numpy's bit for bit.
// Plain C++ without a HIP construct, so that csrc/motion_metrics.hip and tools/curve_host_check.cpp (built with the host sanitizers, run by
// tests/test_motion_metrics_host.py) compile the SAME text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORIG_CURVE_HD __host__ __device__ __forceinline__
#else
#define MORIG_CURVE_HD inline
#endif

// No operation below may be contracted into a fused multiply-add. The pragma stands at file scope, in front of the helpers: hipcc
// contracts across inlined functions unless the operations THEMSELVES were compiled under it. It holds to the end of the translation unit
// that includes this file, which is what its includers want.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace morig_curve {

constexpr int MAX_BINS = 32;                                    // MORIG_CURVE_MAX_BINS: one bit of the mask per bin

// the four float32 operations, as plain operators under the pragma above. HIP's round-to-nearest intrinsics (__fmul_rn, __fadd_rn ...)
// are NOT used: its headers define them as these same operators, compiled there without the pragma, and the compiler fused
// __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)) into v_fmac_f32 -- the assembly of csrc/motion_metrics.hip shows v_mul_f32 / v_add_f32 with
// the form below.
MORIG_CURVE_HD float sub(float a, float b) { return a - b; }
MORIG_CURVE_HD float mul(float a, float b) { return a * b; }
MORIG_CURVE_HD float add(float a, float b) { return a + b; }
MORIG_CURVE_HD float div(float a, float b) { return a / b; }
MORIG_CURVE_HD double root(double s) { return __builtin_sqrt(s); }

// |a - b| of two float32 points as numpy has it: d = a - b per component, (d0^2 + d1^2) + d2^2, then the correctly rounded float32 square
// root -- taken as (float)sqrt((double)s): a float64 root rounded once more is the correctly rounded float32 root (53 >= 2 * 24 + 2),
// whatever fast-sqrt setting the float32 one is compiled under
MORIG_CURVE_HD float distance3(const float* a, const float* b) {
    const float d0 = sub(a[0], b[0]), d1 = sub(a[1], b[1]), d2 = sub(a[2], b[2]);
    const float s = add(add(mul(d0, d0), mul(d1, d1)), mul(d2, d2));
    return (float)root((double)s);
}

// (x - mn) / (mx - mn) in float32. A constant mesh gives 0 / 0 = NaN, a NaN minimum makes every value NaN: nothing compares true then.
MORIG_CURVE_HD float normalised(float x, float mn, float mx) {
    return div(sub(x, mn), sub(mx, mn));
}

// float32 minimum / maximum of a run as np.min / np.max give them: NaN as soon as one element is NaN. `seen_nan` travels separately so
// that partial results can be merged in any order.
struct Range {
    float mn, mx;
    int seen_nan;
};
MORIG_CURVE_HD Range range_empty() { return Range{__builtin_huge_valf(), -__builtin_huge_valf(), 0}; }
MORIG_CURVE_HD Range range_add(Range r, float x) {
    if (x != x) r.seen_nan = 1;
    else {
        r.mn = x < r.mn ? x : r.mn;
        r.mx = x > r.mx ? x : r.mx;
    }
    return r;
}
MORIG_CURVE_HD Range range_merge(Range a, Range b) {
    return Range{b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.seen_nan | b.seen_nan};
}
MORIG_CURVE_HD void range_finish(Range r, float* mn, float* mx) {
    const float nan = __builtin_nanf("");
    *mn = r.seen_nan ? nan : r.mn;
    *mx = r.seen_nan ? nan : r.mx;
}

// The bin loop. Bit b of the result: value < bins[b] (below != 0: a correspondence within the tolerance, strict) or value > bins[b]
// (below == 0: a predicted positive, strict). The bins are float32 already: the caller rounded its Python floats once. A NaN value
// sets no bit. n_bins <= MAX_BINS.
MORIG_CURVE_HD uint32_t bin_mask(float value, const float* bins, int n_bins, int below) {
    uint32_t m = 0;
    for (int b = 0; b < n_bins; ++b) {
        const bool hit = below ? value < bins[b] : value > bins[b];
        m |= (uint32_t)hit << b;
    }
    return m;
}

// One correspondence row (v, p_gt) of a pair with n_vtx vertices and n_pts points (pts: the pair's first point, nn: the pair's first
// vertex entry). nn holds point indices local to the pair (nn_base = 0) or rows of the whole point array (nn_base = the pair's first
// row). -> the mask of tolerances met; *bad is set, and the row counts nothing, when v, p_gt or nn[v] lies outside the pair.
MORIG_CURVE_HD uint32_t corr_row_mask(const float* pts, int n_pts, const int32_t* nn, int n_vtx, int nn_base, int64_t v, int64_t p_gt,
                                      const float* tol, int n_tol, int* bad) {
    if (v < 0 || v >= n_vtx || p_gt < 0 || p_gt >= n_pts) { *bad = 1; return 0; }
    const int64_t p = (int64_t)nn[v] - nn_base;
    if (p < 0 || p >= n_pts) { *bad = 1; return 0; }
    return bin_mask(distance3(pts + 3 * p, pts + 3 * p_gt), tol, n_tol, 1);
}

}  // namespace morig_curve
