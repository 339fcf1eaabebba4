// The per-joint statistics of csrc/labels.hip, shared with the host program tools/boneray_host_check.cpp so that
// they can be checked without a device and under the host sanitizers. A joint owns n <= MAX_RAYS hit distances t (+inf = the ray missed).
//
//     hit         t < +inf (a NaN is no hit)
//     rank_of     the place of hit i among the hits in ascending (t, ray index) order, found by counting: no sort, no scratch memory
//     position    the 20th percentile of n_hit sorted values s lies at h = 0.2 (n_hit - 1): lo = floor(h), hi = min(lo + 1, n_hit - 1),
//                 frac = h - lo
//     value       p20 = s[lo] + frac (s[hi] - s[lo])
//     kept        a hit with t <= keep_factor p20
//     mean_kept   the kept t added in ascending RAY order (not sorted order), divided by their count; `fill` when nothing is kept
// All float64, every operation in the written order (the including file switches contraction off). Plain C++ without a HIP construct.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORIG_BONERAY_HD __host__ __device__ __forceinline__
#else
#define MORIG_BONERAY_HD inline
#endif

namespace morig_boneray {

constexpr int MAX_RAYS = 1024;
constexpr double PCT = 0.2;

struct Stats { int n_hit, n_kept; double p20, featuresize; };

MORIG_BONERAY_HD bool hit(double t) { return t < __builtin_inf(); }

MORIG_BONERAY_HD int rank_of(const double* t, int n, int i) {
    const double ti = t[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
        const double tj = t[j];
        if (hit(tj) && (tj < ti || (tj == ti && j < i))) ++r;
    }
    return r;
}

MORIG_BONERAY_HD void position(int n_hit, int& lo, int& hi, double& frac) {
    const double h = PCT * (double)(n_hit - 1);
    lo = (int)h;                                                                        // h >= 0: truncation is floor
    hi = lo + 1 < n_hit - 1 ? lo + 1 : n_hit - 1;
    frac = h - (double)lo;
}

MORIG_BONERAY_HD double value(double s_lo, double s_hi, double frac) { return s_lo + frac * (s_hi - s_lo); }

MORIG_BONERAY_HD bool kept(double t, double threshold) { return hit(t) && t <= threshold; }

MORIG_BONERAY_HD double mean_kept(const double* t, int n, double threshold, double fill, int& count) {
    double s = 0.0;
    count = 0;
    for (int i = 0; i < n; ++i)
        if (kept(t[i], threshold)) { s = s + t[i]; ++count; }
    return count > 0 ? s / (double)count : fill;
}

// One joint, one thread: what a wave of select_kernel computes with its lanes striding over i. flags: n bytes.
MORIG_BONERAY_HD Stats select_serial(const double* t, int n, double keep_factor, double fill, uint8_t* flags) {
    Stats st;
    st.n_hit = 0;
    for (int i = 0; i < n; ++i) st.n_hit += hit(t[i]) ? 1 : 0;
    st.n_kept = 0;
    st.p20 = __builtin_nan("");
    st.featuresize = fill;
    if (st.n_hit == 0) {
        for (int i = 0; i < n; ++i) flags[i] = 0;
        return st;
    }
    int lo, hi;
    double frac, s_lo = 0.0, s_hi = 0.0;
    position(st.n_hit, lo, hi, frac);
    for (int i = 0; i < n; ++i) {
        if (!hit(t[i])) continue;
        const int r = rank_of(t, n, i);
        if (r == lo) s_lo = t[i];
        if (r == hi) s_hi = t[i];
    }
    st.p20 = value(s_lo, s_hi, frac);
    const double threshold = keep_factor * st.p20;
    for (int i = 0; i < n; ++i) flags[i] = kept(t[i], threshold) ? 1 : 0;
    st.featuresize = mean_kept(t, n, threshold, fill, st.n_kept);
    return st;
}

}  // namespace morig_boneray
