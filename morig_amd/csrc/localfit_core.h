// The sequential arithmetic of the local rigid motion (csrc/local_motion.hip, morig_amd/local_motion.py): what the
// reference's get_gt_rotation_icp does per vertex (data_proc/common_ops.py:47-78 with icp, :155-172). Plain C++ without a HIP construct,
// so that the kernels and tools/localfit_host_check.cpp (built with the host sanitizers, run by tests/test_local_motion_host.py) compile
// the SAME text. float64 throughout, every sum in the written order; the including file switches contraction off.
//
// dist         sqrt((d0^2 + d1^2) + d2^2), the entry of the reference's distance matrix, with the correctly rounded root
// choose_rung  the threshold ladder: 0.04, then 0.04 * 1.25 while fewer than 5 candidates pass, and a break only AFTER the
//              multiplication passes 0.06 -- so the third rung 0.04 * 1.25 * 1.25 is used whatever passes under it
// fit          one (vertex, frame): means in ascending patch order, M = tar_c^T src_c, R from kabsch_core.h, t = mean(tar) - R mean(src),
//              gap = (l1 - l2) / l1 of the two largest eigenvalues of Horn's matrix (0 where l1 <= 0: a patch of one point, or of
//              coincident points), residual = sqrt(mean |R p + t - q|^2) over a third walk. A patch without a point gives NaN.
#pragma once

#include "kabsch_core.h"

namespace morig_localfit {

constexpr int MIN_CANDIDATES = 5;

MORIG_KABSCH_HD double dist(const double* p, const double* q) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

MORIG_KABSCH_HD int choose_rung(int c0, int c1, int c2) {
    (void)c2;
    return c0 >= MIN_CANDIDATES ? 0 : (c1 >= MIN_CANDIDATES ? 1 : 2);
}

// ids [n]: the patch, rows of the mesh, ascending; an id outside [0, nv) is clamped and reported through *bad_id. src: the rest pose of
// the mesh, [nv][3]. tar: the frame's vertex 0 of the mesh, vertex u at tar + u * stride. rot6 [6]: the first, then the second COLUMN of R.
template <typename T>
MORIG_KABSCH_HD void fit(const int* ids, int n, int nv, const double* src, const T* tar, long long stride, double* rot6, double* trans,
                         double* gap, double* residual, int* bad_id) {
    const double nan = __builtin_nan("");
    if (n <= 0 || nv <= 0) {
        for (int c = 0; c < 6; ++c) rot6[c] = nan;
        for (int c = 0; c < 3; ++c) trans[c] = nan;
        *gap = nan;
        *residual = nan;
        return;
    }
    double ms[3] = {0.0, 0.0, 0.0}, mt[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) {
        int u = ids[k];
        if (u < 0 || u >= nv) { *bad_id = 1; u = u < 0 ? 0 : nv - 1; }
        for (int c = 0; c < 3; ++c) {
            ms[c] += src[(long long)u * 3 + c];
            mt[c] += (double)tar[(long long)u * stride + c];
        }
    }
    for (int c = 0; c < 3; ++c) { ms[c] = ms[c] / (double)n; mt[c] = mt[c] / (double)n; }
    double M[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) {
        int u = ids[k];
        if (u < 0 || u >= nv) u = u < 0 ? 0 : nv - 1;
        double sc[3], tc[3];
        for (int c = 0; c < 3; ++c) {
            sc[c] = src[(long long)u * 3 + c] - ms[c];
            tc[c] = (double)tar[(long long)u * stride + c] - mt[c];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[i * 3 + j] += tc[i] * sc[j];
    }
    double R[9], eig[4];
    morig_kabsch::rotation(M, R, eig);
    double l1 = eig[0], l2 = -__builtin_inf();
    for (int k = 1; k < 4; ++k) {
        if (eig[k] > l1) { l2 = l1; l1 = eig[k]; }
        else if (eig[k] > l2) l2 = eig[k];
    }
    *gap = l1 > 0.0 ? (l1 - l2) / l1 : 0.0;
    for (int c = 0; c < 3; ++c) trans[c] = mt[c] - ((R[c * 3] * ms[0] + R[c * 3 + 1] * ms[1]) + R[c * 3 + 2] * ms[2]);
    for (int c = 0; c < 3; ++c) { rot6[c] = R[c * 3]; rot6[3 + c] = R[c * 3 + 1]; }
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        int u = ids[k];
        if (u < 0 || u >= nv) u = u < 0 ? 0 : nv - 1;
        const double* p = src + (long long)u * 3;
        double e[3];
        for (int c = 0; c < 3; ++c)
            e[c] = (((R[c * 3] * p[0] + R[c * 3 + 1] * p[1]) + R[c * 3 + 2] * p[2]) + trans[c]) - (double)tar[(long long)u * stride + c];
        sum += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    *residual = __builtin_sqrt(sum / (double)n);
}

}  // namespace morig_localfit
