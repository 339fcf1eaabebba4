// The per-joint arithmetic of motion playback (csrc/playback.hip): quaternion -> rotation matrix, one step of the
// forward kinematics, the inverse of a bind transform and the affine product both the local-vertex and the skinning kernel use. Plain C++
// without a HIP construct, so that the kernels and tools/pose_host_check.cpp (built with the host sanitizers, run by
// tests/test_playback_host.py) compile the SAME text. float64 throughout, every sum in the written order; compile without contraction
// (-ffp-contract=off; the pragma below covers clang). Matrices are row-major double[9]; a transform is double[12] = the matrix, then the
// translation.
#pragma once
#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define MORIG_POSE_HD __host__ __device__ inline
#else
#define MORIG_POSE_HD inline
#endif

namespace morig_pose {

MORIG_POSE_HD double dot4(const double* a, const double* b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// one component of the reference's smoothing statement: ((q[t] + 0.5 q[t + 1]) + 0.5 q[t - 1]) / 2.0
MORIG_POSE_HD double smooth(double cur, double next, double prev) { return ((cur + 0.5 * next) + 0.5 * prev) / 2.0; }

// q = (x, y, z, w), any length: the matrix of q / |q|. false (and the identity) when |q| is zero or no finite number.
MORIG_POSE_HD bool quat_to_matrix(const double* q, double* R) {
    const double n = sqrt(dot4(q, q));
    if (!(n > 0.0) || !(n <= 1.7976931348623157e308)) {
        R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
        return false;
    }
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    R[0] = ((x2 - y2) - z2) + w2;
    R[1] = 2.0 * (xy - zw);
    R[2] = 2.0 * (xz + yw);
    R[3] = 2.0 * (xy + zw);
    R[4] = ((y2 - x2) - z2) + w2;
    R[5] = 2.0 * (yz - xw);
    R[6] = 2.0 * (xz - yw);
    R[7] = 2.0 * (yz + xw);
    R[8] = ((-x2 - y2) + z2) + w2;
    return true;
}

// a position as the rig stores it: float32 joints round on store, and the children read the rounded value
MORIG_POSE_HD double round_store(double v, bool f32) { return f32 ? (double)(float)v : v; }

// M v + t for a transform M = [matrix | t]: ((m0 v0 + m1 v1) + m2 v2) + t per row
MORIG_POSE_HD void apply(const double* M, const double* v, double* out) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a) out[a] = ((M[3 * a] * v[0] + M[3 * a + 1] * v[1]) + M[3 * a + 2] * v[2]) + M[9 + a];
}

// one child of Rig.FK: G = Gp R, pos = Gp offset + pos_p (rounded to the rig's type). parent, out: transforms [12]
MORIG_POSE_HD void fk_step(const double* parent, const double* R, const double* offset, bool f32, double* out) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int b = 0; b < 3; ++b) out[3 * a + b] = (parent[3 * a] * R[b] + parent[3 * a + 1] * R[3 + b]) + parent[3 * a + 2] * R[6 + b];
    }
    double p[3];
    apply(parent, offset, p);
    for (int a = 0; a < 3; ++a) out[9 + a] = round_store(p[a], f32);
}

// adjugate / determinant, the determinant expanded along the first row
MORIG_POSE_HD void inverse3(const double* A, double* inv) {
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = (A[0] * c0 + A[1] * c1) + A[2] * c2;
    inv[0] = c0 / det;
    inv[1] = (A[2] * A[7] - A[1] * A[8]) / det;
    inv[2] = (A[1] * A[5] - A[2] * A[4]) / det;
    inv[3] = c1 / det;
    inv[4] = (A[0] * A[8] - A[2] * A[6]) / det;
    inv[5] = (A[2] * A[3] - A[0] * A[5]) / det;
    inv[6] = c2 / det;
    inv[7] = (A[1] * A[6] - A[0] * A[7]) / det;
    inv[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}

// the inverse of a bind transform [A | p]: [A^-1 | -(A^-1 p)]
MORIG_POSE_HD void inverse_transform(const double* bind, double* inv) {
    inverse3(bind, inv);
    for (int a = 0; a < 3; ++a) inv[9 + a] = -((inv[3 * a] * bind[9] + inv[3 * a + 1] * bind[10]) + inv[3 * a + 2] * bind[11]);
}

}  // namespace morig_pose
