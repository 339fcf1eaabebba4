// The sequential core of the rigid fit (csrc/piecewise.hip): the proper rotation R that maximises sum_k tar_k . (R src_k) for two centred
// point sets, from their 3 x 3 cross-covariance -- what the reference's `U, s, Vh = svd(M); R = U Vh` plus its determinant fix returns.
// Plain C++ without a HIP construct, so that the kernels and tools/kabsch_host_check.cpp (built with the host sanitizers, run by
// tests/test_piecewise_host.py) compile the SAME text. float64 throughout; the translation is added by the caller.
//
// Method: B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions", J. Opt. Soc. Am. A 4(4), 1987. The unit
// quaternion of R is the eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix N built from M; the eigenvalues of N are
// s1 + s2 + d s3, s1 - s2 - d s3, -s1 + s2 - d s3, -s1 - s2 + d s3 (s: singular values of M, d: the sign of det M), so the answer is
// unique while s2 + d s3 > 0. A fit to three points has s3 = 0 (rank 2) and needs no special case here, where the SVD route needs the
// determinant fix. Collinear or coincident samples (rank <= 1) have no unique answer: this returns one of the maximisers, not
// necessarily the reference's. N is diagonalised by cyclic Jacobi sweeps with a fixed pair order; every loop has constant bounds, so the
// 4 x 4 arrays stay in registers on the device. The error of R is about (machine epsilon) * s1 / (s2 + d s3).
#pragma once

#if defined(__HIPCC__)
#define MORIG_KABSCH_HD __host__ __device__ inline
#else
#define MORIG_KABSCH_HD inline
#endif

namespace morig_kabsch {

constexpr int MAX_SWEEPS = 16;            // 4 x 4 Jacobi converges quadratically: 5 to 7 sweeps in practice; the bound only ends NaN input

// M row-major [3][3], M[i][j] = sum_k tar_c[k][i] * src_c[k][j] (tar_c^T src_c); R row-major [3][3] with tar ~ R src.
// Returns the number of sweeps taken. eig, where given, receives the four eigenvalues of N as the sweeps left them (unsorted).
MORIG_KABSCH_HD int rotation(const double* M, double* R, double* eig = nullptr) {
    // Horn's S_ab = sum_k src_a tar_b = M[b][a]
    const double Sxx = M[0], Sxy = M[3], Sxz = M[6], Syx = M[1], Syy = M[4], Syz = M[7], Szx = M[2], Szy = M[5], Szz = M[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    int sweeps = 0;
    for (; sweeps < MAX_SWEEPS; ++sweeps) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += __builtin_fabs(A[p][q]);
        if (!(off > 0.0)) break;                                                   // diagonal (or NaN: nothing to gain)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                const double g = 100.0 * __builtin_fabs(apq);
                if (__builtin_fabs(A[p][p]) + g == __builtin_fabs(A[p][p]) && __builtin_fabs(A[q][q]) + g == __builtin_fabs(A[q][q])) {
                    A[p][q] = 0.0; A[q][p] = 0.0;                                  // below the rounding of both diagonal entries
                    continue;
                }
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double tt = (theta < 0.0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
                const double c = 1.0 / __builtin_sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                      // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                      // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                      // V <- V J: the columns become the eigenvectors
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];      // the largest eigenvalue; the first on a tie
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) { best = A[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
    const double n = __builtin_sqrt(((w * w + x * x) + y * y) + z * z);
    w /= n; x /= n; y /= n; z /= n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    if (eig) { eig[0] = A[0][0]; eig[1] = A[1][1]; eig[2] = A[2][2]; eig[3] = A[3][3]; }
    return sweeps;
}

}  // namespace morig_kabsch
