// The per-cell arithmetic of csrc/simplify.hip, shared with the host program tools/quadric_host_check.cpp so that
// it can be checked without a device and under the host sanitizers.
//
// A cell of the clustering grid holds member vertices and the corners (face, corner) whose vertex is a member. Its output vertex:
//   cen = the mean of the members;
//   per corner, with A, B, C the vertices of its face: n = (B - A) x (C - A), not normalised; d = n . (A - cen); M += n n^T; b += n d;
//   t = trace M; x = cen where t is not > 0, else x = cen + z with (M + 1e-3 t I) z = b -- symmetric positive definite with condition
//   at most 1001, solved by Cholesky without pivoting; x clamped per axis to the closed cell.
// There is no threshold and no branch on conditioning: x is a continuous function of the input. All float64, every operation in the
// written order: contraction is switched off here for clang, from this point to the end of the including file (a pragma placed after the
// include would leave these functions contracted: with a fused multiply-add the normal of a zero-area face is its rounding error, not
// zero); a host compiler takes -ffp-contract=off.
#pragma once

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define MORIG_QUADRIC_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define MORIG_QUADRIC_HD inline
#endif

namespace morig_quadric {

constexpr double EPS = 1e-3;      // the regularisation, as a share of trace M

// q[0 .. 5] = M: xx, xy, xz, yy, yz, zz; q[6 .. 8] = b
struct Acc { double q[9]; };

MORIG_QUADRIC_HD void zero(Acc& a) { for (int i = 0; i < 9; ++i) a.q[i] = 0.0; }

// a += o, term by term (the device adds its lanes' partial sums with this)
MORIG_QUADRIC_HD void add(Acc& a, const Acc& o) { for (int i = 0; i < 9; ++i) a.q[i] = a.q[i] + o.q[i]; }

// the grid coordinate of p on one axis: g = (p - lo) / ext * r, c = min((int)floor(g), r - 1), held into [0, r - 1] (p >= lo for every
// vertex of the mesh the frame was taken from; a value that is no number lands in cell 0)
MORIG_QUADRIC_HD int cell_coord(double p, double lo, double ext, int r) {
    const double g = (p - lo) / ext * (double)r;
    const double f = floor(g);
    if (!(f >= 0.0)) return 0;
    return f >= (double)(r - 1) ? r - 1 : (int)f;
}

// one corner of the face (A, B, C) into the cell's sums
MORIG_QUADRIC_HD void corner(const double* A, const double* B, const double* C, const double* cen, Acc& a) {
    double e1[3], e2[3], n[3];
    for (int c = 0; c < 3; ++c) { e1[c] = B[c] - A[c]; e2[c] = C[c] - A[c]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double d = (n[0] * (A[0] - cen[0]) + n[1] * (A[1] - cen[1])) + n[2] * (A[2] - cen[2]);
    a.q[0] = a.q[0] + n[0] * n[0];
    a.q[1] = a.q[1] + n[0] * n[1];
    a.q[2] = a.q[2] + n[0] * n[2];
    a.q[3] = a.q[3] + n[1] * n[1];
    a.q[4] = a.q[4] + n[1] * n[2];
    a.q[5] = a.q[5] + n[2] * n[2];
    a.q[6] = a.q[6] + n[0] * d;
    a.q[7] = a.q[7] + n[1] * d;
    a.q[8] = a.q[8] + n[2] * d;
}

// the output vertex of the cell (cx, cy, cz) of the grid (lo, h = ext / r) from its centroid and sums
MORIG_QUADRIC_HD void solve_clamp(const Acc& a, const double* cen, const double* lo, double h, const int* c, double* x) {
    const double t = (a.q[0] + a.q[3]) + a.q[5];
    double z[3] = {0.0, 0.0, 0.0};
    if (t > 0.0) {
        const double lam = EPS * t;
        const double a00 = a.q[0] + lam, a11 = a.q[3] + lam, a22 = a.q[5] + lam;
        const double l00 = sqrt(a00);
        const double l10 = a.q[1] / l00, l20 = a.q[2] / l00;
        const double l11 = sqrt(a11 - l10 * l10);
        const double l21 = (a.q[4] - l20 * l10) / l11;
        const double l22 = sqrt(a22 - (l20 * l20 + l21 * l21));
        const double y0 = a.q[6] / l00;
        const double y1 = (a.q[7] - l10 * y0) / l11;
        const double y2 = (a.q[8] - (l20 * y0 + l21 * y1)) / l22;
        z[2] = y2 / l22;
        z[1] = (y1 - l21 * z[2]) / l11;
        z[0] = (y0 - (l10 * z[1] + l20 * z[2])) / l00;
    }
    for (int k = 0; k < 3; ++k) {
        const double lower = lo[k] + (double)c[k] * h, upper = lo[k] + (double)(c[k] + 1) * h;
        const double v = cen[k] + z[k];
        x[k] = v < lower ? lower : (v > upper ? upper : v);
    }
}

}  // namespace morig_quadric
