// Ray against a closed triangle and the pixel ray of a camera: the rules of csrc/scan.hip, shared with the host
// program tools/raytri_host_check.cpp so that they can be checked without a device and under the host sanitizers.
//
// Moeller-Trumbore numerators for the ray o + t d and the triangle (A, B, C), e1 = B - A, e2 = C - A, p = d x e2, s = o - A, q = s x e1:
//     det = e1 . p      un = s . p      vn = d . q      tn = e2 . q          (every dot product as (x + y) + z)
// The inside test divides nothing: for det > 0 it is un >= 0, vn >= 0, un + vn <= det, mirrored for det < 0; det == 0 (a ray in the
// triangle's plane, a zero-area triangle) or any quantity that is no finite number is a miss. Touching counts: a ray through an edge or a
// corner is inside. Then t = tn / det, and a hit needs t > near. All float64, every operation in the written order (the including file
// switches contraction off): wherever the products are exact -- vertices and rays on a coarse binary grid -- the boundary is decided exactly.
//
// The pixel ray. A camera is 16 doubles: eye [0..2], f [3..5], r [6..8], u [9..11], px [12], py [13], near [14], [15] unused. Pixel
// (row i, column j) of a W x H image has a = ((2 j + 1) - W) px and b = (H - (2 i + 1)) py; orthographic: origin eye + a r + b u,
// direction f; pinhole: origin eye, direction f + a r + b u (not normalised, so t is the depth along the optical axis).
#pragma once

#if defined(__HIPCC__)
#define MORIG_RAYTRI_HD __host__ __device__ __forceinline__
#else
#define MORIG_RAYTRI_HD inline
#endif

namespace morig_raytri {

constexpr int CAM_DOUBLES = 16;
constexpr int ORTHOGRAPHIC = 0, PINHOLE = 1;

struct Num { double det, un, vn, tn; };

MORIG_RAYTRI_HD bool is_finite(double x) { return x - x == 0.0; }

MORIG_RAYTRI_HD Num numerators(const double* o, const double* d, const double* A, const double* B, const double* C) {
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    const double px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
    const double sx = o[0] - A[0], sy = o[1] - A[1], sz = o[2] - A[2];
    const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    Num n;
    n.det = (e1x * px + e1y * py) + e1z * pz;
    n.un = (sx * px + sy * py) + sz * pz;
    n.vn = (d[0] * qx + d[1] * qy) + d[2] * qz;
    n.tn = (e2x * qx + e2y * qy) + e2z * qz;
    return n;
}

MORIG_RAYTRI_HD bool inside(const Num& n) {
    if (!is_finite(n.det) || !is_finite(n.un) || !is_finite(n.vn) || !is_finite(n.tn)) return false;
    if (n.det > 0.0) return n.un >= 0.0 && n.vn >= 0.0 && n.un + n.vn <= n.det;
    if (n.det < 0.0) return n.un <= 0.0 && n.vn <= 0.0 && n.un + n.vn >= n.det;
    return false;
}

// the ray meets the closed triangle at t > near
MORIG_RAYTRI_HD bool hit(const Num& n, double near, double& t) {
    if (!inside(n)) return false;
    t = n.tn / n.det;
    return t > near;
}

MORIG_RAYTRI_HD void pixel_ray(const double* cam, int kind, int W, int H, int i, int j, double* o, double* d) {
    const double a = (double)((2 * j + 1) - W) * cam[12], b = (double)(H - (2 * i + 1)) * cam[13];
    for (int c = 0; c < 3; ++c) {
        if (kind == PINHOLE) {
            o[c] = cam[c];
            d[c] = (cam[3 + c] + a * cam[6 + c]) + b * cam[9 + c];
        } else {
            o[c] = (cam[c] + a * cam[6 + c]) + b * cam[9 + c];
            d[c] = cam[3 + c];
        }
    }
}

}  // namespace morig_raytri
