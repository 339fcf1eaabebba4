// The vertex-to-bone ray of the skinning inputs (calc_pts2bone_visible_mat, joint2rig.py:71-94; DESIGN.md sections 11 and 28): the rule
// of bone_visibility_kernel in csrc/geodesic.hip restated for the tree walk of csrc/bvh.hip and shared with the host program
// tools/visibility_host_check.cpp, so that it can be checked without a device and under the host sanitizers. All float64, every operation
// in the order bone_visibility_kernel writes it (the including file switches contraction off): both kernels decide every face alike.
//
// Ray.      o = the bone's nearest point to the vertex p (pt2line, with its zero-length-bone branch), r = p - o, len = |r|,
//           d = r + 1e-15 per coordinate, dn = |d|.
// Face.     e1 = B - A, e2 = C - A, area = |e1 x e2|, p = d x e2, det = e1 . p. Parallel unless |det| > 1e-12 dn area. inv = 1 / det,
//           u = (s . p) inv with s = o - A, v = (d . q) inv with q = s x e1; a hit needs u in [-1e-12, 1 + 1e-12], v >= -1e-12,
//           u + v <= 1 + 1e-12 and t = (e2 . q) inv > 0.
// Distance. h(t) = sqrt(((t dx)^2 + (t dy)^2) + (t dz)^2): rounding is monotone, so h does not decrease with t > 0 and the smallest h
//           over the hits is h of the smallest t.
// Visible.  |min_hit - len| < 1e-4 with min_hit = len when nothing is hit (or every h is +inf). A hit with h < len that is not within
//           1e-4 of len DECIDES: every nearer hit gives an h that is smaller still, so the ray is invisible whatever else is hit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MORIG_BONEVIS_HD __host__ __device__ __forceinline__
#else
#define MORIG_BONEVIS_HD inline
#endif

namespace morig_bonevis {

struct Ray { double o[3], d[3], len, dn; };

// pts2line: the nearest point of the segment bn[0..2] -> bn[3..5] to p
MORIG_BONEVIS_HD void pt2line(const double* p, const double* bn, double* o) {
    const double ax = bn[0], ay = bn[1], az = bn[2];
    const double ex = bn[3] - ax, ey = bn[4] - ay, ez = bn[5] - az;
    const double l2 = (ex * ex + ey * ey) + ez * ez;
    o[0] = ax; o[1] = ay; o[2] = az;
    if (!(fabs(l2) < 1e-8)) {
        double t = (((p[0] - ax) * ex + (p[1] - ay) * ey) + (p[2] - az) * ez) / l2;
        t = fmin(fmax(t, 0.0), 1.0);
        o[0] = ax + t * ex; o[1] = ay + t * ey; o[2] = az + t * ez;
    }
}

MORIG_BONEVIS_HD Ray ray_of(const double* p, const double* bn) {
    Ray r;
    pt2line(p, bn, r.o);
    const double rx = p[0] - r.o[0], ry = p[1] - r.o[1], rz = p[2] - r.o[2];
    r.len = sqrt((rx * rx + ry * ry) + rz * rz);
    r.d[0] = rx + 1e-15; r.d[1] = ry + 1e-15; r.d[2] = rz + 1e-15;
    r.dn = sqrt((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    return r;
}

// the tolerance Moeller-Trumbore: true and t where the ray meets the face (A, B, C) at t > 0
MORIG_BONEVIS_HD bool hit(const Ray& r, const double* A, const double* B, const double* C, double& t) {
    const double dx = r.d[0], dy = r.d[1], dz = r.d[2];
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double area = sqrt((nx * nx + ny * ny) + nz * nz);
    const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const double det = (e1x * px + e1y * py) + e1z * pz;
    if (!(fabs(det) > 1e-12 * r.dn * area)) return false;
    const double inv = 1.0 / det;
    const double tx = r.o[0] - A[0], ty = r.o[1] - A[1], tz = r.o[2] - A[2];
    const double u = ((tx * px + ty * py) + tz * pz) * inv;
    if (u < -1e-12 || u > 1.0 + 1e-12) return false;
    const double qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
    const double v = ((dx * qx + dy * qy) + dz * qz) * inv;
    if (v < -1e-12 || u + v > 1.0 + 1e-12) return false;
    t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
    return t > 0.0;
}

MORIG_BONEVIS_HD double hit_distance(const Ray& r, double t) {
    const double hx = t * r.d[0], hy = t * r.d[1], hz = t * r.d[2];
    return sqrt((hx * hx + hy * hy) + hz * hz);
}

// min_hit: the smallest h over the hits, +inf without one
MORIG_BONEVIS_HD bool visible(double min_hit, double len) {
    if (isinf(min_hit)) min_hit = len;
    return fabs(min_hit - len) < 1e-4;
}

// a hit at distance h settles the ray as invisible: every nearer hit does too
MORIG_BONEVIS_HD bool decides(double h, double len) { return h < len && !(fabs(h - len) < 1e-4); }

}  // namespace morig_bonevis
