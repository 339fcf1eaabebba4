// Closest point of a closed triangle to a point, and the squared distance between two points: the per-pair rules of csrc/transfer.hip
// (DESIGN.md section 25), shared with the host program tools/pointtri_host_check.cpp so that they can be checked without a device and
// under the host sanitizers.
//
// Ericson's seven regions (Real-Time Collision Detection 5.1.5) for the point p and the triangle (a, b, c), ab = b - a, ac = c - a:
//     d1 = ab . (p - a)   d2 = ac . (p - a)   d3 = ab . (p - b)   d4 = ac . (p - b)   d5 = ab . (p - c)   d6 = ac . (p - c)
//     vc = d1 d4 - d3 d2  vb = d5 d2 - d1 d6  va = d3 d6 - d5 d4                       (every dot product as (x + y) + z)
// tested in this order, the first that holds decides:
//     vertex a   d1 <= 0 and d2 <= 0                                  bary (1, 0, 0)
//     vertex b   d3 >= 0 and d4 <= d3                                 bary (0, 1, 0)
//     edge ab    vc <= 0 and d1 >= 0 and d3 <= 0                      v = d1 / (d1 - d3): (1 - v, v, 0)
//     vertex c   d6 >= 0 and d5 <= d6                                 bary (0, 0, 1)
//     edge ac    vb <= 0 and d2 >= 0 and d6 <= 0                      w = d2 / (d2 - d6): (1 - w, 0, w)
//     edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0            w = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (0, 1 - w, w)
//     face       otherwise                                            s = (va + vb) + vc, v = vb / s, w = vc / s: ((1 - v) - w, v, w)
// Only comparisons decide the region; the divisions give the barycentrics alone. A zero-area triangle has va = vb = vc = 0 wherever the
// products are exact and falls into a vertex or an edge region by the same comparisons. The closest point is (b0 a + b1 b) + b2 c per
// coordinate -- a vertex region returns the vertex's own bits -- and the squared distance (dx^2 + dy^2) + dz^2 of p minus it. Should
// rounding carry a sliver into the face region with s = 0, the distance is no number and loses every comparison `<`.
// All float64, every operation in the written order (the including file switches contraction off).
#pragma once

#if defined(__HIPCC__)
#define MORIG_POINTTRI_HD __host__ __device__ __forceinline__
#else
#define MORIG_POINTTRI_HD inline
#endif

namespace morig_pointtri {

constexpr int VERTEX_A = 0, VERTEX_B = 1, EDGE_AB = 2, VERTEX_C = 3, EDGE_AC = 4, EDGE_BC = 5, FACE = 6;

MORIG_POINTTRI_HD double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// (dx^2 + dy^2) + dz^2: also the coincidence test of the remesh transfer (== 0: differences that underflow count, -0 equals 0)
MORIG_POINTTRI_HD double dist2(const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the barycentrics of the closest point of (a, b, c) to p; returns the region
MORIG_POINTTRI_HD int closest_bary(const double* p, const double* a, const double* b, const double* c, double* bary) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { bary[0] = 1.0; bary[1] = 0.0; bary[2] = 0.0; return VERTEX_A; }
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { bary[0] = 0.0; bary[1] = 1.0; bary[2] = 0.0; return VERTEX_B; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        bary[0] = 1.0 - v; bary[1] = v; bary[2] = 0.0;
        return EDGE_AB;
    }
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { bary[0] = 0.0; bary[1] = 0.0; bary[2] = 1.0; return VERTEX_C; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        bary[0] = 1.0 - w; bary[1] = 0.0; bary[2] = w;
        return EDGE_AC;
    }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
        const double w = e43 / (e43 + e56);
        bary[0] = 0.0; bary[1] = 1.0 - w; bary[2] = w;
        return EDGE_BC;
    }
    const double s = (va + vb) + vc;
    const double v = vb / s, w = vc / s;
    bary[0] = (1.0 - v) - w; bary[1] = v; bary[2] = w;
    return FACE;
}

// the squared distance of p to the point the barycentrics name
MORIG_POINTTRI_HD double bary_dist2(const double* p, const double* a, const double* b, const double* c, const double* bary) {
    double q[3];
    for (int k = 0; k < 3; ++k) q[k] = (bary[0] * a[k] + bary[1] * b[k]) + bary[2] * c[k];
    return dist2(p, q);
}

// The winner over the n triangles tri [n][9] = (a, b, c) in ascending order under a strict `<` from +inf: the smallest squared distance,
// the lowest face among equals; -1 (bary and d2 untouched) when no triangle has a distance below +inf. The serial form of the kernel.
inline int closest_face_serial(const double* p, const double* tri, int n, double* bary, double* d2, int* region) {
    int best = -1;
    double bd = __builtin_inf();
    for (int f = 0; f < n; ++f) {
        double bb[3];
        const double* t = tri + (long long)f * 9;
        const int r = closest_bary(p, t, t + 3, t + 6, bb);
        const double d = bary_dist2(p, t, t + 3, t + 6, bb);
        if (d < bd) { bd = d; best = f; bary[0] = bb[0]; bary[1] = bb[1]; bary[2] = bb[2]; *region = r; }
    }
    if (best >= 0) *d2 = bd;
    return best;
}

}  // namespace morig_pointtri
