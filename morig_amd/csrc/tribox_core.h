// Triangle against voxel, the surface rule of csrc/meshprep.hip, shared with the host program
// tools/tribox_host_check.cpp so that it can be checked without a device and under the host sanitizers.
//
// A triangle, as a closed set, overlaps the closed cube [i, i + 1] x [j, j + 1] x [k, k + 1] when none of 13 axes separates them: the
// three box axes, the triangle's normal, and the nine cross products of a triangle edge with a box axis. On an axis a the triangle spans
// [min a.v, max a.v] (vertices relative to the cube's centre) and the cube [-r, r] with r = (|ax| + |ay| + |az|) / 2; the axis separates
// when min > r or max < -r -- strictly, so touching counts. A zero axis (a degenerate triangle's normal, an edge parallel to a box
// axis, a zero edge) gives min = max = r = 0 and separates nothing: such triangles are decided by the axes they have left.
// All float64, every operation in the written order (the including file switches contraction off). With vertices on integer or
// half-integer grid coordinates every quantity here is exact.
#pragma once

#if defined(__HIPCC__)
#define MORIG_TRIBOX_HD __host__ __device__ __forceinline__
#else
#define MORIG_TRIBOX_HD inline
#endif

namespace morig_tribox {

struct Tri {
    double v[3][3];     // the vertices in grid coordinates
    double a[10][3];    // the normal, then edge e x unit axis u at 1 + 3 e + u
};

MORIG_TRIBOX_HD double absd(double x) { return x < 0.0 ? -x : x; }

// the axes of a triangle: they do not depend on the voxel
MORIG_TRIBOX_HD void prepare(const double* p0, const double* p1, const double* p2, Tri& t) {
    for (int c = 0; c < 3; ++c) { t.v[0][c] = p0[c]; t.v[1][c] = p1[c]; t.v[2][c] = p2[c]; }
    double e[3][3];
    for (int c = 0; c < 3; ++c) { e[0][c] = p1[c] - p0[c]; e[1][c] = p2[c] - p1[c]; e[2][c] = p0[c] - p2[c]; }
    t.a[0][0] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
    t.a[0][1] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
    t.a[0][2] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    for (int k = 0; k < 3; ++k) {
        double* ax = t.a[1 + 3 * k];
        double* ay = t.a[2 + 3 * k];
        double* az = t.a[3 + 3 * k];
        ax[0] = 0.0;       ax[1] = e[k][2];   ax[2] = -e[k][1];   // e x (1, 0, 0)
        ay[0] = -e[k][2];  ay[1] = 0.0;       ay[2] = e[k][0];    // e x (0, 1, 0)
        az[0] = e[k][1];   az[1] = -e[k][0];  az[2] = 0.0;        // e x (0, 0, 1)
    }
}

MORIG_TRIBOX_HD bool overlaps(const Tri& t, int i, int j, int k) {
    const double c[3] = {(double)i + 0.5, (double)j + 0.5, (double)k + 0.5};
    double r[3][3];
    for (int n = 0; n < 3; ++n)
        for (int d = 0; d < 3; ++d) r[n][d] = t.v[n][d] - c[d];
    for (int d = 0; d < 3; ++d) {                                                     // the box axes
        double lo = r[0][d], hi = r[0][d];
        for (int n = 1; n < 3; ++n) { lo = r[n][d] < lo ? r[n][d] : lo; hi = r[n][d] > hi ? r[n][d] : hi; }
        if (lo > 0.5 || hi < -0.5) return false;
    }
    for (int x = 0; x < 10; ++x) {                                                    // the normal and the nine edge axes
        const double* a = t.a[x];
        const double rad = 0.5 * ((absd(a[0]) + absd(a[1])) + absd(a[2]));
        double lo = 0.0, hi = 0.0;
        for (int n = 0; n < 3; ++n) {
            const double p = (a[0] * r[n][0] + a[1] * r[n][1]) + a[2] * r[n][2];
            lo = (n == 0 || p < lo) ? p : lo;
            hi = (n == 0 || p > hi) ? p : hi;
        }
        if (lo > rad || hi < -rad) return false;
    }
    return true;
}

}  // namespace morig_tribox
