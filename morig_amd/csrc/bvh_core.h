// The 64-wide implicit mesh BVH (csrc/bvh.hip, morig_amd/spatial.py): the Morton key of a face, the level table,
// the box of a face and the two ENTERING rules, shared with the host program tools/bvh_host_check.cpp so that they can be checked
// without a device and under the host sanitizers. All float64, every operation in the written order (the including file switches
// contraction off). A box is six doubles: minimum x, y, z, maximum x, y, z; the EMPTY box is (+inf, +inf, +inf, -inf, -inf, -inf).
//
// Key.      c = ((A + B) + C) / 3 per coordinate; per axis q = (c - lo) / ext * 1024, cell = min((int)floor(q), 1023) clamped to
//           [0, 1023], with lo the minimum of the mesh's bounding box and ext its largest extent; the cells interleave into 30 bits with
//           x highest (bit 3 i + 2 = x_i, 3 i + 1 = y_i, 3 i = z_i). The code is 0 where ext is not > 0 or a centroid coordinate is no
//           finite number. key = mesh << 30 | code.
// Levels.   n_1 = ceil(faces / 64), n_k = ceil(n_(k-1) / 64) while n_(k-1) > 1: at most MAX_LEVELS = 4, so at most 64^4 faces.
// Face box. The exact minimum and maximum of the three corners; EMPTY when a corner coordinate is NaN (such a face never wins: its
//           ray numerators and its squared distance are NaN). An infinite coordinate stays in the box: the point rule can still return a
//           finite corner of such a face.
// Entering. Both rules take `scale`, a bound on |q - x| (1-norm) over the points x of the mesh's root box for the query point q (the ray
//           origin): scale = (the root's extents added) + |q - centre|_1. A comparison that a NaN reaches is false, and every `skip` is a
//           conjunction of such comparisons' results: a NaN always ENTERS.
//   ray     pad = 2^-40 scale. Per axis with d_k != 0 the parameters at which o + t d crosses lo_k - pad and hi_k + pad, taken as (near,
//           far) by the sign of d_k (an EMPTY box has near > far); with d_k == 0 the box is missed when o_k lies outside
//           [lo_k - pad, hi_k + pad]. tmin = the largest near, tmax = the smallest far; tmin is deflated and tmax inflated by 2^-40 of
//           their magnitude. Skip when missed, tmin > tmax, tmax < 0 or tmin > best. The bound handed back is the deflated tmin.
//           The pad's share of scale is a parameter: 2^-40 by default, BONE_SLACK = 2^-36 for the vertex-to-bone rule of bonevis_core.h,
//           whose accepted hits may lie 1e-12 (|e1_k| + |e2_k|) <= 2e-12 scale outside their triangle per coordinate.
//   point   e_k = max(lo_k - p_k, p_k - hi_k, 0), bound = (e_x^2 + e_y^2) + e_z^2. Skip when bound > best + 2^-40 scale^2.
//           `wanted` repeats the last comparison of either rule for a child that waited while the best improved.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORIG_BVH_HD __host__ __device__ __forceinline__
#else
#define MORIG_BVH_HD inline
#endif

namespace morig_bvh {

constexpr int WIDTH = 64, MAX_LEVELS = 4, MORTON_BITS = 10;
constexpr long long MAX_FACES = 64LL * 64 * 64 * 64;
constexpr double SLACK = 0x1p-40;
constexpr double BONE_SLACK = 0x1p-36;             // the pad of the vertex-to-bone rule (bonevis_core.h): its 1e-12 tolerances stay a seventh of it

MORIG_BVH_HD double inf() { return __builtin_inf(); }
MORIG_BVH_HD bool is_finite(double x) { return x - x == 0.0; }
MORIG_BVH_HD double absd(double x) { return x < 0.0 ? -x : x; }

// ---- the order
MORIG_BVH_HD int cell_of(double c, double lo, double ext) {
    const double q = (c - lo) / ext * 1024.0;
    if (!(q >= 0.0)) return 0;                       // below the box, or NaN
    if (q >= 1023.0) return 1023;
    return (int)q;                                   // floor of a value in [0, 1023)
}

MORIG_BVH_HD unsigned spread10(unsigned v) {       // bit i of v -> bit 3 i
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// bbox: the six doubles of morig_mesh_bbox for the face's mesh
MORIG_BVH_HD unsigned morton30(const double* A, const double* B, const double* C, const double* bbox) {
    double ext = bbox[3] - bbox[0];
    if (bbox[4] - bbox[1] > ext) ext = bbox[4] - bbox[1];
    if (bbox[5] - bbox[2] > ext) ext = bbox[5] - bbox[2];
    if (!(ext > 0.0) || !is_finite(ext)) return 0u;
    int cell[3];
    for (int k = 0; k < 3; ++k) {
        const double c = ((A[k] + B[k]) + C[k]) / 3.0;
        if (!is_finite(c)) return 0u;
        cell[k] = cell_of(c, bbox[k], ext);
    }
    return (spread10((unsigned)cell[0]) << 2) | (spread10((unsigned)cell[1]) << 1) | spread10((unsigned)cell[2]);
}

MORIG_BVH_HD long long face_key(int mesh, unsigned code) { return ((long long)mesh << 30) | (long long)code; }

// ---- the levels: count[k - 1] = the nodes of level k (0 above the mesh's top level); returns the number of levels, -1 above MAX_FACES
inline int level_counts(long long faces, long long* count) {
    for (int k = 0; k < MAX_LEVELS; ++k) count[k] = 0;
    if (faces > MAX_FACES) return -1;
    int levels = 0;
    long long n = faces;
    while (n > 0 && (levels == 0 || n > 1)) {
        n = (n + WIDTH - 1) / WIDTH;
        count[levels++] = n;
    }
    return levels;
}

// ---- boxes
MORIG_BVH_HD void empty_box(double* box) {
    for (int k = 0; k < 3; ++k) { box[k] = inf(); box[3 + k] = -inf(); }
}

MORIG_BVH_HD void face_box(const double* A, const double* B, const double* C, double* box) {
    bool nan = false;
    for (int k = 0; k < 3; ++k) {
        nan = nan || A[k] != A[k] || B[k] != B[k] || C[k] != C[k];
        double lo = A[k], hi = A[k];
        if (B[k] < lo) lo = B[k];
        if (C[k] < lo) lo = C[k];
        if (B[k] > hi) hi = B[k];
        if (C[k] > hi) hi = C[k];
        box[k] = lo; box[3 + k] = hi;
    }
    if (nan) empty_box(box);
}

MORIG_BVH_HD void grow_box(double* box, const double* other) {
    for (int k = 0; k < 3; ++k) {
        if (other[k] < box[k]) box[k] = other[k];
        if (other[3 + k] > box[3 + k]) box[3 + k] = other[3 + k];
    }
}

// the bound on |q - x|_1 over the root box (see above); NaN or +inf for a root that is EMPTY or unbounded: everything is entered
MORIG_BVH_HD double query_scale(const double* q, const double* root) {
    double s = 0.0;
    for (int k = 0; k < 3; ++k) s += (root[3 + k] - root[k]) + absd(q[k] - 0.5 * (root[k] + root[3 + k]));
    return s;
}

// ---- entering, rays: true = skip; bound = the deflated entry parameter (-inf where nothing bounds it)
// `slack`: the share of scale the box is padded by (SLACK for the rules of raytri_core.h, whose hits lie in their closed triangle; a rule
// that accepts a hit outside its triangle by a tolerance passes a pad above that tolerance: bvh.hip BoneQuery)
MORIG_BVH_HD bool ray_skips(const double* o, const double* d, const double* box, double scale, double best, double& bound, double slack) {
    const double pad = slack * scale;
    double tmin = -inf(), tmax = inf();
    bool missed = false;
    for (int k = 0; k < 3; ++k) {
        const double a = (box[k] - pad) - o[k], b = (box[3 + k] + pad) - o[k];
        if (d[k] == 0.0) {
            if (a > 0.0 || b < 0.0) missed = true;
            continue;
        }
        const double ta = a / d[k], tb = b / d[k];
        if (ta != ta || tb != tb) continue;          // a NaN bounds nothing
        const double near = d[k] > 0.0 ? ta : tb, far = d[k] > 0.0 ? tb : ta;
        if (near > tmin) tmin = near;
        if (far < tmax) tmax = far;
    }
    if (is_finite(tmin)) tmin = tmin - SLACK * absd(tmin);
    if (is_finite(tmax)) tmax = tmax + SLACK * absd(tmax);
    bound = tmin;
    return missed || tmin > tmax || tmax < 0.0 || tmin > best;
}

MORIG_BVH_HD bool ray_skips(const double* o, const double* d, const double* box, double scale, double best, double& bound) {
    return ray_skips(o, d, box, scale, best, bound, SLACK);
}

MORIG_BVH_HD bool ray_wanted(double bound, double best) { return !(bound > best); }

// ---- entering, points: true = skip; bound = the squared distance to the box as computed
MORIG_BVH_HD double point_slack(double scale) { return SLACK * (scale * scale); }

MORIG_BVH_HD bool point_skips(const double* p, const double* box, double slack, double best, double& bound) {
    double s[3];
    for (int k = 0; k < 3; ++k) {
        double e = 0.0;
        const double below = box[k] - p[k], above = p[k] - box[3 + k];
        if (below > e) e = below;
        if (above > e) e = above;
        s[k] = e * e;
    }
    bound = (s[0] + s[1]) + s[2];
    return bound > best + slack;
}

MORIG_BVH_HD bool point_wanted(double bound, double slack, double best) { return !(bound > best + slack); }

}  // namespace morig_bvh
