// The mesh BVH (morig_amd/spatial.py): a 64-wide implicit tree per mesh of a ragged batch, built on the device
// without pointers, two queries on it that return what the brute-force kernels return -- morig_ray_cast (labels.hip) and
// morig_transfer_closest (transfer.hip) -- bit for bit, and the any-hit test of segments. Everything is float64 in the written order of operations (contraction off) or
// integer; the only atomic is the integer OR into a status word or a mesh's flag word: two runs give the same bits, and a mesh alone
// gives the bits it gives inside a batch.
//
// keys        one thread per face: mesh << 30 | the 30-bit Morton code of the centroid in the mesh's cubic frame (bvh_core.h). The host
//             sorts them with a stable sort: `order` maps a sorted position to its row of `faces`.
// boxes       one wave per node, one launch per level. Level 1: lane i takes the box of sorted face 64 n + i of the node's mesh; level
//             k: the box of node 64 n + i of level k - 1. A butterfly of __shfl_xor takes the minimum and the maximum, which do not round:
//             a node's box is a function of its faces alone. Face indices are clamped into the mesh's vertex block as the brute-force
//             kernels clamp them, and MORIG_BVH_BAD_FACE is ORed into the mesh's flag word, which the queries hand on to their status.
// queries     one wave per query. At a node every lane tests one child box (bvh_core.h: ray_skips / point_skips) and a ballot gives the
//             children to enter; the pending children of the at most four levels are wave-uniform 64-bit masks in named scalars and the
//             bound of every pending child stays in its lane, so there is no stack and no runtime-indexed private array. The pending
//             child with the smallest bound (the lowest child among equals) is entered next, unless the best has improved past its bound
//             in the meantime. At a leaf every lane tests one face through raytri_core.h / pointtri_core.h and the butterfly takes the
//             lexicographic minimum of (value, face) together with the running best: ties go to the lowest face whatever the visiting
//             order. A level above a mesh's top level has the single child 0, entered untested. A segment query keeps t_max as its
//             bound and ends with the first leaf that holds a hit.
// visibility  two more rules on the same walk. The scan rule of csrc/scan.hip: one wave per (view, vertex) over the
//             VIEW TREE of its view -- the view's own vertex rows, the faces and the order of the view's mesh, boxes per view -- as an
//             any-hit walk with the bound 1. The vertex-to-bone rule of csrc/geodesic.hip (bonevis_core.h): one wave per (vertex, bone)
//             over the occluder's tree, the nearest hit on t, boxes padded by 2^-36 of the scale, ended early by a hit that decides.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the rule headers: the pragma holds from here on

#include "bonevis_core.h"
#include "bvh_core.h"
#include "pointtri_core.h"
#include "raytri_core.h"

namespace morig {

namespace {

using morig_raytri::Num;
constexpr int NO_FACE = 0x7fffffff;
constexpr int LEVELS = morig_bvh::MAX_LEVELS;

// the corners of face row f of a mesh with nv >= 1 vertices from row v0; true when an index had to be clamped
__device__ __forceinline__ bool load_face(const double* __restrict__ verts, const int* __restrict__ faces, int v0, int nv, size_t f, double (*P)[3]) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int raw = faces[f * 3 + k];
        const int id = min(max(raw, 0), nv - 1);
        bad = bad || id != raw;
#pragma unroll
        for (int c = 0; c < 3; ++c) P[k][c] = verts[((size_t)v0 + id) * 3 + c];
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------------------------------ keys
__global__ void __launch_bounds__(256) bvh_keys_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                       int n_faces, const int* __restrict__ fptr, int n_meshes, const double* __restrict__ bbox,
                                                       long long* __restrict__ keys) {
    const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    const int v0 = vptr[b], nv = vptr[b + 1] - v0;
    unsigned code = 0u;
    if (nv >= 1) {
        double P[3][3], box[6];
        load_face(verts, faces, v0, nv, (size_t)f, P);
#pragma unroll
        for (int c = 0; c < 6; ++c) box[c] = bbox[(size_t)b * 6 + c];
        code = morig_bvh::morton30(P[0], P[1], P[2], box);
    }
    keys[f] = morig_bvh::face_key(b, code);
}

// ------------------------------------------------------------------------------------------------------------------------ boxes
// node_ptr [LEVELS][n_meshes + 1]: mesh b owns the rows [node_ptr[k - 1][b], node_ptr[k - 1][b + 1]) of `boxes` at level k
__global__ void __launch_bounds__(256) bvh_boxes_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                        const int* __restrict__ fptr, int n_meshes, const int* __restrict__ order,
                                                        const int* __restrict__ node_ptr, int level, int first, int n_nodes,
                                                        double* __restrict__ boxes, int* __restrict__ flags) {
    const int w = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_nodes) return;                                                           // uniform per wave
    const int node = first + w;
    const int* mine = node_ptr + (size_t)(level - 1) * (n_meshes + 1);
    const int b = segment_of(mine, n_meshes, node);
    if (!(mine[b] <= node && node < mine[b + 1])) return;                               // a table that is not the host's: nothing is written
    const long long child = ((long long)(node - mine[b]) << 6) + lane;
    double box[6];
    morig_bvh::empty_box(box);
    bool bad = false;
    if (level == 1) {
        const int v0 = vptr[b], nv = vptr[b + 1] - v0, f0 = fptr[b], nf = fptr[b + 1] - f0;
        bad = nv < 1;
        if (child < nf && nv >= 1) {
            const int row = min(max(order[(size_t)f0 + child], f0), f0 + nf - 1);
            double P[3][3];
            bad = load_face(verts, faces, v0, nv, (size_t)row, P);
            morig_bvh::face_box(P[0], P[1], P[2], box);
        }
    } else {
        const int* below = node_ptr + (size_t)(level - 2) * (n_meshes + 1);
        if (child < below[b + 1] - below[b])
#pragma unroll
            for (int c = 0; c < 6; ++c) box[c] = boxes[((size_t)below[b] + child) * 6 + c];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        double other[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) other[c] = __shfl_xor(box[c], m, 64);
        morig_bvh::grow_box(box, other);
    }
    if (__any(bad) && lane == 0) atomicOr(flags + b, MORIG_BVH_BAD_FACE);
    if (lane < 6) {
        double v = box[0];
#pragma unroll
        for (int c = 1; c < 6; ++c) v = lane == c ? box[c] : v;
        boxes[(size_t)node * 6 + lane] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ the walk
struct Tree {
    const double* verts; const int* faces; const int* order; const double* boxes;
    int v0, nv, f0, nf;
    int base[LEVELS], count[LEVELS];           // indexed by compile-time constants only
};

__device__ __forceinline__ Tree tree_of(const double* verts, const int* vptr, const int* faces, const int* fptr, const int* order, const double* boxes,
                                        const int* node_ptr, int n_meshes, int b) {
    Tree T;
    T.verts = verts; T.faces = faces; T.order = order; T.boxes = boxes;
    T.v0 = vptr[b]; T.nv = vptr[b + 1] - T.v0; T.f0 = fptr[b];
    T.nf = T.nv >= 1 ? fptr[b + 1] - T.f0 : 0;                                          // faces of a mesh without vertices name nothing
#pragma unroll
    for (int k = 0; k < LEVELS; ++k) {
        T.base[k] = node_ptr[(size_t)k * (n_meshes + 1) + b];
        T.count[k] = node_ptr[(size_t)k * (n_meshes + 1) + b + 1] - T.base[k];
    }
    return T;
}

// the root box of a mesh with faces: the single node of its top level
__device__ __forceinline__ void root_box(const Tree& T, double* root) {
    int at = T.base[0];
#pragma unroll
    for (int k = 1; k < LEVELS; ++k) at = T.count[k] > 0 ? T.base[k] : at;
#pragma unroll
    for (int c = 0; c < 6; ++c) root[c] = T.boxes[(size_t)at * 6 + c];
}

// the children of node `parent` of level K + 1 that the query enters, as a mask; bound: every lane's own child's bound
template <int K, class Q> __device__ __forceinline__ unsigned long long children(const Tree& T, const Q& q, int parent, int lane, double& bound, int& visits) {
    bound = -INFINITY;
    if (T.count[K - 1] == 0) return 1ull;                                               // above the top level: child 0, untested
    const long long child = ((long long)parent << 6) + lane;
    const int n = (int)min(64LL, (long long)T.count[K - 1] - ((long long)parent << 6));
    visits += n;
    bool enter = false;
    if (lane < n) {
        double box[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) box[c] = T.boxes[((size_t)T.base[K - 1] + child) * 6 + c];
        enter = !q.skips(box, bound);
    }
    return __ballot(enter);
}

// takes the pending child with the smallest bound (the lowest child among equals) out of the mask; -1 once none is wanted any more
template <class Q> __device__ __forceinline__ int next_child(unsigned long long& mask, double bound, const Q& q, int lane) {
    if (mask == 0ull || q.done()) { mask = 0ull; return -1; }
    const bool pending = (mask >> lane) & 1ull;
    double key = pending ? bound : INFINITY;
    int who = pending ? lane : 64;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double ok = __shfl_xor(key, m, 64);
        const int ow = __shfl_xor(who, m, 64);
        if (ok < key || (ok == key && ow < who)) { key = ok; who = ow; }
    }
    if (!q.wanted(key)) { mask = 0ull; return -1; }                                     // every other pending bound is at least this one
    mask &= ~(1ull << who);
    return who;
}

template <class Q> __device__ __forceinline__ void walk(const Tree& T, Q& q, int lane, int& visits) {
    if (T.nf <= 0) return;
    double b4, b3, b2, b1;
    unsigned long long m4 = children<4>(T, q, 0, lane, b4, visits), m3, m2, m1;
    for (int c4 = next_child(m4, b4, q, lane); c4 >= 0; c4 = next_child(m4, b4, q, lane)) {
        m3 = children<3>(T, q, c4, lane, b3, visits);
        for (int c3 = next_child(m3, b3, q, lane); c3 >= 0; c3 = next_child(m3, b3, q, lane)) {
            const int i3 = (c4 << 6) + c3;
            m2 = children<2>(T, q, i3, lane, b2, visits);
            for (int c2 = next_child(m2, b2, q, lane); c2 >= 0; c2 = next_child(m2, b2, q, lane)) {
                const int i2 = (i3 << 6) + c2;
                m1 = children<1>(T, q, i2, lane, b1, visits);
                for (int c1 = next_child(m1, b1, q, lane); c1 >= 0; c1 = next_child(m1, b1, q, lane)) {
                    const long long first = ((long long)((i2 << 6) + c1)) << 6;
                    const int n = (int)min(64LL, (long long)T.nf - first);
                    visits += n;
                    int f = NO_FACE;
                    double value = INFINITY;
                    if (lane < n) {
                        const int row = min(max(T.order[(size_t)T.f0 + first + lane], T.f0), T.f0 + T.nf - 1);
                        double P[3][3];
                        load_face(T.verts, T.faces, T.v0, T.nv, (size_t)row, P);
                        if (q.face(T.faces + (size_t)row * 3, T.nv, P, value)) f = row - T.f0; else value = INFINITY;
                    }
                    if (q.best < value || (q.best == value && q.best_face < f)) { value = q.best; f = q.best_face; }
#pragma unroll
                    for (int m = 32; m > 0; m >>= 1) {
                        const double ov = __shfl_xor(value, m, 64);
                        const int of = __shfl_xor(f, m, 64);
                        if (ov < value || (ov == value && of < f)) { value = ov; f = of; }
                    }
                    q.best = value; q.best_face = f;
                }
            }
        }
    }
}

struct RayQuery {
    double o[3], d[3], scale, best;
    int best_face;
    __device__ __forceinline__ bool skips(const double* box, double& bound) const { return morig_bvh::ray_skips(o, d, box, scale, best, bound); }
    __device__ __forceinline__ bool wanted(double bound) const { return morig_bvh::ray_wanted(bound, best); }
    __device__ __forceinline__ bool done() const { return false; }
    __device__ __forceinline__ bool face(const int*, int, const double (*P)[3], double& t) const {     // t = +inf never wins
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
        return morig_raytri::hit(n, 0.0, t) && t < INFINITY;
    }
};

// any hit below t_max on a face that does not name `skip`: best starts at t_max, so the boxes beyond it are skipped, and the walk ends
// with the first leaf that holds a hit
struct SegmentQuery {
    double o[3], d[3], scale, best, t_max;
    int best_face, skip;
    __device__ __forceinline__ bool skips(const double* box, double& bound) const { return morig_bvh::ray_skips(o, d, box, scale, t_max, bound); }
    __device__ __forceinline__ bool wanted(double bound) const { return morig_bvh::ray_wanted(bound, t_max); }
    __device__ __forceinline__ bool done() const { return best_face != NO_FACE; }
    __device__ __forceinline__ bool face(const int* ids, int nv, const double (*P)[3], double& t) const {
        if (skip >= 0)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (min(max(ids[k], 0), nv - 1) == skip) return false;
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
        return morig_raytri::hit(n, 0.0, t) && t < t_max;
    }
};

struct PointQuery {
    double p[3], slack, best;
    int best_face;
    __device__ __forceinline__ bool skips(const double* box, double& bound) const { return morig_bvh::point_skips(p, box, slack, best, bound); }
    __device__ __forceinline__ bool wanted(double bound) const { return morig_bvh::point_wanted(bound, slack, best); }
    __device__ __forceinline__ bool done() const { return false; }
    __device__ __forceinline__ bool face(const int*, int, const double (*P)[3], double& d2) const {    // a NaN or +inf distance never wins
        double bary[3];
        morig_pointtri::closest_bary(p, P[0], P[1], P[2], bary);
        d2 = morig_pointtri::bary_dist2(p, P[0], P[1], P[2], bary);
        return d2 < INFINITY;
    }
};

// ------------------------------------------------------------------------------------------------------------------------ rays
__global__ void __launch_bounds__(256) bvh_ray_cast_kernel(const double* __restrict__ origins, const double* __restrict__ dirs, const int* __restrict__ ray_ptr,
                                                           int n_rays, const double* __restrict__ verts, const int* __restrict__ vptr,
                                                           const int* __restrict__ faces, const int* __restrict__ fptr, int n_meshes,
                                                           const int* __restrict__ order, const double* __restrict__ boxes,
                                                           const int* __restrict__ node_ptr, const int* __restrict__ flags, int orientation,
                                                           double* __restrict__ t_out, int* __restrict__ face_out, double* __restrict__ point,
                                                           int* __restrict__ visits_out, int* __restrict__ status) {
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rays) return;                                                            // uniform per wave
    const int b = segment_of(ray_ptr, n_meshes, r);
    const bool owned = ray_ptr[b] <= r && r < ray_ptr[b + 1];
    Tree T = tree_of(verts, vptr, faces, fptr, order, boxes, node_ptr, n_meshes, b);
    const bool bad = !owned || (fptr[b + 1] - T.f0 > 0 && (T.nv < 1 || (flags[b] & MORIG_BVH_BAD_FACE)));
    if (!owned) T.nf = 0;
    RayQuery q;
#pragma unroll
    for (int c = 0; c < 3; ++c) { q.o[c] = origins[(size_t)r * 3 + c]; q.d[c] = dirs[(size_t)r * 3 + c]; }
    q.best = INFINITY; q.best_face = NO_FACE; q.scale = 0.0;
    int visits = 0;
    if (T.nf > 0) {
        double root[6];
        root_box(T, root);
        q.scale = morig_bvh::query_scale(q.o, root);
    }
    walk(T, q, lane, visits);
    if (lane != 0) return;
    if (bad) atomicOr(status, !owned ? MORIG_RAY_BAD_TABLE : MORIG_RAY_BAD_FACE);
    double best = q.best, p[3] = {NAN, NAN, NAN};
    int bf = q.best_face;
    if (bf != NO_FACE) {
        double P[3][3];
        load_face(verts, faces, T.v0, T.nv, (size_t)T.f0 + bf, P);
        const Num n = morig_raytri::numerators(q.o, q.d, P[0], P[1], P[2]);             // the bits the owning lane saw
        const bool wrong = (orientation > 0 && !(n.det < 0.0)) || (orientation < 0 && !(n.det > 0.0));
        if (wrong) { best = INFINITY; bf = NO_FACE; }
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = q.o[c] + best * q.d[c];
        }
    }
    t_out[r] = bf != NO_FACE ? best : INFINITY;
    face_out[r] = bf != NO_FACE ? bf : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) point[(size_t)r * 3 + c] = p[c];
    if (visits_out) visits_out[r] = visits;
}

// ------------------------------------------------------------------------------------------------------------------------ closest points
__global__ void __launch_bounds__(256) bvh_closest_kernel(const double* __restrict__ pts, const int* __restrict__ pptr, int n_pts,
                                                          const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                          const int* __restrict__ fptr, int n_meshes, const int* __restrict__ order,
                                                          const double* __restrict__ boxes, const int* __restrict__ node_ptr,
                                                          const int* __restrict__ flags, int* __restrict__ face_out, double* __restrict__ bary_out,
                                                          double* __restrict__ dist_out, int* __restrict__ visits_out, int* __restrict__ status) {
    const int i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_pts) return;                                                             // uniform per wave
    const int b = segment_of(pptr, n_meshes, i);
    if (!(pptr[b] <= i && i < pptr[b + 1])) return;                                     // a table that is not the host's: nothing is written
    const Tree T = tree_of(verts, vptr, faces, fptr, order, boxes, node_ptr, n_meshes, b);
    const bool bad = fptr[b + 1] - T.f0 > 0 && (T.nv < 1 || (flags[b] & MORIG_BVH_BAD_FACE));
    PointQuery q;
#pragma unroll
    for (int c = 0; c < 3; ++c) q.p[c] = pts[(size_t)i * 3 + c];
    q.best = INFINITY; q.best_face = NO_FACE; q.slack = 0.0;
    int visits = 0;
    if (T.nf > 0) {
        double root[6];
        root_box(T, root);
        q.slack = morig_bvh::point_slack(morig_bvh::query_scale(q.p, root));
    }
    walk(T, q, lane, visits);
    if (lane != 0) return;
    if (bad) atomicOr(status, MORIG_TRANSFER_BAD_FACE);
    if (T.nf == 0) atomicOr(status, MORIG_TRANSFER_NO_FACES);
    double bary[3] = {NAN, NAN, NAN};
    if (q.best_face != NO_FACE) {
        double P[3][3];
        load_face(verts, faces, T.v0, T.nv, (size_t)T.f0 + q.best_face, P);
        morig_pointtri::closest_bary(q.p, P[0], P[1], P[2], bary);                      // the bits the owning lane saw
    }
    face_out[i] = q.best_face != NO_FACE ? q.best_face : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) bary_out[(size_t)i * 3 + c] = bary[c];
    dist_out[i] = q.best_face != NO_FACE ? sqrt(q.best) : NAN;
    if (visits_out) visits_out[i] = visits;
}

// ------------------------------------------------------------------------------------------------------------------------ segments
__global__ void __launch_bounds__(256) bvh_blocked_kernel(const double* __restrict__ a, const double* __restrict__ b_end, const int* __restrict__ seg_ptr,
                                                          int n_segs, const int* __restrict__ skip_vertex, const double* __restrict__ t_max,
                                                          const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                          const int* __restrict__ fptr, int n_meshes, const int* __restrict__ order,
                                                          const double* __restrict__ boxes, const int* __restrict__ node_ptr,
                                                          const int* __restrict__ flags, unsigned char* __restrict__ blocked,
                                                          int* __restrict__ visits_out, int* __restrict__ status) {
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_segs) return;                                                            // uniform per wave
    const int b = segment_of(seg_ptr, n_meshes, r);
    const bool owned = seg_ptr[b] <= r && r < seg_ptr[b + 1];
    Tree T = tree_of(verts, vptr, faces, fptr, order, boxes, node_ptr, n_meshes, b);
    const bool bad = !owned || (fptr[b + 1] - T.f0 > 0 && (T.nv < 1 || (flags[b] & MORIG_BVH_BAD_FACE)));
    if (!owned) T.nf = 0;
    SegmentQuery q;
#pragma unroll
    for (int c = 0; c < 3; ++c) { q.o[c] = a[(size_t)r * 3 + c]; q.d[c] = b_end[(size_t)r * 3 + c] - q.o[c]; }
    q.t_max = t_max ? t_max[r] : 1.0;
    q.skip = skip_vertex ? skip_vertex[r] : -1;
    q.best = q.t_max; q.best_face = NO_FACE; q.scale = 0.0;
    int visits = 0;
    if (T.nf > 0) {
        double root[6];
        root_box(T, root);
        q.scale = morig_bvh::query_scale(q.o, root);
    }
    walk(T, q, lane, visits);
    if (lane != 0) return;
    if (bad) atomicOr(status, !owned ? MORIG_RAY_BAD_TABLE : MORIG_RAY_BAD_FACE);
    blocked[r] = q.best_face != NO_FACE ? 1 : 0;
    if (visits_out) visits_out[r] = visits;
}

// ------------------------------------------------------------------------------------------------------------------------ view trees
// A tree per VIEW of a scan (csrc/scan.hip): the vertex rows are the view's, the faces and their order are those of the view's mesh.
// node_ptr [LEVELS][n_views + 1]: view v owns the rows [node_ptr[k - 1][v], node_ptr[k - 1][v + 1]) of `boxes` at level k. The boxes are
// exact for the view's own vertices whatever pose ordered the faces, so only the pruning depends on the order.
__global__ void __launch_bounds__(256) bvh_view_boxes_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ view_mesh,
                                                             int n_views, const int* __restrict__ faces, const int* __restrict__ fptr, int n_meshes,
                                                             const int* __restrict__ order, const int* __restrict__ node_ptr, int level, int first,
                                                             int n_nodes, double* __restrict__ boxes, int* __restrict__ flags) {
    const int w = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_nodes) return;                                                           // uniform per wave
    const int node = first + w;
    const int* mine = node_ptr + (size_t)(level - 1) * (n_views + 1);
    const int v = segment_of(mine, n_views, node);
    if (!(mine[v] <= node && node < mine[v + 1])) return;                               // a table that is not the host's: nothing is written
    const long long child = ((long long)(node - mine[v]) << 6) + lane;
    double box[6];
    morig_bvh::empty_box(box);
    bool bad = false;
    if (level == 1) {
        const int m = view_mesh[v];
        const bool named = m >= 0 && m < n_meshes;                                      // a view that names no mesh draws nothing
        const int v0 = vptr[v], nv = vptr[v + 1] - v0, f0 = named ? fptr[m] : 0, nf = named ? fptr[m + 1] - f0 : 0;
        bad = nv < 1;
        if (child < nf && nv >= 1) {
            const int row = min(max(order[(size_t)f0 + child], f0), f0 + nf - 1);
            double P[3][3];
            bad = load_face(verts, faces, v0, nv, (size_t)row, P);
            morig_bvh::face_box(P[0], P[1], P[2], box);
        }
    } else {
        const int* below = node_ptr + (size_t)(level - 2) * (n_views + 1);
        if (child < below[v + 1] - below[v])
#pragma unroll
            for (int c = 0; c < 6; ++c) box[c] = boxes[((size_t)below[v] + child) * 6 + c];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        double other[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) other[c] = __shfl_xor(box[c], m, 64);
        morig_bvh::grow_box(box, other);
    }
    if (__any(bad) && lane == 0) atomicOr(flags + v, MORIG_BVH_BAD_FACE);
    if (lane < 6) {
        double x = box[0];
#pragma unroll
        for (int c = 1; c < 6; ++c) x = lane == c ? box[c] : x;
        boxes[(size_t)node * 6 + lane] = x;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ scan visibility
// The rule of scan_visibility_kernel (csrc/scan.hip) as an any-hit walk: a face blocks when it does not name the vertex and meets the
// segment from the camera point to the vertex at 0 < t < 1 with t len < len - vis_eps. The bound stays 1: an accepted face has
// 0 < t < 1, so ray_skips with best = 1 enters its box and every box above it.
struct ScanQuery {
    double o[3], d[3], scale, best, len, vis_eps;
    int best_face, self;
    __device__ __forceinline__ bool skips(const double* box, double& bound) const { return morig_bvh::ray_skips(o, d, box, scale, 1.0, bound); }
    __device__ __forceinline__ bool wanted(double bound) const { return morig_bvh::ray_wanted(bound, 1.0); }
    __device__ __forceinline__ bool done() const { return best_face != NO_FACE; }
    __device__ __forceinline__ bool face(const int* ids, int nv, const double (*P)[3], double& t) const {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (min(max(ids[k], 0), nv - 1) == self) return false;
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
        if (!morig_raytri::inside(n)) return false;
        t = n.tn / n.det;
        return t > 0.0 && t < 1.0 && t * len < len - vis_eps;
    }
};

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__global__ void __launch_bounds__(256) bvh_scan_visibility_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                                  const int* __restrict__ fptr, const double* __restrict__ cams,
                                                                  const int* __restrict__ views, int n_views, int n_meshes, int n_rows, double vis_eps,
                                                                  const int* __restrict__ order, const double* __restrict__ boxes,
                                                                  const int* __restrict__ node_ptr, const int* __restrict__ flags,
                                                                  unsigned char* __restrict__ vis, int* __restrict__ visits_out,
                                                                  int* __restrict__ status) {
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rows) return;                                                            // uniform per wave
    const int v = segment_of(vptr, n_views, r);
    if (!(vptr[v] <= r && r < vptr[v + 1])) return;                                     // a table that is not the host's: nothing is written
    const int* view = views + (size_t)v * MORIG_SCAN_VIEW_INTS;
    const int mesh = view[0], W = view[1], H = view[2], kind = view[3];
    const bool ok = mesh >= 0 && mesh < n_meshes && W >= 1 && W <= MORIG_SCAN_MAX_SIDE && H >= 1 && H <= MORIG_SCAN_MAX_SIDE &&
                    (kind == MORIG_SCAN_ORTHOGRAPHIC || kind == MORIG_SCAN_PINHOLE);
    if (!ok) {
        if (lane == 0) { vis[r] = 0; if (visits_out) visits_out[r] = 0; }
        return;
    }
    Tree T;
    T.verts = verts; T.faces = faces; T.order = order; T.boxes = boxes;
    T.v0 = vptr[v]; T.nv = vptr[v + 1] - T.v0; T.f0 = fptr[mesh]; T.nf = fptr[mesh + 1] - T.f0;      // nv >= 1: the view owns row r
#pragma unroll
    for (int k = 0; k < LEVELS; ++k) {
        T.base[k] = node_ptr[(size_t)k * (n_views + 1) + v];
        T.count[k] = node_ptr[(size_t)k * (n_views + 1) + v + 1] - T.base[k];
    }
    const double* cam = cams + (size_t)v * MORIG_SCAN_CAM_DOUBLES;
    const double* p = verts + (size_t)r * 3;
    ScanQuery q;
    const double de[3] = {p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]};
    const double z = dot3(de, cam + 3);
    double a = dot3(de, cam + 6), b = dot3(de, cam + 9);
    if (kind == MORIG_SCAN_PINHOLE) { a = a / z; b = b / z; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q.o[k] = kind == MORIG_SCAN_PINHOLE ? cam[k] : p[k] - z * cam[3 + k];
        q.d[k] = p[k] - q.o[k];
    }
    q.len = sqrt((q.d[0] * q.d[0] + q.d[1] * q.d[1]) + q.d[2] * q.d[2]);
    const bool seen = z > cam[14] && fabs(a) <= (double)W * cam[12] && fabs(b) <= (double)H * cam[13];
    q.vis_eps = vis_eps; q.self = r - T.v0;
    q.best = 1.0; q.best_face = NO_FACE; q.scale = 0.0;
    int visits = 0;
    if (seen) {                                                                         // outside the frustum: nothing is walked
        if (T.nf > 0) {
            double root[6];
            root_box(T, root);
            q.scale = morig_bvh::query_scale(q.o, root);
        }
        walk(T, q, lane, visits);
    }
    if (lane != 0) return;
    if (T.nf > 0 && (flags[v] & MORIG_BVH_BAD_FACE)) atomicOr(status, MORIG_SCAN_BAD_FACE);
    vis[r] = seen && q.best_face == NO_FACE ? 1 : 0;
    if (visits_out) visits_out[r] = visits;
}

// ------------------------------------------------------------------------------------------------------------------------ bone visibility
// The rule of bone_visibility_kernel (csrc/geodesic.hip, restated in bonevis_core.h) as a nearest-hit walk on t over the occluder's tree.
// h(t) does not decrease with t, so the smallest hit distance is that of the smallest t; the walk ends as soon as a hit decides the ray
// as invisible (bonevis_core.h decides). The boxes are padded by BONE_SLACK of the query's scale: an accepted hit may lie outside its
// triangle by the rule's 1e-12 tolerances.
struct BoneQuery {
    morig_bonevis::Ray ray;
    double scale, best;
    int best_face;
    __device__ __forceinline__ bool skips(const double* box, double& bound) const {
        return morig_bvh::ray_skips(ray.o, ray.d, box, scale, best, bound, morig_bvh::BONE_SLACK);
    }
    __device__ __forceinline__ bool wanted(double bound) const { return morig_bvh::ray_wanted(bound, best); }
    __device__ __forceinline__ bool done() const { return best_face != NO_FACE && morig_bonevis::decides(morig_bonevis::hit_distance(ray, best), ray.len); }
    __device__ __forceinline__ bool face(const int*, int, const double (*P)[3], double& t) const {      // t = +inf never wins: its h is no minimum
        return morig_bonevis::hit(ray, P[0], P[1], P[2], t) && t < INFINITY;
    }
};

__global__ void __launch_bounds__(256) bvh_bone_visibility_kernel(const double* __restrict__ pos, const int* __restrict__ vtx_ptr, const double* __restrict__ bones,
                                                                  const int* __restrict__ bone_ptr, const double* __restrict__ tri_pos,
                                                                  const int* __restrict__ tp_ptr, const int* __restrict__ faces,
                                                                  const int* __restrict__ f_ptr, const long long* __restrict__ off, int n_meshes,
                                                                  long long n_pairs, const int* __restrict__ order, const double* __restrict__ boxes,
                                                                  const int* __restrict__ node_ptr, const int* __restrict__ flags,
                                                                  unsigned char* __restrict__ vis, int* __restrict__ visits_out, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_pairs) return;                                                           // uniform per wave
    const int b = segment_of(off, n_meshes, i);
    const int v0 = vtx_ptr[b], nv = vtx_ptr[b + 1] - v0, c0 = bone_ptr[b], nb = bone_ptr[b + 1] - c0;
    const long long k = i - off[b];
    if (!(off[b] <= i && i < off[b + 1]) || nb < 1 || k >= (long long)nv * nb) return;  // a table that is not the host's: nothing is written
    const Tree T = tree_of(tri_pos, tp_ptr, faces, f_ptr, order, boxes, node_ptr, n_meshes, b);
    BoneQuery q;
    q.ray = morig_bonevis::ray_of(pos + (size_t)(v0 + (int)(k / nb)) * 3, bones + (size_t)(c0 + (int)(k % nb)) * 6);
    q.best = INFINITY; q.best_face = NO_FACE; q.scale = 0.0;
    int visits = 0;
    if (T.nf > 0) {
        double root[6];
        root_box(T, root);
        q.scale = morig_bvh::query_scale(q.ray.o, root);
    }
    walk(T, q, lane, visits);
    if (lane != 0) return;
    if (T.nf > 0 && (flags[b] & MORIG_BVH_BAD_FACE)) atomicOr(status, MORIG_BVH_BAD_FACE);
    const double h = q.best_face != NO_FACE ? morig_bonevis::hit_distance(q.ray, q.best) : INFINITY;
    vis[i] = morig_bonevis::visible(h, q.ray.len) ? 1 : 0;
    if (visits_out) visits_out[i] = visits;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_bvh_build_keys(const double* verts, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr, int32_t n_meshes,
                         const double* bbox, int64_t* keys, void* stream) {
    if (n_faces < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!vptr || !faces || !fptr || !bbox || !keys || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_BVH_BUILD, s, 0.0, 0.0);
    bvh_keys_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(verts, vptr, faces, n_faces, fptr, n_meshes, bbox, (long long*)keys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bvh_boxes(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t n_meshes, int64_t max_faces,
                    const int32_t* order, const int32_t* node_ptr, int32_t n1, int32_t n2, int32_t n3, int32_t n4, double* boxes, int32_t* flags,
                    void* stream) {
    if (n_meshes < 0 || max_faces < 0 || n1 < 0 || n2 < 0 || n3 < 0 || n4 < 0) return MORIG_E_INVALID;
    if (max_faces > MORIG_BVH_MAX_FACES) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0) return MORIG_OK;
    if (!flags) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n_meshes, s));
    if (n1 == 0) return MORIG_OK;
    if (!vptr || !faces || !fptr || !order || !node_ptr || !boxes) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_BUILD, s, 0.0, 0.0);
    const int32_t n[LEVELS] = {n1, n2, n3, n4};
    int first = 0;
    for (int level = 1; level <= LEVELS && n[level - 1] > 0; ++level) {
        bvh_boxes_kernel<<<cdiv(n[level - 1], 4), 256, 0, s>>>(verts, vptr, faces, fptr, n_meshes, order, node_ptr, level, first, n[level - 1], boxes,
                                                               flags);
        MORIG_LAUNCH_CHECK();
        first += n[level - 1];
    }
    return MORIG_OK;
}

int morig_bvh_ray_cast(const double* origins, const double* dirs, const int32_t* ray_ptr, int32_t n_rays, const double* verts, const int32_t* vptr,
                       const int32_t* faces, const int32_t* fptr, int32_t n_meshes, const int32_t* order, const double* boxes,
                       const int32_t* node_ptr, const int32_t* flags, int32_t orientation, double* t, int32_t* face, double* point, int32_t* visits,
                       int32_t* status, void* stream) {
    if (n_rays < 0 || n_meshes < 0 || orientation < -1 || orientation > 1 || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_rays == 0) return MORIG_OK;
    if (!origins || !dirs || !ray_ptr || !vptr || !fptr || !node_ptr || !flags || !t || !face || !point || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_QUERY, s, 0.0, 0.0);
    bvh_ray_cast_kernel<<<cdiv(n_rays, 4), 256, 0, s>>>(origins, dirs, ray_ptr, n_rays, verts, vptr, faces, fptr, n_meshes, order, boxes, node_ptr,
                                                        flags, orientation, t, face, point, visits, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bvh_closest(const double* points, const int32_t* pptr, int32_t n_points, const double* verts, const int32_t* vptr, const int32_t* faces,
                      const int32_t* fptr, int32_t n_meshes, const int32_t* order, const double* boxes, const int32_t* node_ptr,
                      const int32_t* flags, int32_t* face, double* bary, double* distance, int32_t* visits, int32_t* status, void* stream) {
    if (n_points < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (n_points == 0) return MORIG_OK;
    if (!points || !pptr || !vptr || !fptr || !node_ptr || !flags || !face || !bary || !distance || !status || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_BVH_QUERY, s, 0.0, 0.0);
    bvh_closest_kernel<<<cdiv(n_points, 4), 256, 0, s>>>(points, pptr, n_points, verts, vptr, faces, fptr, n_meshes, order, boxes, node_ptr, flags,
                                                         face, bary, distance, visits, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bvh_blocked(const double* a, const double* b, const int32_t* seg_ptr, int32_t n_segments, const int32_t* skip_vertex, const double* t_max,
                      const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t n_meshes, const int32_t* order,
                      const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* blocked, int32_t* visits, int32_t* status,
                      void* stream) {
    if (n_segments < 0 || n_meshes < 0 || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_segments == 0) return MORIG_OK;
    if (!a || !b || !seg_ptr || !vptr || !fptr || !node_ptr || !flags || !blocked || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_QUERY, s, 0.0, 0.0);
    bvh_blocked_kernel<<<cdiv(n_segments, 4), 256, 0, s>>>(a, b, seg_ptr, n_segments, skip_vertex, t_max, verts, vptr, faces, fptr, n_meshes, order,
                                                           boxes, node_ptr, flags, blocked, visits, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bvh_view_boxes(const double* verts, const int32_t* vptr, const int32_t* view_mesh, int32_t n_views, const int32_t* faces, const int32_t* fptr,
                         int32_t n_meshes, int64_t max_faces, const int32_t* order, const int32_t* node_ptr, int32_t n1, int32_t n2, int32_t n3,
                         int32_t n4, double* boxes, int32_t* flags, void* stream) {
    if (n_views < 0 || n_meshes < 0 || max_faces < 0 || n1 < 0 || n2 < 0 || n3 < 0 || n4 < 0) return MORIG_E_INVALID;
    if (max_faces > MORIG_BVH_MAX_FACES) return MORIG_E_UNSUPPORTED;
    if (n_views == 0) return MORIG_OK;
    if (!flags) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)n_views, s));
    if (n1 == 0) return MORIG_OK;
    if (!vptr || !view_mesh || !faces || !fptr || !order || !node_ptr || !boxes || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_BUILD, s, 0.0, 0.0);
    const int32_t n[LEVELS] = {n1, n2, n3, n4};
    int first = 0;
    for (int level = 1; level <= LEVELS && n[level - 1] > 0; ++level) {
        bvh_view_boxes_kernel<<<cdiv(n[level - 1], 4), 256, 0, s>>>(verts, vptr, view_mesh, n_views, faces, fptr, n_meshes, order, node_ptr, level, first,
                                                                    n[level - 1], boxes, flags);
        MORIG_LAUNCH_CHECK();
        first += n[level - 1];
    }
    return MORIG_OK;
}

int morig_bvh_scan_visibility(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams,
                              const int32_t* views, int32_t n_views, int32_t n_meshes, int32_t n_rows, double vis_eps, const int32_t* order,
                              const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* vis, int32_t* visits, int32_t* status,
                              void* stream) {
    if (n_views < 0 || n_meshes < 0 || n_rows < 0 || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_rows == 0) return MORIG_OK;
    if (!verts || !vptr || !fptr || !cams || !views || !node_ptr || !flags || !vis || n_views == 0 || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_QUERY, s, 0.0, 0.0);
    bvh_scan_visibility_kernel<<<cdiv(n_rows, 4), 256, 0, s>>>(verts, vptr, faces, fptr, cams, views, n_views, n_meshes, n_rows, vis_eps, order, boxes,
                                                               node_ptr, flags, vis, visits, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bvh_bone_visibility(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, const double* tri_pos,
                              const int32_t* tp_ptr, const int32_t* faces, const int32_t* f_ptr, const int64_t* off, int32_t n_meshes, int64_t n_pairs,
                              const int32_t* order, const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* vis, int32_t* visits,
                              int32_t* status, void* stream) {
    if (n_meshes < 0 || n_pairs < 0 || !status) return MORIG_E_INVALID;
    if (n_pairs > (((int64_t)1 << 31) - 1) * 4) return MORIG_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_pairs == 0) return MORIG_OK;
    if (!pos || !vtx_ptr || !bones || !bone_ptr || !tp_ptr || !f_ptr || !off || !node_ptr || !flags || !vis || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_BVH_QUERY, s, 0.0, 0.0);
    bvh_bone_visibility_kernel<<<cdiv(n_pairs, 4), 256, 0, s>>>(pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr, (const long long*)off, n_meshes,
                                                                (long long)n_pairs, order, boxes, node_ptr, flags, vis, visits, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
