// Surface geodesics and vertex-to-bone distances: the inference-side skinning inputs the reference computes on the CPU.
//   stage 1  data_proc/common_ops.py:175-211 calc_surface_geodesic: 5-NN graph of the surface samples filtered by normals, all-pairs
//            shortest paths (scipy's dijkstra there), the 8 + euclid patch of unreachable pairs, the nearest sample of every vertex
//   stage 2  evaluate/joint2rig.py:41-68 pts2line, :307-360 calc_geodesic_matrix, :413-442 the bind loop of predict_skinning
//   stage 3  evaluate/joint2rig.py:71-94 calc_pts2bone_visible_mat (ray casting; trimesh there, brute-force Moeller-Trumbore here)
//
// Shortest paths. With non-negative weights and IEEE addition (monotone) Dijkstra's distance is the minimum over paths of the
// left-to-right float64 sum, and a label-correcting relaxation d[v] = min(d[v], d[u] + w) run to its fixed point -- in any order, in place
// or not -- reaches the same bits. So: one job = (mesh, NSRC consecutive sources); a persistent grid of 1024-thread workgroups pulls jobs
// from a counter; the NSRC distance vectors of a job live in LDS interleaved per node (d[v][s]: one 32-byte read per neighbour at
// NSRC = 4); every thread owns nodes tid, tid + 1024, ... and PULLS the minimum over their neighbours (no atomics), in place; a sweep
// that lowers nothing ends the job. In-place reads may see this sweep's or the last sweep's value of a neighbour: both are lengths of real
// paths, values only fall, and a sweep without a write read a stable state, so the fixed point is the same. The adjacency (undirected
// CSR, 8 bytes per entry: neighbour id + the float32 weight) is streamed from L2 once per sweep for the NSRC sources. A mesh with more
// than 16384 / NSRC samples keeps the vectors in a per-workgroup global buffer instead (same code, NSRC = 4).
#include "common.h"

// every value below is compared bit for bit or decides an index: products and sums round separately, as numpy does
#pragma clang fp contract(off)

namespace morig {

constexpr int SG_THREADS = 1024;
constexpr int SG_LDS_DOUBLES = 16384;                    // 128 KiB of the 160 KiB LDS
constexpr int SG_KNN = 5;
constexpr int SG_MAX_SAMPLES = 65535;
enum { SG_ERR_SWEEPS = 1, SG_ERR_SIZE = 2 };

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrt((dx * dx + dy * dy) + dz * dz);          // np.sqrt(np.sum(d ** 2, axis=-1)): (x + y) + z
}

// common_ops.py:184-194: the 5 nearest other samples of every sample (ascending distance, the smaller index first among equals), kept
// where cos(normals) > -0.5; the weight is the float64 distance rounded to float32 (lil_matrix(dtype=np.float32)). nbr = -1: filtered.
__global__ void sg_knn_kernel(const double* __restrict__ pts, const double* __restrict__ normals, const int32_t* __restrict__ s_ptr,
                              int n_meshes, int n_total, int32_t* __restrict__ nbr, float* __restrict__ nbw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const int b = segment_of(s_ptr, n_meshes, i);
    const int s0 = s_ptr[b], s1 = s_ptr[b + 1];
    const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
    double bd[SG_KNN];
    int bi[SG_KNN];
#pragma unroll
    for (int j = 0; j < SG_KNN; ++j) { bd[j] = INFINITY; bi[j] = -1; }
    for (int q = s0; q < s1; ++q) {
        if (q == i) continue;
        const double d = dist3(pts[(size_t)q * 3], pts[(size_t)q * 3 + 1], pts[(size_t)q * 3 + 2], px, py, pz);
        if (d < bd[SG_KNN - 1]) {
            bd[SG_KNN - 1] = d; bi[SG_KNN - 1] = q;
#pragma unroll
            for (int j = SG_KNN - 1; j > 0; --j)
                if (bd[j] < bd[j - 1]) { const double t = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = t; const int u = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = u; }
        }
    }
    const double nx = normals[(size_t)i * 3], ny = normals[(size_t)i * 3 + 1], nz = normals[(size_t)i * 3 + 2];
    const double norm_p = sqrt((nx * nx + ny * ny) + nz * nz);
#pragma unroll
    for (int j = 0; j < SG_KNN; ++j) {
        int q = bi[j];
        if (q >= 0) {
            const double mx = normals[(size_t)q * 3], my = normals[(size_t)q * 3 + 1], mz = normals[(size_t)q * 3 + 2];
            const double norm_q = sqrt((mx * mx + my * my) + mz * mz);
            const double c = ((mx * nx + my * ny) + mz * nz) / (norm_q * norm_p + 1e-10);
            if (!(c > -0.5)) q = -1;
        }
        nbr[(size_t)i * SG_KNN + j] = q >= 0 ? q - s0 : -1;
        nbw[(size_t)i * SG_KNN + j] = (float)bd[j];
    }
}

__device__ __forceinline__ bool sg_has_arc(const int32_t* __restrict__ nbr, int from, int to) {
    bool h = false;
#pragma unroll
    for (int j = 0; j < SG_KNN; ++j) h |= nbr[(size_t)from * SG_KNN + j] == to;
    return h;
}

// The undirected CSR of one mesh per workgroup (dijkstra(directed=False): an arc in either direction connects both ways; both directions
// carry the same float32 weight, so an arc whose reverse exists is entered once per end). rowptr: S + 1 entries per mesh at
// s_ptr[b] + b; adj: capacity 10 S per mesh at 10 s_ptr[b]. The order of a row's entries is whatever the atomics give: a minimum does
// not depend on it. The counters are updated by device-scope atomics, so their plain reads and writes are device-scope too.
__global__ __launch_bounds__(SG_THREADS) void sg_graph_kernel(const int32_t* __restrict__ nbr_all, const float* __restrict__ nbw_all,
                                                              const int32_t* __restrict__ s_ptr, int32_t* __restrict__ rowptr_all,
                                                              int32_t* __restrict__ cursor_all, uint2* __restrict__ adj_all, int32_t* __restrict__ status) {
    __shared__ int s_sum[SG_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s0 = s_ptr[b], S = s_ptr[b + 1] - s0;
    const int32_t* nbr = nbr_all + (size_t)s0 * SG_KNN;
    const float* nbw = nbw_all + (size_t)s0 * SG_KNN;
    int32_t* rowptr = rowptr_all + s0 + b;
    int32_t* cur = cursor_all + s0;
    uint2* adj = adj_all + (size_t)s0 * 2 * SG_KNN;
    for (int v = tid; v < S; v += SG_THREADS) cur[v] = 0;
    __syncthreads();
    for (int i = tid; i < S * SG_KNN; i += SG_THREADS) {
        const int p = i / SG_KNN, q = nbr[i];
        if (q < 0) continue;
        atomicAdd(&cur[p], 1);
        if (!sg_has_arc(nbr, q, p)) atomicAdd(&cur[q], 1);
    }
    __syncthreads();
    // exclusive scan of the degrees: a contiguous chunk per thread, the chunk sums scanned in LDS
    const int chunk = (S + SG_THREADS - 1) / SG_THREADS;
    const int v0 = min(tid * chunk, S), v1 = min(v0 + chunk, S);
    int sum = 0;
    for (int v = v0; v < v1; ++v) sum += __hip_atomic_load(&cur[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_sum[tid] = sum;
    __syncthreads();
    for (int o = 1; o < SG_THREADS; o <<= 1) {
        const int t = tid >= o ? s_sum[tid - o] : 0;
        __syncthreads();
        s_sum[tid] += t;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int v = v0; v < v1; ++v) {
        const int d = __hip_atomic_load(&cur[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rowptr[v] = run;
        __hip_atomic_store(&cur[v], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run += d;
    }
    if (tid == SG_THREADS - 1) { rowptr[S] = s_sum[tid]; atomicAdd(status + 4, s_sum[tid]); }
    __syncthreads();
    for (int i = tid; i < S * SG_KNN; i += SG_THREADS) {
        const int p = i / SG_KNN, q = nbr[i];
        if (q < 0) continue;
        const uint32_t w = __float_as_uint(nbw[i]);
        adj[atomicAdd(&cur[p], 1)] = make_uint2((uint32_t)q, w);
        if (!sg_has_arc(nbr, q, p)) adj[atomicAdd(&cur[q], 1)] = make_uint2((uint32_t)p, w);
    }
}

// status[0]: error, status[1]: job counter, status[2]: the largest sweep count of a job, status[3]: the sum of all jobs' sweep counts,
// status[4]: the directed adjacency entries of all meshes (sg_graph_kernel)
template <int NSRC, bool LDS>
__global__ __launch_bounds__(SG_THREADS) void sg_apsp_kernel(const double* __restrict__ pts, const int32_t* __restrict__ s_ptr,
                                                             const int32_t* __restrict__ job_ptr, int n_meshes, int n_jobs,
                                                             const int32_t* __restrict__ rowptr_all, const uint2* __restrict__ adj_all,
                                                             const int64_t* __restrict__ out_off, double* __restrict__ gws, int max_s,
                                                             int32_t* __restrict__ status, double* __restrict__ out) {
    __shared__ double s_d[LDS ? SG_LDS_DOUBLES : 1];
    __shared__ int s_job;
    const int tid = threadIdx.x;
    double* d;
    if constexpr (LDS) d = s_d; else d = gws + (size_t)blockIdx.x * NSRC * max_s;
    for (;;) {
        __syncthreads();
        if (tid == 0) s_job = atomicAdd(status + 1, 1);
        __syncthreads();
        const int g = s_job;
        if (g >= n_jobs) return;
        const int b = segment_of(job_ptr, n_meshes, g);
        const int s0 = s_ptr[b], S = s_ptr[b + 1] - s0;
        if (S > max_s || (LDS && (long)S * NSRC > SG_LDS_DOUBLES)) {     // refused by the host layer; uniform
            if (tid == 0) atomicMax(status, SG_ERR_SIZE);
            continue;
        }
        const int src0 = (g - job_ptr[b]) * NSRC;
        const int32_t* rowptr = rowptr_all + s0 + b;
        const uint2* adj = adj_all + (size_t)s0 * 2 * SG_KNN;
        for (int v = tid; v < S; v += SG_THREADS)
#pragma unroll
            for (int s = 0; s < NSRC; ++s) d[v * NSRC + s] = v == src0 + s ? 0.0 : (double)INFINITY;
        __syncthreads();
        int sweeps = 0;
        bool failed = false;
        for (;;) {
            int changed = 0;
            for (int v = tid; v < S; v += SG_THREADS) {
                double best[NSRC], old[NSRC];
#pragma unroll
                for (int s = 0; s < NSRC; ++s) { old[s] = d[v * NSRC + s]; best[s] = old[s]; }
                const int e1 = rowptr[v + 1];
                for (int e = rowptr[v]; e < e1; ++e) {
                    const uint2 a = adj[e];
                    const double w = (double)__uint_as_float(a.y);
                    const double* du = d + (size_t)a.x * NSRC;
#pragma unroll
                    for (int s = 0; s < NSRC; ++s) { const double c = du[s] + w; best[s] = c < best[s] ? c : best[s]; }
                }
#pragma unroll
                for (int s = 0; s < NSRC; ++s)
                    if (best[s] < old[s]) { d[v * NSRC + s] = best[s]; changed = 1; }
            }
            ++sweeps;
            if (!__syncthreads_or(changed)) break;
            if (sweeps > S) { failed = true; break; }    // S sweeps settle every node of an S-node graph: never spin
        }
        if (tid == 0) { atomicMax(status + 2, sweeps); atomicAdd(status + 3, sweeps); }
        if (failed) {
            if (tid == 0) atomicMax(status, SG_ERR_SWEEPS);
            continue;
        }
        // rows src0 .. of the mesh's [S][S] matrix; an unreachable pair is 8.0 + its Euclidean distance (common_ops.py:200-203)
        double* o = out + out_off[b];
        const double* P = pts + (size_t)s0 * 3;
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
            const int src = src0 + s;
            if (src >= S) break;
            const double sx = P[(size_t)src * 3], sy = P[(size_t)src * 3 + 1], sz = P[(size_t)src * 3 + 2];
            for (int v = tid; v < S; v += SG_THREADS) {
                double x = d[v * NSRC + s];
                if (isinf(x)) x = 8.0 + dist3(P[(size_t)v * 3], P[(size_t)v * 3 + 1], P[(size_t)v * 3 + 2], sx, sy, sz);
                o[(size_t)src * S + v] = x;
            }
        }
    }
}

// common_ops.py:206-207 (squared = 0: argmin of the float64 distance) and joint2rig.py:356-357 (squared = 1: of the squared distance);
// np.argmin: the first minimum
__global__ void nearest_point_kernel(const double* __restrict__ q, const int32_t* __restrict__ q_ptr, const double* __restrict__ pts,
                                     const int32_t* __restrict__ p_ptr, int n_meshes, int n_q, int squared, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_q) return;
    const int b = segment_of(q_ptr, n_meshes, i);
    const int p0 = p_ptr[b], p1 = p_ptr[b + 1];
    const double x = q[(size_t)i * 3], y = q[(size_t)i * 3 + 1], z = q[(size_t)i * 3 + 2];
    double best = INFINITY;
    int bi = p1 > p0 ? 0 : -1;
    for (int p = p0; p < p1; ++p) {
        const double dx = x - pts[(size_t)p * 3], dy = y - pts[(size_t)p * 3 + 1], dz = z - pts[(size_t)p * 3 + 2];
        double d = (dx * dx + dy * dy) + dz * dz;
        if (!squared) d = sqrt(d);
        if (d < best) { best = d; bi = p - p0; }
    }
    out[i] = bi;
}

// ---- stage 2: pts2line (joint2rig.py:41-68), one thread per (vertex, bone). origins [pair][3], dist [pair]; pair = off[b] + v * nb + c
struct PairIdx { int b, v, c, nb, v0, c0; };
__device__ __forceinline__ PairIdx pair_of(const int64_t* __restrict__ off, const int32_t* __restrict__ vtx_ptr, const int32_t* __restrict__ bone_ptr,
                                           int n_meshes, int64_t i) {
    const int lo = segment_of(off, n_meshes, i);
    PairIdx r;
    r.b = lo; r.v0 = vtx_ptr[lo]; r.c0 = bone_ptr[lo]; r.nb = bone_ptr[lo + 1] - r.c0;
    const int64_t k = i - off[lo];
    r.v = (int)(k / r.nb); r.c = (int)(k % r.nb);
    return r;
}

__device__ __forceinline__ void pt2line(const double* __restrict__ p, const double* __restrict__ bn, double* o, double& dist) {
    const double ax = bn[0], ay = bn[1], az = bn[2];
    const double ex = bn[3] - ax, ey = bn[4] - ay, ez = bn[5] - az;
    const double l2 = (ex * ex + ey * ey) + ez * ez;
    o[0] = ax; o[1] = ay; o[2] = az;
    if (!(fabs(l2) < 1e-8)) {
        double t = (((p[0] - ax) * ex + (p[1] - ay) * ey) + (p[2] - az) * ez) / l2;
        t = fmin(fmax(t, 0.0), 1.0);
        o[0] = ax + t * ex; o[1] = ay + t * ey; o[2] = az + t * ez;
    }
    dist = dist3(o[0], o[1], o[2], p[0], p[1], p[2]);
}

__global__ void bone_point_kernel(const double* __restrict__ pos, const int32_t* __restrict__ vtx_ptr, const double* __restrict__ bones,
                                  const int32_t* __restrict__ bone_ptr, int n_meshes, const int64_t* __restrict__ off, int64_t n_pairs,
                                  double* __restrict__ origins, double* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const PairIdx k = pair_of(off, vtx_ptr, bone_ptr, n_meshes, i);
    double o[3], d;
    pt2line(pos + (size_t)(k.v0 + k.v) * 3, bones + (size_t)(k.c0 + k.c) * 6, o, d);
    origins[i * 3] = o[0]; origins[i * 3 + 1] = o[1]; origins[i * 3 + 2] = o[2];
    dist[i] = d;
}

// ---- stage 3: visibility (joint2rig.py:71-94). One thread per ray (vertex, bone): origin = the bone's nearest point, direction =
// (vertex - origin) + 1e-15; the triangles of the mesh's occluder pass through LDS in tiles (v0, e1, e2, |e1 x e2|: one broadcast read per
// thread). Moeller-Trumbore in float64: |det| <= 1e-12 |dir| |e1 x e2| is parallel; barycentric tolerance 1e-12; a hit needs t > 0.
// min_hit = the nearest hit's distance from the origin, or the ray's length; visible iff |min_hit - length| < 1e-4.
constexpr int VIS_THREADS = 256;
constexpr int VIS_TILE = 256;
__global__ __launch_bounds__(VIS_THREADS) void bone_visibility_kernel(
        const double* __restrict__ pos, const int32_t* __restrict__ vtx_ptr, const double* __restrict__ bones, const int32_t* __restrict__ bone_ptr,
        const double* __restrict__ tri_pos, const int32_t* __restrict__ tp_ptr, const int32_t* __restrict__ faces, const int32_t* __restrict__ f_ptr,
        const int64_t* __restrict__ off, const int32_t* __restrict__ blk_ptr, int n_meshes, uint8_t* __restrict__ vis) {
    __shared__ double s_tri[VIS_TILE][10];
    const BlockRow at = block_row(blk_ptr, n_meshes, (int)blockIdx.x, (int)threadIdx.x, VIS_THREADS);
    const int b = at.seg, v0 = vtx_ptr[b], nv = vtx_ptr[b + 1] - v0, c0 = bone_ptr[b], nb = bone_ptr[b + 1] - c0;
    const int64_t k = at.row;
    const bool live = k >= 0 && k < (int64_t)nv * nb;
    double o[3] = {0.0, 0.0, 0.0}, dx = 0.0, dy = 0.0, dz = 0.0, len = 0.0, dn = 0.0;
    if (live) {
        const double* p = pos + (size_t)(v0 + (int)(k / nb)) * 3;
        double dd;
        pt2line(p, bones + (size_t)(c0 + (int)(k % nb)) * 6, o, dd);
        const double rx = p[0] - o[0], ry = p[1] - o[1], rz = p[2] - o[2];
        len = sqrt((rx * rx + ry * ry) + rz * rz);
        dx = rx + 1e-15; dy = ry + 1e-15; dz = rz + 1e-15;
        dn = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    double min_hit = INFINITY;
    const int f0 = f_ptr[b], nf = f_ptr[b + 1] - f0, t0 = tp_ptr[b], nt = tp_ptr[b + 1] - t0;
    for (int base = 0; base < nf; base += VIS_TILE) {
        __syncthreads();
        for (int j = threadIdx.x; j < VIS_TILE; j += VIS_THREADS) {
            double* T = s_tri[j];
            if (base + j >= nf) continue;
            if (nt <= 0) {                               // no corner to read: a degenerate triangle, never hit
                for (int c = 0; c < 10; ++c) T[c] = 0.0;
            } else {
                const int32_t* f = faces + (size_t)(f0 + base + j) * 3;
                // an index out of range is refused by the host layer; clamped here so that no read leaves the buffer
                const int i0 = min(max(f[0], 0), nt - 1), i1 = min(max(f[1], 0), nt - 1), i2 = min(max(f[2], 0), nt - 1);
                const double* A = tri_pos + (size_t)(t0 + i0) * 3;
                const double* B = tri_pos + (size_t)(t0 + i1) * 3;
                const double* C = tri_pos + (size_t)(t0 + i2) * 3;
                T[0] = A[0]; T[1] = A[1]; T[2] = A[2];
                const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
                const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
                T[3] = e1x; T[4] = e1y; T[5] = e1z; T[6] = e2x; T[7] = e2y; T[8] = e2z;
                const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
                T[9] = sqrt((nx * nx + ny * ny) + nz * nz);
            }
        }
        __syncthreads();
        const int m = min(VIS_TILE, nf - base);
        if (live) {
            for (int j = 0; j < m; ++j) {
                const double* T = s_tri[j];
                const double e1x = T[3], e1y = T[4], e1z = T[5], e2x = T[6], e2y = T[7], e2z = T[8];
                const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
                const double det = (e1x * px + e1y * py) + e1z * pz;
                if (!(fabs(det) > 1e-12 * dn * T[9])) continue;
                const double inv = 1.0 / det;
                const double tx = o[0] - T[0], ty = o[1] - T[1], tz = o[2] - T[2];
                const double u = ((tx * px + ty * py) + tz * pz) * inv;
                if (u < -1e-12 || u > 1.0 + 1e-12) continue;
                const double qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
                const double v = ((dx * qx + dy * qy) + dz * qz) * inv;
                if (v < -1e-12 || u + v > 1.0 + 1e-12) continue;
                const double t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
                if (!(t > 0.0)) continue;
                const double hx = t * dx, hy = t * dy, hz = t * dz;
                const double h = sqrt((hx * hx + hy * hy) + hz * hz);
                min_hit = h < min_hit ? h : min_hit;
            }
        }
    }
    if (live) {
        if (isinf(min_hit)) min_hit = len;
        vis[off[b] + k] = fabs(min_hit - len) < 1e-4 ? 1 : 0;
    }
}

// ---- stage 2: calc_geodesic_matrix (joint2rig.py:333-354) ----
// One workgroup per (mesh, bone): np.percentile(dist[visible], 15) with numpy's default linear interpolation (virtual index (n - 1) q,
// _lerp), from the two order statistics found by rank counting; then visibility is cleared where dist > 1.3 x percentile. vis_t is the
// result, bone-major: [bone_ptr-wise columns][V]; n_vis[bone] the number of visible vertices left.
// The column (dist where visible, NaN elsewhere: a NaN never counts) is staged in LDS when the mesh has at most PCT_CAP vertices, so that
// the rank counting reads LDS by broadcast; a larger mesh reads it from global memory.
constexpr int PCT_THREADS = 1024;
constexpr int PCT_CAP = 8192;
__global__ __launch_bounds__(PCT_THREADS) void bone_percentile_kernel(const double* __restrict__ dist, const uint8_t* __restrict__ vis,
                                                                      const int32_t* __restrict__ vtx_ptr, const int32_t* __restrict__ bone_ptr,
                                                                      const int64_t* __restrict__ off, int n_meshes, uint8_t* __restrict__ vis_after,
                                                                      int32_t* __restrict__ n_vis, double* __restrict__ pct) {
    __shared__ int s_n, s_n2;
    __shared__ double s_ab[2];
    __shared__ double s_x[PCT_CAP];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int b = segment_of(bone_ptr, n_meshes, g);
    const int nb = bone_ptr[b + 1] - bone_ptr[b], c = g - bone_ptr[b], nv = vtx_ptr[b + 1] - vtx_ptr[b];
    const double* D = dist + off[b] + c;
    const uint8_t* Vs = vis + off[b] + c;
    uint8_t* Va = vis_after + off[b] + c;
    if (tid == 0) { s_n = 0; s_n2 = 0; }
    __syncthreads();
    const bool staged = nv <= PCT_CAP;
    int cnt = 0;
    for (int v = tid; v < nv; v += PCT_THREADS) {
        const bool on = Vs[(size_t)v * nb] != 0;
        cnt += on ? 1 : 0;
        if (staged) s_x[v] = on ? D[(size_t)v * nb] : (double)NAN;
    }
    if (cnt) atomicAdd(&s_n, cnt);
    __syncthreads();
    const int n = s_n;
    if (n == 0) {
        for (int v = tid; v < nv; v += PCT_THREADS) Va[(size_t)v * nb] = 0;
        if (tid == 0) { n_vis[g] = 0; pct[g] = NAN; }
        return;
    }
    const double vi = (double)(n - 1) * (15.0 / 100.0);
    const double fl = floor(vi);
    const int lo = (int)fl, hi = min(lo + 1, n - 1);
    const double t = vi - fl;
    for (int v = tid; v < nv; v += PCT_THREADS) {
        if (!Vs[(size_t)v * nb]) continue;
        const double x = D[(size_t)v * nb];
        int rank = 0;
        if (staged) {
            for (int u = 0; u < nv; ++u) { const double y = s_x[u]; rank += (y < x || (y == x && u < v)) ? 1 : 0; }
        } else {
            for (int u = 0; u < nv; ++u) {
                if (!Vs[(size_t)u * nb]) continue;
                const double y = D[(size_t)u * nb];
                rank += (y < x || (y == x && u < v)) ? 1 : 0;
            }
        }
        if (rank == lo) s_ab[0] = x;
        if (rank == hi) s_ab[1] = x;
    }
    __syncthreads();
    const double a = s_ab[0], bb = s_ab[1];
    const double diff = bb - a;
    const double p = t >= 0.5 ? bb - diff * (1.0 - t) : a + diff * t;      // numpy's _lerp
    const double thr = 1.3 * p;
    cnt = 0;
    for (int v = tid; v < nv; v += PCT_THREADS) {
        const uint8_t keep = (Vs[(size_t)v * nb] && !(D[(size_t)v * nb] > thr)) ? 1 : 0;
        Va[(size_t)v * nb] = keep;
        cnt += keep;
    }
    if (cnt) atomicAdd(&s_n2, cnt);
    __syncthreads();
    if (tid == 0) { n_vis[g] = s_n2; pct[g] = p; }
}

// One thread per (vertex r, bone c), lanes along c: a visible pair takes dist; a bone without visible vertices takes dist for the whole
// column; otherwise the minimum of surface_geodesic[r, visible] (first arg-min in vertex order) + dist at that vertex, or 8 + dist where
// the minimum is infinite. sg: the mesh's [V][V] float64 matrix at sg_off[b]. nn: the arg-min vertex (-1 where none was searched).
__global__ void bone_geodesic_kernel(const double* __restrict__ dist, const uint8_t* __restrict__ vis_after, const int32_t* __restrict__ n_vis,
                                     const double* __restrict__ sg, const int64_t* __restrict__ sg_off, const int32_t* __restrict__ vtx_ptr,
                                     const int32_t* __restrict__ bone_ptr, const int64_t* __restrict__ off, int n_meshes, int64_t n_pairs,
                                     double* __restrict__ out, int32_t* __restrict__ nn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    const PairIdx k = pair_of(off, vtx_ptr, bone_ptr, n_meshes, i);
    const int nv = vtx_ptr[k.b + 1] - k.v0;
    const double dv = dist[i];
    double r = dv;
    int arg = -1;
    if (!vis_after[i] && n_vis[k.c0 + k.c] > 0) {
        const double* row = sg + sg_off[k.b] + (size_t)k.v * nv;
        const uint8_t* col = vis_after + off[k.b] + k.c;
        double best = INFINITY;
        for (int u = 0; u < nv; ++u) {
            if (!col[(size_t)u * k.nb]) continue;
            const double x = row[u];
            if (arg < 0 || x < best) { best = x; arg = u; }
        }
        r = isinf(best) ? 8.0 + dv : best + dist[off[k.b] + (int64_t)arg * k.nb + k.c];
    }
    out[i] = r;
    nn[i] = arg;
}

// predict_skinning's loop (joint2rig.py:413-442): the k nearest bones of every vertex by the float64 distance, equal distances by
// ascending bone id; per slot the bone (6), 1 / (D + 1e-10), the leaf flag, as float32; a slot past the bone count repeats the nearest
// bone with skin_nn = 0 and loss_mask = 0.
__global__ void skin_bind_geo_kernel(const double* __restrict__ dist, const int64_t* __restrict__ off, const int32_t* __restrict__ vtx_ptr,
                                     const int32_t* __restrict__ bone_ptr, int n_meshes, int n, const double* __restrict__ bones,
                                     const uint8_t* __restrict__ is_leaf, int k, float* __restrict__ skin_input, int64_t* __restrict__ skin_nn,
                                     int64_t* __restrict__ loss_mask) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int b = segment_of(vtx_ptr, n_meshes, v);
    const int c0 = bone_ptr[b], nb = bone_ptr[b + 1] - c0;
    if (nb <= 0) return;                                 // refused by the host layer
    const double* row = dist + off[b] + (size_t)(v - vtx_ptr[b]) * nb;
    double pd = 0.0, fd = 0.0;
    int pj = -1, first = 0;
    for (int s = 0; s < k; ++s) {
        int id = -1;
        double dsel = 0.0;
        if (s < nb) {
            for (int j = 0; j < nb; ++j) {
                const double x = row[j];
                const bool after = pj < 0 || x > pd || (x == pd && j > pj);
                if (after && (id < 0 || x < dsel)) { id = j; dsel = x; }
            }
            if (id < 0) { id = 0; dsel = row[0]; }       // NaN distances: keep the indices in range
            pd = dsel; pj = id;
        }
        if (s == 0) { first = id; fd = dsel; }
        const bool valid = s < nb;
        const int t = valid ? id : first;
        const double D = valid ? dsel : fd;
        const size_t o = (size_t)v * k + s;
        const double* bo = bones + (size_t)(c0 + t) * 6;
        float* si = skin_input + o * 8;
        for (int c = 0; c < 6; ++c) si[c] = (float)bo[c];
        si[6] = (float)(1.0 / (D + 1e-10));
        si[7] = is_leaf[c0 + t] ? 1.0f : 0.0f;
        skin_nn[o] = valid ? t : 0;
        loss_mask[o] = valid ? 1 : 0;
    }
}

}  // namespace morig

using namespace morig;

static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

extern "C" int64_t morig_surface_geodesic_workspace(int64_t total_samples, int32_t n_meshes, int32_t max_samples, int32_t n_slots, int32_t use_lds) {
    if (total_samples < 0 || n_meshes < 0 || max_samples < 0 || n_slots < 0) return MORIG_E_INVALID;
    // nbr int32 [5 S], nbw float [5 S], rowptr int32 [S + B], cursor int32 [S], adj uint2 [10 S], vectors double [slots][4][max S]
    return align256(total_samples * SG_KNN * 4) * 2 + align256((total_samples + n_meshes) * 4) + align256(total_samples * 4) +
           align256(total_samples * 2 * SG_KNN * 8) + (use_lds ? 0 : align256((int64_t)n_slots * 4 * max_samples * 8));
}

extern "C" int morig_surface_geodesic(const double* pts, const double* normals, const int32_t* s_ptr, const int32_t* job_ptr, int32_t n_meshes,
                                      int64_t total_samples, int32_t max_samples, int32_t n_jobs, int32_t nsrc, int32_t use_lds,
                                      const int64_t* out_off, int32_t n_slots, void* workspace, int64_t workspace_bytes, int32_t* status,
                                      double* out, void* stream) {
    if (!pts || !normals || !s_ptr || !job_ptr || !out_off || !status || !out || !workspace || n_meshes <= 0 || total_samples <= 0 ||
        total_samples > 0x7fffffff / (2 * SG_KNN) || max_samples < SG_KNN + 1 || max_samples > SG_MAX_SAMPLES || n_jobs <= 0 || n_slots <= 0)
        return MORIG_E_INVALID;
    if (use_lds ? !((nsrc == 1 || nsrc == 2 || nsrc == 4) && (int64_t)nsrc * max_samples <= SG_LDS_DOUBLES) : nsrc != 4) return MORIG_E_INVALID;
    if (workspace_bytes < morig_surface_geodesic_workspace(total_samples, n_meshes, max_samples, n_slots, use_lds)) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, 8 * sizeof(int32_t), s));
    char* w = reinterpret_cast<char*>(workspace);
    int32_t* nbr = reinterpret_cast<int32_t*>(w); w += align256(total_samples * SG_KNN * 4);
    float* nbw = reinterpret_cast<float*>(w); w += align256(total_samples * SG_KNN * 4);
    int32_t* rowptr = reinterpret_cast<int32_t*>(w); w += align256((total_samples + n_meshes) * 4);
    int32_t* cursor = reinterpret_cast<int32_t*>(w); w += align256(total_samples * 4);
    uint2* adj = reinterpret_cast<uint2*>(w); w += align256(total_samples * 2 * SG_KNN * 8);
    double* gws = reinterpret_cast<double*>(w);
    const int n = (int)total_samples;
    hipLaunchKernelGGL(sg_knn_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, pts, normals, s_ptr, n_meshes, n, nbr, nbw);
    MORIG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sg_graph_kernel, dim3(n_meshes), dim3(SG_THREADS), 0, s, nbr, nbw, s_ptr, rowptr, cursor, adj, status);
    MORIG_LAUNCH_CHECK();
    const dim3 grid(n_slots < n_jobs ? n_slots : n_jobs), block(SG_THREADS);
#define SG_LAUNCH(N, L) hipLaunchKernelGGL((sg_apsp_kernel<N, L>), grid, block, 0, s, pts, s_ptr, job_ptr, n_meshes, n_jobs, rowptr, adj, out_off, \
                                           gws, max_samples, status, out)
    if (!use_lds) SG_LAUNCH(4, false);
    else if (nsrc == 4) SG_LAUNCH(4, true);
    else if (nsrc == 2) SG_LAUNCH(2, true);
    else SG_LAUNCH(1, true);
#undef SG_LAUNCH
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_nearest_point(const double* q, const int32_t* q_ptr, const double* pts, const int32_t* p_ptr, int32_t n_meshes, int32_t n_q,
                                   int32_t squared, int32_t* out, void* stream) {
    if (!q_ptr || !p_ptr || n_meshes <= 0 || n_q < 0) return MORIG_E_INVALID;
    if (n_q == 0) return MORIG_OK;
    if (!q || !pts || !out) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(nearest_point_kernel, dim3(cdiv(n_q, 128)), dim3(128), 0, s, q, q_ptr, pts, p_ptr, n_meshes, n_q, squared, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_bone_point_distance(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, int32_t n_meshes,
                                         const int64_t* off, int64_t n_pairs, double* origins, double* dist, void* stream) {
    if (!vtx_ptr || !bone_ptr || !off || n_meshes <= 0 || n_pairs < 0) return MORIG_E_INVALID;
    if (n_pairs == 0) return MORIG_OK;
    if (!pos || !bones || !origins || !dist) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(bone_point_kernel, dim3(cdiv(n_pairs, 256)), dim3(256), 0, s, pos, vtx_ptr, bones, bone_ptr, n_meshes, off, n_pairs, origins, dist);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_bone_visibility(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, const double* tri_pos,
                                     const int32_t* tp_ptr, const int32_t* faces, const int32_t* f_ptr, const int64_t* off, const int32_t* blk_ptr,
                                     int32_t n_meshes, int32_t n_blocks, uint8_t* vis, void* stream) {
    if (!vtx_ptr || !bone_ptr || !tp_ptr || !f_ptr || !off || !blk_ptr || n_meshes <= 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!pos || !bones || !vis) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(bone_visibility_kernel, dim3(n_blocks), dim3(VIS_THREADS), 0, s, pos, vtx_ptr, bones, bone_ptr, tri_pos, tp_ptr, faces, f_ptr,
                       off, blk_ptr, n_meshes, vis);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_bone_geodesic(const double* dist, const uint8_t* vis, const double* sg, const int64_t* sg_off, const int32_t* vtx_ptr,
                                   const int32_t* bone_ptr, const int64_t* off, int32_t n_meshes, int32_t n_bones, int64_t n_pairs,
                                   uint8_t* vis_after, int32_t* n_vis, double* pct, double* out, int32_t* nn, void* stream) {
    if (!vtx_ptr || !bone_ptr || !off || !sg_off || n_meshes <= 0 || n_bones < 0 || n_pairs < 0) return MORIG_E_INVALID;
    if (n_pairs == 0 || n_bones == 0) return MORIG_OK;
    if (!dist || !vis || !sg || !vis_after || !n_vis || !pct || !out || !nn) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(bone_percentile_kernel, dim3(n_bones), dim3(PCT_THREADS), 0, s, dist, vis, vtx_ptr, bone_ptr, off, n_meshes, vis_after, n_vis, pct);
    MORIG_LAUNCH_CHECK();
    hipLaunchKernelGGL(bone_geodesic_kernel, dim3(cdiv(n_pairs, 256)), dim3(256), 0, s, dist, vis_after, n_vis, sg, sg_off, vtx_ptr, bone_ptr, off,
                       n_meshes, n_pairs, out, nn);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skin_bind_geo(const double* dist, const int64_t* off, const int32_t* vtx_ptr, const int32_t* bone_ptr, int32_t n_meshes,
                                   int32_t n_vertices, const double* bones, const uint8_t* is_leaf, int32_t k, float* skin_input, int64_t* skin_nn,
                                   int64_t* loss_mask, void* stream) {
    if (!dist || !off || !vtx_ptr || !bone_ptr || !bones || !is_leaf || !skin_input || !skin_nn || !loss_mask || n_meshes <= 0 || n_vertices < 0 ||
        k < 1) return MORIG_E_INVALID;
    if (n_vertices == 0) return MORIG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(skin_bind_geo_kernel, dim3(cdiv(n_vertices, 128)), dim3(128), 0, s, dist, off, vtx_ptr, bone_ptr, n_meshes, n_vertices, bones,
                       is_leaf, k, skin_input, skin_nn, loss_mask);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
