// Mesh diagnosis and cleaning (morig_amd/meshprep.py diagnose / clean): weld classes, degenerate and duplicate
// faces, the edges of the kept faces with their classes, connected components with their table, and the compaction of the cleaned mesh,
// for a ragged batch of meshes. The module's idiom: a kernel emits 64-bit keys, the caller sorts them (torch.sort), a kernel marks the
// runs. Everything is an integer or float64 in the written order (contraction off); the only atomics are integer ones (OR, add, min),
// whose result does not depend on order: two runs give the same bits, a mesh alone gives the bits it gives inside a batch. Nothing
// depends on one workgroup seeing another's store inside a launch: the launch boundary is the only synchronisation.
//
// coord keys    one thread per vertex row: an order-preserving key per coordinate (topo_core.h), and whether the row is finite.
// weld mark     one thread per position of the rows sorted (stably) by z, y, x: the first row of every run of equal rows of ONE mesh. Rows
//               of equal keys stay in ascending row order, so the rows of a mesh are contiguous inside a run of equal coordinates and no
//               sort by mesh is needed; a row with a non-finite coordinate is a run of its own.
// run rep       two launches: the first item of run k goes to start[k], then every item reads the start of its run: the representative
//               (stability makes it the lowest index). The same pair gives every face its surviving duplicate.
// face keys     one thread per face: the representatives of its corners; major = the lowest of them (INT64_MAX where two coincide),
//               minor = mid << 32 | high: two stable sorts order the faces by their vertex set with no limit below the int32 row tables.
// face edges    one thread per face: a kept face marks its classes referenced (atomicOr), tells whether its normal is exactly zero and
//               emits its three directed edge keys lo << 32 | hi << 1 | dir.
// cc round      one round of the component rule: next = cur, then with gp = cur[cur] every vertex and both ends of every edge key lower
//               next[v] and next[cur[v]] by atomicMin. The round reads cur only, so the state after it is a function of the input.
// classify      one thread per sorted edge key; the thread at the first key of a run walks the run (of any length, anywhere) and
//               writes its class; a boundary edge is added to the count of its component's root (atomicAdd on int32).
// comp counts   referenced classes and kept faces per root (atomicAdd on int32), and the root of every face for the component sort.
// comp area     one wave per component over its faces in ascending input order: lane l adds the faces l, l + 64, ..., lane 0 folds the
//               64 sums 32, 16, 8, 4, 2, 1 (topo_core.h fold_lanes). No floating-point atomic.
// keep, compact which classes and faces leave, then the output vertices, faces and the two maps at their prefix-sum ranks.
#include "common.h"

#pragma clang fp contract(off)                 // in front of topo_core.h: its functions are compiled under it too

#include "topo_core.h"

namespace morig {

namespace {

using namespace morig_topo;

constexpr long long ROOT_NONE = 0x7fffffffLL;

__global__ void __launch_bounds__(256) mc_coord_keys_kernel(const double* __restrict__ verts, int n_rows, long long* __restrict__ keys,
                                                            int* __restrict__ nonfinite) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = verts[(size_t)v * 3 + c];
        keys[(size_t)c * n_rows + v] = coord_key(x);
        fin = fin && finite(x);
    }
    nonfinite[v] = fin ? 0 : 1;
}

__global__ void __launch_bounds__(256) mc_weld_mark_kernel(const long long* __restrict__ keys, const int* __restrict__ nonfinite,
                                                           const long long* __restrict__ order, int n_rows, const int* __restrict__ vptr,
                                                           int n_meshes, int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const long long r = order[i], p = i > 0 ? order[i - 1] : -1;
    bool first = i == 0 || r < 0 || r >= n_rows || p < 0 || p >= n_rows;
    if (!first) {
        first = nonfinite[r] || nonfinite[p] || segment_of(vptr, n_meshes, r) != segment_of(vptr, n_meshes, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) first = first || keys[(size_t)c * n_rows + r] != keys[(size_t)c * n_rows + p];
    }
    flags[i] = first ? 1 : 0;
}

// rank: the inclusive prefix sum of flags
__global__ void __launch_bounds__(256) mc_run_start_kernel(const long long* __restrict__ order, const int* __restrict__ flags,
                                                           const long long* __restrict__ rank, int n, int* __restrict__ start) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const long long at = rank[i] - 1, item = order[i];
    if (at >= 0 && at < n && item >= 0 && item < n) start[at] = (int)item;
}

__global__ void __launch_bounds__(256) mc_run_rep_kernel(const long long* __restrict__ order, const long long* __restrict__ rank,
                                                         const int* __restrict__ dead, int n, const int* __restrict__ start,
                                                         int* __restrict__ rep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long item = order[i], at = rank[i] - 1;
    if (item < 0 || item >= n) return;
    if (dead && dead[item]) { rep[item] = -1; return; }
    rep[item] = (at >= 0 && at < n) ? start[at] : (int)item;
}

__global__ void __launch_bounds__(256) mc_face_keys_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                           const int* __restrict__ vptr, int n_meshes, const int* __restrict__ rep, int n_rows,
                                                           int* __restrict__ tri, long long* __restrict__ major, long long* __restrict__ minor,
                                                           int* __restrict__ degenerate, int* __restrict__ status) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    int v0 = vptr[b], nv = vptr[b + 1] - v0;
    if (v0 < 0 || nv < 0 || (long long)v0 + nv > n_rows) nv = 0;
    long long r[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int id = faces[(size_t)f * 3 + c];
        r[c] = -1;
        if (id < 0 || id >= nv) { ok = false; continue; }
        r[c] = rep[v0 + id];
        if (r[c] < 0 || r[c] >= n_rows) ok = false;
    }
    if (!ok) atomicOr(status, MORIG_MESHCHECK_BAD_FACE);                               // never followed: counted with the degenerate faces
#pragma unroll
    for (int c = 0; c < 3; ++c) tri[(size_t)f * 3 + c] = ok ? (int)r[c] : -1;
    const bool deg = !ok || r[0] == r[1] || r[1] == r[2] || r[0] == r[2];
    const long long lo = min(r[0], min(r[1], r[2])), hi = max(r[0], max(r[1], r[2]));
    const long long mid = r[0] + r[1] + r[2] - lo - hi;
    degenerate[f] = deg ? 1 : 0;
    major[f] = deg ? KEY_SENTINEL : lo;
    minor[f] = deg ? KEY_SENTINEL : ((mid << 32) | hi);
}

__global__ void __launch_bounds__(256) mc_face_mark_kernel(const long long* __restrict__ major, const long long* __restrict__ minor,
                                                           const long long* __restrict__ order, int n_faces, int* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_faces) return;
    const long long f = order[i], p = i > 0 ? order[i - 1] : -1;
    int flag = 0;
    if (f >= 0 && f < n_faces && major[f] != KEY_SENTINEL)
        flag = (i == 0 || p < 0 || p >= n_faces || major[p] != major[f] || minor[p] != minor[f]) ? 1 : 0;
    flags[i] = flag;
}

// tri: the representatives of every face's corners (-1: never followed); surv: the surviving face of every face (-1: degenerate)
__global__ void __launch_bounds__(256) mc_face_edges_kernel(const double* __restrict__ verts, const int* __restrict__ tri,
                                                            const int* __restrict__ surv, int n_faces, int n_rows, int* __restrict__ referenced,
                                                            int* __restrict__ zero_area, long long* __restrict__ ekeys) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    long long r[3];
    bool kept = surv[f] == f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[c] = tri[(size_t)f * 3 + c];
        kept = kept && r[c] >= 0 && r[c] < n_rows;
    }
    kept = kept && r[0] != r[1] && r[1] != r[2] && r[0] != r[2];
    bool zero = false;
    if (kept) {
        tri_area(verts + (size_t)r[0] * 3, verts + (size_t)r[1] * 3, verts + (size_t)r[2] * 3, &zero);
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicOr(referenced + r[c], 1);
    }
    zero_area[f] = zero ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) ekeys[(size_t)f * 3 + c] = kept ? edge_key(r[c], r[(c + 1) % 3]) : KEY_SENTINEL;
}

__device__ __forceinline__ void cc_lower(const int* __restrict__ cur, int* __restrict__ next, int t, int g, int& changed) {
    if (g < cur[t]) { atomicMin(next + t, g); changed = 1; }
}

// next holds a copy of cur when this starts (made by the launch in front of it)
__global__ void __launch_bounds__(256) mc_cc_round_kernel(const int* __restrict__ cur, int* __restrict__ next, int n_rows,
                                                          const long long* __restrict__ ekeys, long long n_keys, const int* __restrict__ vptr,
                                                          int n_meshes, int* __restrict__ changed) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int ch = 0;
    long long at = t;                                                                   // a row of the mesh this thread works for
    if (t < n_rows) {
        const int p = cur[t];
        if (p >= 0 && p < n_rows) cc_lower(cur, next, (int)t, cur[p], ch);                // next[cur[v]] cannot fall by gp[v] = cur[cur[v]]
    } else if (t - n_rows < n_keys) {
        const long long k = ekeys[t - n_rows];
        const long long u = edge_lo(k), w = edge_hi(k);
        at = u;
        if (k != KEY_SENTINEL && k >= 0 && u < n_rows && w < n_rows) {
            const int pu = cur[u], pw = cur[w];
            if (pu >= 0 && pu < n_rows && pw >= 0 && pw < n_rows) {
                const int gu = cur[pu], gw = cur[pw];
                cc_lower(cur, next, (int)u, gw, ch);
                cc_lower(cur, next, pu, gw, ch);
                cc_lower(cur, next, (int)w, gu, ch);
                cc_lower(cur, next, pw, gu, ch);
            }
        }
    }
    // every writer stores the same 1: a relaxed atomic STORE, not a read-modify-write (a million atomicOr on one word serialise)
    if (ch) __hip_atomic_store(changed + segment_of(vptr, n_meshes, at), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) mc_edge_classify_kernel(const long long* __restrict__ keys, long long n_keys, const int* __restrict__ label,
                                                               int n_rows, int* __restrict__ eclass, int* __restrict__ root_boundary) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_keys) return;
    long long count;
    const int cls = classify_run(keys, i, n_keys, &count);
    eclass[i] = cls;
    if (cls == EDGE_BOUNDARY) {
        const long long lo = edge_lo(keys[i]);
        if (lo >= 0 && lo < n_rows) {
            const int root = label[lo];
            if (root >= 0 && root < n_rows) atomicAdd(root_boundary + root, 1);
        }
    }
}

__global__ void __launch_bounds__(256) mc_comp_counts_kernel(const int* __restrict__ tri, const int* __restrict__ surv, int n_faces,
                                                             const int* __restrict__ referenced, const int* __restrict__ label, int n_rows,
                                                             int* __restrict__ root_verts, int* __restrict__ root_faces,
                                                             long long* __restrict__ face_root) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n_rows) {
        const int root = label[t];
        if (referenced[t] && root >= 0 && root < n_rows) atomicAdd(root_verts + root, 1);
    } else if (t - n_rows < n_faces) {
        const int f = (int)(t - n_rows), a = tri[(size_t)f * 3];
        long long root = ROOT_NONE;
        if (surv[f] == f && a >= 0 && a < n_rows) {
            const int l = label[a];
            if (l >= 0 && l < n_rows) { root = l; atomicAdd(root_faces + l, 1); }
        }
        face_root[f] = root;
    }
}

// order: the faces sorted stably by root; kptr [n_comps + 1]: the run of every component
__global__ void __launch_bounds__(256) mc_comp_area_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ tri, int n_faces,
                                                           const long long* __restrict__ order, const long long* __restrict__ kptr, int n_comps,
                                                           double* __restrict__ area) {
    __shared__ double sums[4][64];
    const int wave = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    const bool live = c < n_comps;
    long long k0 = live ? kptr[c] : 0, k1 = live ? kptr[c + 1] : 0;
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > n_faces ? n_faces : k1;
    double s = 0.0;
    for (long long k = k0 + lane; k < k1; k += 64) {
        const long long f = order[k];
        if (f < 0 || f >= n_faces) continue;
        const int a = tri[(size_t)f * 3], b = tri[(size_t)f * 3 + 1], d = tri[(size_t)f * 3 + 2];
        if (a < 0 || b < 0 || d < 0 || a >= n_rows || b >= n_rows || d >= n_rows) continue;
        bool zero;
        s = s + tri_area(verts + (size_t)a * 3, verts + (size_t)b * 3, verts + (size_t)d * 3, &zero);
    }
    sums[wave][lane] = s;
    __syncthreads();
    if (lane == 0 && live) area[c] = fold_lanes(sums[wave]);
}

// keep_root [n_rows]: whether the component with that root stays
__global__ void __launch_bounds__(256) mc_keep_flags_kernel(const int* __restrict__ rep, const int* __restrict__ referenced,
                                                            const int* __restrict__ label, const int* __restrict__ keep_root,
                                                            int drop_unreferenced, int n_rows, const int* __restrict__ tri,
                                                            const int* __restrict__ surv, int n_faces, int* __restrict__ vkeep,
                                                            int* __restrict__ fkeep) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n_rows) {
        int keep = rep[t] == t ? 1 : 0;
        if (keep && drop_unreferenced) {
            const int root = label[t];
            keep = referenced[t] && root >= 0 && root < n_rows && keep_root[root];
        }
        vkeep[t] = keep;
    } else if (t - n_rows < n_faces) {
        const int f = (int)(t - n_rows), a = tri[(size_t)f * 3];
        int keep = 0;
        if (surv[f] == f && a >= 0 && a < n_rows) {
            const int root = label[a];
            keep = root >= 0 && root < n_rows && keep_root[root];
        }
        fkeep[f] = keep;
    }
}

// vrank / frank: the inclusive prefix sums of vkeep / fkeep; ovptr / ofptr [n_meshes + 1]: the output rows in front of every mesh
__global__ void __launch_bounds__(256) mc_compact_kernel(const double* __restrict__ verts, const int* __restrict__ rep, const int* __restrict__ vkeep,
                                                         const long long* __restrict__ vrank, const int* __restrict__ vptr,
                                                         const long long* __restrict__ ovptr, int n_rows, int n_meshes,
                                                         const int* __restrict__ tri, const int* __restrict__ surv, const int* __restrict__ fkeep,
                                                         const long long* __restrict__ frank, const int* __restrict__ fptr,
                                                         const long long* __restrict__ ofptr, int n_faces, long long n_out_v, long long n_out_f,
                                                         double* __restrict__ out_verts, long long* __restrict__ out_faces,
                                                         long long* __restrict__ vertex_map, long long* __restrict__ face_map) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n_rows) {
        const int r = rep[t];
        long long to = -1;
        if (r >= 0 && r < n_rows && vkeep[r]) to = vrank[r] - 1;
        if (to >= n_out_v) to = -1;
        vertex_map[t] = to < 0 ? -1 : to - ovptr[segment_of(vptr, n_meshes, t)];
        if (to >= 0 && r == t)
#pragma unroll
            for (int c = 0; c < 3; ++c) out_verts[(size_t)to * 3 + c] = verts[(size_t)t * 3 + c];
    } else if (t - n_rows < n_faces) {
        const int f = (int)(t - n_rows), s = surv[f];
        long long to = -1;
        if (s >= 0 && s < n_faces && fkeep[s]) to = frank[s] - 1;
        if (to >= n_out_f) to = -1;
        const int b = segment_of(fptr, n_meshes, f);
        face_map[f] = to < 0 ? -1 : to - ofptr[b];
        if (to >= 0 && s == f)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r = tri[(size_t)f * 3 + c];
                long long at = -1;
                if (r >= 0 && r < n_rows && vkeep[r]) at = vrank[r] - 1 - ovptr[b];
                out_faces[(size_t)to * 3 + c] = at;
            }
    }
}

inline bool rows_ok(long long n) { return n >= 0 && n <= 0x7fffffffLL - 256; }

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_meshcheck_coord_keys(const double* verts, int32_t n_rows, int64_t* keys, int32_t* nonfinite, void* stream) {
    if (!rows_ok(n_rows)) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!verts || !keys || !nonfinite) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_WELD, s, 0.0, 52.0 * (double)n_rows);
    mc_coord_keys_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, n_rows, (long long*)keys, nonfinite);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_weld_mark(const int64_t* keys, const int32_t* nonfinite, const int64_t* order, int32_t n_rows, const int32_t* vptr,
                              int32_t n_meshes, int32_t* flags, void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0) return MORIG_OK;
    if (!keys || !nonfinite || !order || !vptr || !flags) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_WELD, s, 0.0, 72.0 * (double)n_rows);
    mc_weld_mark_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>((const long long*)keys, nonfinite, (const long long*)order, n_rows, vptr, n_meshes, flags);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_run_rep(const int64_t* order, const int32_t* flags, const int64_t* rank, const int32_t* dead, int32_t n, int32_t* start,
                            int32_t* rep, void* stream) {
    if (!rows_ok(n)) return MORIG_E_INVALID;
    if (n == 0) return MORIG_OK;
    if (!order || !flags || !rank || !start || !rep) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_WELD, s, 0.0, 48.0 * (double)n);
    mc_run_start_kernel<<<cdiv(n, 256), 256, 0, s>>>((const long long*)order, flags, (const long long*)rank, n, start);
    MORIG_LAUNCH_CHECK();
    mc_run_rep_kernel<<<cdiv(n, 256), 256, 0, s>>>((const long long*)order, (const long long*)rank, dead, n, start, rep);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_face_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* rep,
                              int32_t n_rows, int32_t* tri, int64_t* major, int64_t* minor, int32_t* degenerate, int32_t* status, void* stream) {
    if (!rows_ok(n_faces) || !rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_faces == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !rep || !tri || !major || !minor || !degenerate || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_FACES, s, 0.0, 56.0 * (double)n_faces);
    mc_face_keys_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, rep, n_rows, tri, (long long*)major, (long long*)minor,
                                                           degenerate, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_face_mark(const int64_t* major, const int64_t* minor, const int64_t* order, int32_t n_faces, int32_t* flags, void* stream) {
    if (!rows_ok(n_faces)) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!major || !minor || !order || !flags) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_FACES, s, 0.0, 44.0 * (double)n_faces);
    mc_face_mark_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>((const long long*)major, (const long long*)minor, (const long long*)order, n_faces, flags);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_face_edges(const double* verts, int32_t n_rows, const int32_t* tri, const int32_t* surv, int32_t n_faces, int32_t* referenced,
                               int32_t* zero_area, int64_t* ekeys, void* stream) {
    if (!rows_ok(n_rows) || n_faces < 0 || n_faces > (0x7fffffff - 256) / 3) return MORIG_E_INVALID;
    if (n_rows == 0 && n_faces == 0) return MORIG_OK;
    if ((n_rows > 0 && (!verts || !referenced)) || (n_faces > 0 && (!tri || !surv || !zero_area || !ekeys))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_rows > 0) MORIG_HIP_TRY(hipMemsetAsync(referenced, 0, (size_t)n_rows * sizeof(int32_t), s));
    if (n_faces == 0) return MORIG_OK;
    ProfScope ps(K_MESHCHECK_FACES, s, 0.0, 128.0 * (double)n_faces);
    mc_face_edges_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(verts, tri, surv, n_faces, n_rows, referenced, zero_area, (long long*)ekeys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_cc_round(const int32_t* cur, int32_t* next, int32_t n_rows, const int64_t* ekeys, int64_t n_keys, const int32_t* vptr,
                             int32_t n_meshes, int32_t* changed, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_keys) || !rows_ok((long long)n_rows + n_keys) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!changed || !vptr || (n_rows > 0 && (!cur || !next || cur == next)) || (n_keys > 0 && (!ekeys || n_rows == 0))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_COMPONENTS, s, 0.0, 8.0 * (double)n_rows + 40.0 * (double)n_keys);
    MORIG_HIP_TRY(hipMemsetAsync(changed, 0, (size_t)n_meshes * sizeof(int32_t), s));
    if (n_rows == 0) return MORIG_OK;
    MORIG_HIP_TRY(hipMemcpyAsync(next, cur, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    mc_cc_round_kernel<<<cdiv((long long)n_rows + n_keys, 256), 256, 0, s>>>(cur, next, n_rows, (const long long*)ekeys, n_keys, vptr, n_meshes, changed);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_edge_classify(const int64_t* keys, int64_t n_keys, const int32_t* label, int32_t n_rows, int32_t* eclass, int32_t* root_boundary,
                                  void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_keys)) return MORIG_E_INVALID;
    if (n_rows == 0 && n_keys == 0) return MORIG_OK;
    if ((n_rows > 0 && (!label || !root_boundary)) || (n_keys > 0 && (!keys || !eclass || n_rows == 0))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_rows > 0) MORIG_HIP_TRY(hipMemsetAsync(root_boundary, 0, (size_t)n_rows * sizeof(int32_t), s));
    if (n_keys == 0) return MORIG_OK;
    ProfScope ps(K_MESHCHECK_EDGES, s, 0.0, 28.0 * (double)n_keys);
    mc_edge_classify_kernel<<<cdiv(n_keys, 256), 256, 0, s>>>((const long long*)keys, n_keys, label, n_rows, eclass, root_boundary);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_comp_counts(const int32_t* tri, const int32_t* surv, int32_t n_faces, const int32_t* referenced, const int32_t* label,
                                int32_t n_rows, int32_t* root_verts, int32_t* root_faces, int64_t* face_root, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_faces) || !rows_ok((long long)n_rows + n_faces)) return MORIG_E_INVALID;
    if (n_rows == 0 && n_faces == 0) return MORIG_OK;
    if ((n_rows > 0 && (!referenced || !label || !root_verts || !root_faces)) || (n_faces > 0 && (!tri || !surv || !face_root))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_rows > 0) {
        MORIG_HIP_TRY(hipMemsetAsync(root_verts, 0, (size_t)n_rows * sizeof(int32_t), s));
        MORIG_HIP_TRY(hipMemsetAsync(root_faces, 0, (size_t)n_rows * sizeof(int32_t), s));
    }
    ProfScope ps(K_MESHCHECK_COMPONENTS, s, 0.0, 16.0 * (double)n_rows + 32.0 * (double)n_faces);
    mc_comp_counts_kernel<<<cdiv((long long)n_rows + n_faces, 256), 256, 0, s>>>(tri, surv, n_faces, referenced, label, n_rows, root_verts, root_faces,
                                                                                 (long long*)face_root);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_comp_area(const double* verts, int32_t n_rows, const int32_t* tri, int32_t n_faces, const int64_t* order, const int64_t* kptr,
                              int32_t n_comps, double* area, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_faces) || !rows_ok(n_comps)) return MORIG_E_INVALID;
    if (n_comps == 0) return MORIG_OK;
    if (!verts || !tri || !order || !kptr || !area) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_COMPONENTS, s, 0.0, 92.0 * (double)n_faces);
    mc_comp_area_kernel<<<cdiv(n_comps, 4), 256, 0, s>>>(verts, n_rows, tri, n_faces, (const long long*)order, (const long long*)kptr, n_comps, area);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_keep_flags(const int32_t* rep, const int32_t* referenced, const int32_t* label, const int32_t* keep_root, int32_t drop_unreferenced,
                               int32_t n_rows, const int32_t* tri, const int32_t* surv, int32_t n_faces, int32_t* vkeep, int32_t* fkeep, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_faces) || !rows_ok((long long)n_rows + n_faces)) return MORIG_E_INVALID;
    if (n_rows == 0 && n_faces == 0) return MORIG_OK;
    if ((n_rows > 0 && (!rep || !referenced || !label || !keep_root || !vkeep)) || (n_faces > 0 && (!tri || !surv || !fkeep || n_rows == 0)))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_COMPACT, s, 0.0, 24.0 * (double)n_rows + 24.0 * (double)n_faces);
    mc_keep_flags_kernel<<<cdiv((long long)n_rows + n_faces, 256), 256, 0, s>>>(rep, referenced, label, keep_root, drop_unreferenced, n_rows, tri, surv,
                                                                                n_faces, vkeep, fkeep);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshcheck_compact(const double* verts, const int32_t* rep, const int32_t* vkeep, const int64_t* vrank, const int32_t* vptr,
                            const int64_t* ovptr, int32_t n_rows, int32_t n_meshes, const int32_t* tri, const int32_t* surv, const int32_t* fkeep,
                            const int64_t* frank, const int32_t* fptr, const int64_t* ofptr, int32_t n_faces, int64_t n_out_v, int64_t n_out_f,
                            double* out_verts, int64_t* out_faces, int64_t* vertex_map, int64_t* face_map, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_faces) || !rows_ok((long long)n_rows + n_faces) || n_meshes < 0 || n_out_v < 0 || n_out_v > n_rows ||
        n_out_f < 0 || n_out_f > n_faces)
        return MORIG_E_INVALID;
    if (n_meshes == 0 || (n_rows == 0 && n_faces == 0)) return MORIG_OK;
    if (!vptr || !fptr || !ovptr || !ofptr || (n_rows > 0 && (!verts || !rep || !vkeep || !vrank || !vertex_map)) ||
        (n_faces > 0 && (!tri || !surv || !fkeep || !frank || !face_map || n_rows == 0)) || (n_out_v > 0 && !out_verts) || (n_out_f > 0 && !out_faces))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHCHECK_COMPACT, s, 0.0, 52.0 * (double)n_rows + 44.0 * (double)n_faces + 24.0 * (double)(n_out_v + n_out_f));
    mc_compact_kernel<<<cdiv((long long)n_rows + n_faces, 256), 256, 0, s>>>(verts, rep, vkeep, (const long long*)vrank, vptr, (const long long*)ovptr, n_rows,
                                                                             n_meshes, tri, surv, fkeep, (const long long*)frank, fptr,
                                                                             (const long long*)ofptr, n_faces, n_out_v, n_out_f, out_verts,
                                                                             (long long*)out_faces, (long long*)vertex_map, (long long*)face_map);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
