// Mesh simplification (morig_amd/meshprep.py simplify): vertex clustering on a per-mesh grid of resolution r with a
// regularised quadric representative per occupied cell, for a ragged batch of meshes. Everything is float64 in the written order of
// operations (contraction off) or integer, and there are no atomics: two runs give the same bits, and a mesh alone gives the bits it gives
// inside a batch.
//
// cell keys     one thread per vertex: mesh << 30 | ((cx r + cy) r + cz). The caller sorts them stably, marks the first key of every run
//               (morig_tpl_edge_flags) and numbers the runs across the call: that number is the vertex's cell, the output vertex.
// face keys     one thread per face: the cells of its corners (for the corner sort of the quadrics) and the ascending triple of them at 21
//               bits each, INT64_MAX where two corners share a cell. The caller sorts stably and marks the runs again.
// face compact  one thread per sorted position: a marked face leaves as mesh-local cells in its input orientation, smallest first.
// quadrics      one wave per cell. Lane l adds the members l, l + 64, ... of the cell's run in ascending order, the lanes are added by a
//               butterfly of __shfl_xor (a + b == b + a, so every lane ends on the same bits): the centroid. The same for the nine sums of
//               quadric_core.h over the cell's run of corners; lane 0 solves, clamps and stores. Runs are ragged -- one corner up to the
//               whole mesh at r = 1 -- and a wave walks a long run in 64-wide strides; the order of every sum depends on the run alone.
//               At the sizes the networks take (r about 20 to 40, a dozen corners per cell) most lanes idle, which is cheap next to the two
//               dependent gathers (face row, vertex row) every corner costs: the kernel is bound by their latency, hidden by the
//               thousands of independent waves of a batch.
#include "common.h"

#pragma clang fp contract(off)                 // in front of quadric_core.h: its functions are compiled under it too

#include "quadric_core.h"

namespace morig {

namespace {

constexpr long long KEY_SENTINEL = 0x7fffffffffffffffLL;
constexpr int BITS = MORIG_SIMPLIFY_INDEX_BITS;
constexpr long long CELL_MASK = (1LL << MORIG_SIMPLIFY_MESH_SHIFT) - 1;

__global__ void __launch_bounds__(256) simplify_cell_keys_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ vptr,
                                                                 int n_meshes, const double* __restrict__ frame, const int* __restrict__ res,
                                                                 long long* __restrict__ keys) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int b = segment_of(vptr, n_meshes, v);
    int r = res[b];
    r = r < 1 ? 1 : (r > MORIG_SIMPLIFY_MAX_RES ? MORIG_SIMPLIFY_MAX_RES : r);             // the launcher refused anything else
    const double ext = frame[(size_t)b * 4 + 3];
    long long c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = morig_quadric::cell_coord(verts[(size_t)v * 3 + k], frame[(size_t)b * 4 + k], ext, r);
    keys[v] = ((long long)b << MORIG_SIMPLIFY_MESH_SHIFT) | ((c[0] * r + c[1]) * r + c[2]);
}

// the cells of a face's corners, or false where the face is never followed
__device__ __forceinline__ bool face_cells(const int* __restrict__ faces, long long f, int v0, int nv, const int* __restrict__ cell, int n_cells,
                                           int* c) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int id = faces[(size_t)f * 3 + k];
        if (id < 0 || id >= nv) { ok = false; c[k] = -1; continue; }
        c[k] = cell[v0 + id];
        if (c[k] < 0 || c[k] >= n_cells) ok = false;
    }
    return ok;
}

__global__ void __launch_bounds__(256) simplify_face_keys_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                                 const int* __restrict__ vptr, int n_meshes, const int* __restrict__ cell,
                                                                 int n_rows, int n_cells, int* __restrict__ corner_cell,
                                                                 long long* __restrict__ keys) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    int v0 = vptr[b], nv = vptr[b + 1] - v0;
    if (v0 < 0 || nv < 0 || (long long)v0 + nv > n_rows) nv = 0;
    int c[3];
    const bool ok = face_cells(faces, f, v0, nv, cell, n_cells, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) corner_cell[(size_t)f * 3 + k] = ok ? c[k] : -1;
    long long key = KEY_SENTINEL;
    if (ok && c[0] != c[1] && c[1] != c[2] && c[0] != c[2]) {
        const long long lo = min(c[0], min(c[1], c[2])), hi = max(c[0], max(c[1], c[2]));
        const long long mid = (long long)c[0] + c[1] + c[2] - lo - hi;
        key = (lo << (2 * BITS)) | (mid << BITS) | hi;
    }
    keys[f] = key;
}

__global__ void __launch_bounds__(256) simplify_face_compact_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                                    const int* __restrict__ vptr, int n_meshes, const int* __restrict__ cell,
                                                                    const int* __restrict__ cptr, const long long* __restrict__ order,
                                                                    const int* __restrict__ flags, const long long* __restrict__ rank,
                                                                    long long n_out, long long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_faces || !flags[i]) return;
    const long long at = rank[i] - 1, f = order[i];
    if (at < 0 || at >= n_out || f < 0 || f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    const int v0 = vptr[b], nv = vptr[b + 1] - v0, c0 = cptr[b], nc = cptr[b + 1] - c0;
    int c[3];
    if (!face_cells(faces, f, v0, nv, cell, c0 + nc, c)) return;                       // never marked: its key is the sentinel
    const int first = (c[0] <= c[1] && c[0] <= c[2]) ? 0 : (c[1] <= c[2] ? 1 : 2);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[at * 3 + k] = (long long)c[(first + k) % 3] - c0;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}

__device__ __forceinline__ long long clampll(long long x, long long lo, long long hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(256) simplify_quadrics_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ vptr,
                                                                const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                                int n_meshes, const double* __restrict__ frame, const int* __restrict__ res,
                                                                const long long* __restrict__ cell_key, const long long* __restrict__ mptr,
                                                                const long long* __restrict__ members, const long long* __restrict__ kptr,
                                                                const long long* __restrict__ corners, int n_cells, double* __restrict__ out) {
    const int cell = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (cell >= n_cells) return;                                                       // the whole wave
    const long long key = cell_key[cell];
    const long long b = key >> MORIG_SIMPLIFY_MESH_SHIFT;
    double x[3] = {0.0, 0.0, 0.0};
    bool good = b >= 0 && b < n_meshes;
    int r = good ? res[b] : 1;
    good = good && r >= 1 && r <= MORIG_SIMPLIFY_MAX_RES;
    if (!good) r = 1;
    const long long ck = key & CELL_MASK;
    const int c[3] = {(int)(ck / ((long long)r * r)), (int)((ck / r) % r), (int)(ck % r)};
    good = good && c[0] < r;
    if (good) {                                                                        // uniform over the wave
        const int v0 = vptr[b], nv = vptr[b + 1] - v0, f0 = fptr[b], nf = fptr[b + 1] - f0;
        const bool tables = v0 >= 0 && nv >= 0 && (long long)v0 + nv <= n_rows && f0 >= 0 && nf >= 0 && (long long)f0 + nf <= n_faces;
        const long long m0 = clampll(mptr[cell], 0, n_rows), m1 = clampll(mptr[cell + 1], m0, n_rows);
        const long long k0 = clampll(kptr[cell], 0, 3LL * n_faces), k1 = clampll(kptr[cell + 1], k0, 3LL * n_faces);
        double s[3] = {0.0, 0.0, 0.0};
        for (long long i = m0 + lane; i < m1; i += 64) {
            const long long v = members[i];
            if (!tables || v < v0 || v >= (long long)v0 + nv) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = s[k] + verts[(size_t)v * 3 + k];
        }
        double cen[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = wave_sum(s[k]) / (double)(m1 - m0);
        morig_quadric::Acc acc;
        morig_quadric::zero(acc);
        for (long long i = k0 + lane; i < k1; i += 64) {
            const long long f = corners[i] / 3;
            if (!tables || corners[i] < 0 || f < f0 || f >= (long long)f0 + nf) continue;
            const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
            if (ia < 0 || ib < 0 || ic < 0 || ia >= nv || ib >= nv || ic >= nv) continue;
            morig_quadric::corner(verts + (size_t)(v0 + ia) * 3, verts + (size_t)(v0 + ib) * 3, verts + (size_t)(v0 + ic) * 3, cen, acc);
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) acc.q[q] = wave_sum(acc.q[q]);
        const double ext = frame[(size_t)b * 4 + 3];
        morig_quadric::solve_clamp(acc, cen, frame + (size_t)b * 4, ext / (double)r, c, x);
    }
    if (lane < 3) out[(size_t)cell * 3 + lane] = lane == 0 ? x[0] : (lane == 1 ? x[1] : x[2]);
}

int res_status(int32_t min_res, int32_t max_res) {
    return (min_res < 1 || max_res > MORIG_SIMPLIFY_MAX_RES || min_res > max_res) ? MORIG_E_UNSUPPORTED : MORIG_OK;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_simplify_cell_keys(const double* verts, int32_t n_rows, const int32_t* vptr, int32_t n_meshes, const double* frame, const int32_t* res,
                             int32_t min_res, int32_t max_res, int64_t* keys, void* stream) {
    if (n_rows < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (res_status(min_res, max_res) != MORIG_OK || n_rows > MORIG_SIMPLIFY_MAX_INDEX || n_meshes > MORIG_SIMPLIFY_MAX_INDEX) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0 || n_rows == 0) return MORIG_OK;
    if (!verts || !vptr || !frame || !res || !keys) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SIMPLIFY_KEYS, s, 0.0, 32.0 * (double)n_rows);
    simplify_cell_keys_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, n_rows, vptr, n_meshes, frame, res, (long long*)keys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_simplify_face_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* cell,
                             int32_t n_rows, int32_t n_cells, int32_t* corner_cell, int64_t* keys, void* stream) {
    if (n_faces < 0 || n_meshes < 0 || n_rows < 0 || n_cells < 0 || n_faces > (1 << 28)) return MORIG_E_INVALID;
    if (n_rows > MORIG_SIMPLIFY_MAX_INDEX || n_cells > MORIG_SIMPLIFY_MAX_INDEX) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0 || n_faces == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !cell || !corner_cell || !keys) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SIMPLIFY_KEYS, s, 0.0, 44.0 * (double)n_faces);
    simplify_face_keys_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, cell, n_rows, n_cells, corner_cell,
                                                                 (long long*)keys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_simplify_face_compact(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes,
                                const int32_t* cell, const int32_t* cptr, const int64_t* order, const int32_t* flags, const int64_t* rank,
                                int64_t n_out, int64_t* out, void* stream) {
    if (n_faces < 0 || n_meshes < 0 || n_out < 0 || n_out > n_faces || n_faces > (1 << 28)) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_faces == 0 || n_out == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !cell || !cptr || !order || !flags || !rank || !out) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SIMPLIFY_KEYS, s, 0.0, 32.0 * (double)n_faces + 24.0 * (double)n_out);
    simplify_face_compact_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, cell, cptr, (const long long*)order, flags,
                                                                    (const long long*)rank, n_out, (long long*)out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_simplify_quadrics(const double* verts, int32_t n_rows, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr,
                            int32_t n_meshes, const double* frame, const int32_t* res, int32_t min_res, int32_t max_res, const int64_t* cell_key,
                            const int64_t* mptr, const int64_t* members, const int64_t* kptr, const int64_t* corners, int32_t n_cells,
                            double* out, void* stream) {
    if (n_rows < 0 || n_faces < 0 || n_meshes < 0 || n_cells < 0 || n_faces > (1 << 28)) return MORIG_E_INVALID;
    if (res_status(min_res, max_res) != MORIG_OK || n_rows > MORIG_SIMPLIFY_MAX_INDEX || n_cells > MORIG_SIMPLIFY_MAX_INDEX) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0 || n_cells == 0) return MORIG_OK;
    if (!verts || !vptr || !fptr || !frame || !res || !cell_key || !mptr || !members || !kptr || !out || (n_faces > 0 && (!faces || !corners)))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SIMPLIFY_QUADRICS, s, 0.0, 32.0 * (double)n_rows + 92.0 * 3.0 * (double)n_faces + 56.0 * (double)n_cells);
    simplify_quadrics_kernel<<<cdiv(n_cells, 4), 256, 0, s>>>(verts, n_rows, vptr, faces, n_faces, fptr, n_meshes, frame, res,
                                                              (const long long*)cell_key, (const long long*)mptr, (const long long*)members,
                                                              (const long long*)kptr, (const long long*)corners, n_cells, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
