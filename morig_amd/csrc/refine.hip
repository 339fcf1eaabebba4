// Mesh refinement (morig_amd/meshprep.py refine / interpolate) for a ragged batch: one pass of edge splits, and
// the interpolation of per-vertex values along the parents. The idiom is meshcheck.hip's: a kernel emits 64-bit keys, the caller sorts
// them (torch.sort) and marks the runs (morig_tpl_edge_flags), a kernel reads the runs. Integers or float64 in the written order
// (contraction off); the only atomics are one integer max (on the bit patterns of non-negative doubles, whose order is numeric order) and
// one integer OR, whose results do not depend on order. Nothing depends on one workgroup seeing another's store inside a launch.
//
// edge records   one thread per face: three (undirected key, squared length) records; the largest finite squared length of every mesh,
//                reduced over the wave first where the wave lies in one mesh.
// mark           one thread per sorted record: the first record of a run decides for the edge, by the mode and threshold of its mesh.
// budget         one thread per position of the records ordered by (mesh, length descending, key): marks behind the budget are cleared.
// number         the thread of a marked run start walks its run and gives every record the new vertex of the edge.
// pattern        one thread per face: how many of its edges are marked, how many children it has.
// emit           three launches: the old rows at their new places, the new vertices with their parents, the children of every face
//                (split_core.h) at the prefix sum of the child counts.
// interpolate    one thread per 16 bytes (or per element) of the rows of one pass level.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the core header: its functions are compiled under it too

#include "split_core.h"

namespace morig {

namespace {

using namespace morig_topo;
using namespace morig_split;

__global__ void __launch_bounds__(256) rf_edge_records_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ faces, int n_faces,
                                                              const int* __restrict__ fptr, const int* __restrict__ vptr, int n_meshes,
                                                              long long* __restrict__ keys, double* __restrict__ len2_out,
                                                              long long* __restrict__ maxbits, int* __restrict__ degenerate, int* __restrict__ status) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const bool live = f < n_faces;
    int b = -1;
    long long top = -1;
    if (live) {
        b = segment_of(fptr, n_meshes, f);
        int v0 = vptr[b], nv = vptr[b + 1] - v0;
        if (v0 < 0 || nv < 0 || (long long)v0 + nv > n_rows) nv = 0;
        long long r[3];
        bool inside = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int id = faces[(size_t)f * 3 + c];
            r[c] = 0;
            if (id < 0 || id >= nv) { inside = false; continue; }
            r[c] = (long long)v0 + id;
        }
        const bool twice = inside && (r[0] == r[1] || r[1] == r[2] || r[0] == r[2]);
        const bool ok = inside && !twice;
        if (!inside) atomicOr(status, MORIG_MESHCHECK_BAD_FACE);
        degenerate[f] = twice ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            long long k = KEY_NONE;
            double l2 = 0.0;
            if (ok) {
                const long long a = r[c], d = r[(c + 1) % 3];
                const long long lo = a < d ? a : d, hi = a < d ? d : a;
                k = split_key(lo, hi);
                l2 = len2(verts + (size_t)hi * 3, verts + (size_t)lo * 3);
                const long long image = len2_image(l2);
                top = image > top ? image : top;
            }
            keys[(size_t)f * 3 + c] = k;
            len2_out[(size_t)f * 3 + c] = l2;
        }
    }
    // one atomic per wave where all its live faces lie in one mesh, else one per face
    int bl = live ? b : 0x7fffffff, bh = b;
    long long wtop = top;
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        const int ol = __shfl_xor(bl, h), oh = __shfl_xor(bh, h);
        const long long ot = __shfl_xor(wtop, h);
        bl = ol < bl ? ol : bl;
        bh = oh > bh ? oh : bh;
        wtop = ot > wtop ? ot : wtop;
    }
    if (bl == bh) {
        if ((threadIdx.x & 63) == 0 && bh >= 0 && wtop > 0) atomicMax(maxbits + bh, wtop);
    } else if (live && top > 0) {
        atomicMax(maxbits + b, top);
    }
}

// the mesh of the batch row ``row`` (0 <= row < vptr[n_meshes]) or -1
__device__ __forceinline__ int mesh_of_row(const int* __restrict__ vptr, int n_meshes, long long row) {
    if (row < 0 || row >= vptr[n_meshes]) return -1;
    return segment_of(vptr, n_meshes, (int)row);
}

__global__ void __launch_bounds__(256) rf_mark_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                      const int* __restrict__ flags, const double* __restrict__ len2_in, long long n_records,
                                                      const int* __restrict__ vptr, int n_meshes, const int* __restrict__ mode, double limit2,
                                                      const long long* __restrict__ maxbits, int* __restrict__ mark, long long* __restrict__ image) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records) return;
    int m = 0;
    long long im = -1;
    const long long k = keys[i], o = order[i];
    if (flags[i] && k != KEY_NONE && k >= 0 && o >= 0 && o < n_records) {
        const int b = mesh_of_row(vptr, n_meshes, k >> 32);
        if (b >= 0) {
            const double l2 = len2_in[o];
            const int md = mode[b];
            const long long bits = len2_image(l2);
            bool over = false;
            if (md == MORIG_REFINE_LENGTH) over = l2 > limit2;
            else if (md == MORIG_REFINE_LONGEST) over = l2 > 0.25 * image_len2(maxbits[b] > 0 ? maxbits[b] : 0);
            if (bits >= 0 && over) { m = 1; im = bits; }
        }
    }
    mark[i] = m;
    image[i] = im;
}

__global__ void __launch_bounds__(256) rf_budget_kernel(const long long* __restrict__ perm, long long n_records, const long long* __restrict__ rptr,
                                                        const long long* __restrict__ budget, int n_meshes, int* __restrict__ mark) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_records || j >= rptr[n_meshes] || j < rptr[0]) return;
    const int b = segment_of(rptr, n_meshes, j);
    const long long p = perm[j];
    if (p >= 0 && p < n_records && j - rptr[b] >= budget[b]) mark[p] = 0;
}

__global__ void __launch_bounds__(256) rf_number_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                        const int* __restrict__ mark, const long long* __restrict__ erank, long long n_records,
                                                        const int* __restrict__ vptr, const long long* __restrict__ mptr, int n_meshes,
                                                        int* __restrict__ edge_mid) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records || !mark[i]) return;
    const long long k = keys[i];
    if (k == KEY_NONE || k < 0) return;
    const int b = mesh_of_row(vptr, n_meshes, k >> 32);
    if (b < 0) return;
    const long long local = (long long)(vptr[b + 1] - vptr[b]) + erank[i] - 1 - mptr[b];
    if (local < 0 || local > 0x7fffffffLL - 257) return;
    for (long long j = i; j < n_records && keys[j] == k; ++j) {
        const long long o = order[j];
        if (o >= 0 && o < n_records) edge_mid[o] = (int)local;
    }
}

__global__ void __launch_bounds__(256) rf_pattern_kernel(const int* __restrict__ edge_mid, const int* __restrict__ degenerate, int n_faces,
                                                         int* __restrict__ nchild, int* __restrict__ pattern) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int mid[3] = {edge_mid[(size_t)f * 3], edge_mid[(size_t)f * 3 + 1], edge_mid[(size_t)f * 3 + 2]};
    const int mask = degenerate[f] ? 0 : mask_of(mid);
    pattern[f] = marked_edges(mask);
    nchild[f] = child_count(mask);
}

__global__ void __launch_bounds__(256) rf_emit_rows_kernel(const double* __restrict__ verts, const long long* __restrict__ parents, int n_rows,
                                                           const int* __restrict__ vptr, const long long* __restrict__ mptr, int n_meshes,
                                                           long long n_out_rows, double* __restrict__ out_verts, long long* __restrict__ out_parents) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int b = mesh_of_row(vptr, n_meshes, v);
    if (b < 0) return;
    const long long at = (long long)v + mptr[b];
    if (at < 0 || at >= n_out_rows) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) out_verts[(size_t)at * 3 + d] = verts[(size_t)v * 3 + d];
    out_parents[(size_t)at * 2] = parents[(size_t)v * 2];
    out_parents[(size_t)at * 2 + 1] = parents[(size_t)v * 2 + 1];
}

__global__ void __launch_bounds__(256) rf_emit_mids_kernel(const double* __restrict__ verts, int n_rows, const long long* __restrict__ keys,
                                                           const int* __restrict__ mark, const long long* __restrict__ erank, long long n_records,
                                                           const int* __restrict__ vptr, int n_meshes, long long n_out_rows,
                                                           double* __restrict__ out_verts, long long* __restrict__ out_parents) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records || !mark[i]) return;
    const long long k = keys[i];
    if (k == KEY_NONE || k < 0) return;
    const long long lo = k >> 32, hi = k & 0xffffffffLL;
    const int b = mesh_of_row(vptr, n_meshes, lo);
    if (b < 0 || hi >= n_rows) return;
    const long long at = (long long)vptr[b + 1] + erank[i] - 1;
    if (at < 0 || at >= n_out_rows) return;
    double m[3];
    midpoint(verts + (size_t)lo * 3, verts + (size_t)hi * 3, m);
#pragma unroll
    for (int d = 0; d < 3; ++d) out_verts[(size_t)at * 3 + d] = m[d];
    out_parents[(size_t)at * 2] = lo - vptr[b];
    out_parents[(size_t)at * 2 + 1] = hi - vptr[b];
}

__global__ void __launch_bounds__(256) rf_emit_faces_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ faces,
                                                            const long long* __restrict__ face_map, const int* __restrict__ edge_mid,
                                                            const long long* __restrict__ crank, int n_faces, const int* __restrict__ fptr,
                                                            const int* __restrict__ vptr, int n_meshes, long long n_out_faces,
                                                            int* __restrict__ out_faces, long long* __restrict__ out_face_map) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    int v0 = vptr[b], nv = vptr[b + 1] - v0;
    if (v0 < 0 || nv < 0 || (long long)v0 + nv > n_rows) nv = 0;
    long long v[3], mid[3];
    int m32[3];
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = faces[(size_t)f * 3 + c];
        m32[c] = edge_mid[(size_t)f * 3 + c];
        mid[c] = m32[c];
        inside = inside && v[c] >= 0 && v[c] < nv;
    }
    const int mask = inside ? mask_of(m32) : 0;                                        // a marked edge has both ends inside
    const int n = child_count(mask);
    const long long at = crank[f] - n;
    if (at < 0 || at + n > n_out_faces) return;
    int diag = 0;
    if (marked_edges(mask) == 2) {
        const int r = rotation(mask);
        const long long ia = v[r], ib = v[(r + 1) % 3], ic = v[(r + 2) % 3];
        const double* pa = verts + (size_t)(v0 + ia) * 3;
        const double* pb = verts + (size_t)(v0 + ib) * 3;
        const double* pc = verts + (size_t)(v0 + ic) * 3;
        diag = frame_diagonal(pa, pb, pc, ib, ic);
    }
    long long out[4][3];
    const int made = children(v, mid, mask, diag, out);
    const long long origin = face_map[f];
    for (int k = 0; k < made; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out_faces[(size_t)(at + k) * 3 + c] = (int)out[k][c];
        out_face_map[at + k] = origin;
    }
}

template <class T, int VEC> struct alignas(sizeof(T) * VEC) Pack { T x[VEC]; };

template <class T, int VEC>
__global__ void __launch_bounds__(256) rf_interpolate_kernel(T* values, long long per_row, const long long* __restrict__ parents,
                                                             long long row0, long long n_work) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_work) return;
    const long long r = row0 + w / per_row, e = w % per_row;
    const long long p0 = parents[(size_t)r * 2], p1 = parents[(size_t)r * 2 + 1];
    if (p0 < 0 || p0 >= row0 || p1 < 0 || p1 >= row0) return;
    using P = Pack<T, VEC>;
    const P* src = reinterpret_cast<const P*>(values);
    const P a = src[(size_t)p0 * per_row + e], b = src[(size_t)p1 * per_row + e];
    P out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) out.x[k] = (T)0.5 * (a.x[k] + b.x[k]);
    reinterpret_cast<P*>(values)[(size_t)r * per_row + e] = out;
}

inline bool rows_ok(long long n) { return n >= 0 && n <= 0x7fffffffLL - 256; }
constexpr int MAX_FACES = (0x7fffffff - 256) / 3;

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_refine_edge_records(const double* verts, int32_t n_rows, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr,
                              int32_t n_meshes, int64_t* keys, double* len2, int64_t* maxbits, int32_t* degenerate, int32_t* status, void* stream) {
    if (n_faces < 0 || n_faces > MAX_FACES || !rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!maxbits) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(maxbits, 0, (size_t)n_meshes * sizeof(int64_t), s));
    if (n_faces == 0) return MORIG_OK;
    if (!verts || !faces || !fptr || !vptr || !keys || !len2 || !degenerate || !status) return MORIG_E_INVALID;
    ProfScope ps(K_REFINE_EDGES, s, 24.0 * (double)n_faces, 136.0 * (double)n_faces);
    rf_edge_records_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(verts, n_rows, faces, n_faces, fptr, vptr, n_meshes, (long long*)keys, len2,
                                                              (long long*)maxbits, degenerate, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_refine_mark(const int64_t* keys, const int64_t* order, const int32_t* flags, const double* len2, int64_t n_records, const int32_t* vptr,
                      int32_t n_meshes, const int32_t* mode, double limit2, const int64_t* maxbits, int32_t* mark, int64_t* image, void* stream) {
    if (!rows_ok(n_records) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_records == 0) return MORIG_OK;
    if (n_meshes == 0 || !keys || !order || !flags || !len2 || !vptr || !mode || !maxbits || !mark || !image) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_REFINE_EDGES, s, 0.0, 40.0 * (double)n_records);
    rf_mark_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)keys, (const long long*)order, flags, len2, n_records, vptr, n_meshes, mode,
                                                        limit2, (const long long*)maxbits, mark, (long long*)image);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_refine_budget(const int64_t* perm, int64_t n_records, const int64_t* rptr, const int64_t* budget, int32_t n_meshes, int32_t* mark,
                        void* stream) {
    if (!rows_ok(n_records) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_records == 0 || n_meshes == 0) return MORIG_OK;
    if (!perm || !rptr || !budget || !mark) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_REFINE_EDGES, s, 0.0, 12.0 * (double)n_records);
    rf_budget_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)perm, n_records, (const long long*)rptr, (const long long*)budget, n_meshes,
                                                          mark);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_refine_number(const int64_t* keys, const int64_t* order, const int32_t* mark, const int64_t* erank, int64_t n_records, const int32_t* vptr,
                        const int64_t* mptr, int32_t n_meshes, int32_t* edge_mid, void* stream) {
    if (!rows_ok(n_records) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_records == 0) return MORIG_OK;
    if (n_meshes == 0 || !keys || !order || !mark || !erank || !vptr || !mptr || !edge_mid) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(edge_mid, 0xff, (size_t)n_records * sizeof(int32_t), s));
    ProfScope ps(K_REFINE_EDGES, s, 0.0, 32.0 * (double)n_records);
    rf_number_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)keys, (const long long*)order, mark, (const long long*)erank, n_records, vptr,
                                                          (const long long*)mptr, n_meshes, edge_mid);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_refine_pattern(const int32_t* edge_mid, const int32_t* degenerate, int32_t n_faces, int32_t* nchild, int32_t* pattern, void* stream) {
    if (n_faces < 0 || n_faces > MAX_FACES) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!edge_mid || !degenerate || !nchild || !pattern) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_REFINE_EDGES, s, 0.0, 24.0 * (double)n_faces);
    rf_pattern_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(edge_mid, degenerate, n_faces, nchild, pattern);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_refine_emit(const double* verts, const int64_t* parents, int32_t n_rows, const int32_t* faces, const int64_t* face_map,
                      const int32_t* edge_mid, const int64_t* crank, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, const int64_t* mptr,
                      int32_t n_meshes, const int64_t* keys, const int32_t* mark, const int64_t* erank, int64_t n_records, int64_t n_out_rows,
                      int64_t n_out_faces, double* out_verts, int64_t* out_parents, int32_t* out_faces, int64_t* out_face_map, void* stream) {
    if (!rows_ok(n_rows) || n_faces < 0 || n_faces > MAX_FACES || n_meshes < 0 || n_records != 3LL * n_faces) return MORIG_E_INVALID;
    if (!rows_ok(n_out_rows) || n_out_rows < n_rows || n_out_rows > (long long)n_rows + n_records) return MORIG_E_INVALID;
    if (n_out_faces < n_faces || n_out_faces > 4LL * n_faces || n_out_faces > MAX_FACES) return MORIG_E_INVALID;
    if (n_meshes == 0 || (n_rows == 0 && n_faces == 0)) return MORIG_OK;
    if (!vptr || !mptr || (n_out_rows > 0 && (!verts || !parents || !out_verts || !out_parents))) return MORIG_E_INVALID;
    if (n_faces > 0 && (!faces || !face_map || !edge_mid || !crank || !fptr || !keys || !mark || !erank || !out_faces || !out_face_map || n_rows == 0))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_REFINE_EMIT, s, 3.0 * (double)(n_out_rows - n_rows), 80.0 * (double)n_out_rows + 60.0 * (double)n_faces + 20.0 * (double)n_out_faces);
    if (n_rows > 0) {
        rf_emit_rows_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, (const long long*)parents, n_rows, vptr, (const long long*)mptr, n_meshes, n_out_rows,
                                                              out_verts, (long long*)out_parents);
        MORIG_LAUNCH_CHECK();
    }
    if (n_faces > 0) {
        rf_emit_mids_kernel<<<cdiv(n_records, 256), 256, 0, s>>>(verts, n_rows, (const long long*)keys, mark, (const long long*)erank, n_records, vptr,
                                                                 n_meshes, n_out_rows, out_verts, (long long*)out_parents);
        MORIG_LAUNCH_CHECK();
        rf_emit_faces_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(verts, n_rows, faces, (const long long*)face_map, edge_mid, (const long long*)crank, n_faces,
                                                                fptr, vptr, n_meshes, n_out_faces, out_faces, (long long*)out_face_map);
        MORIG_LAUNCH_CHECK();
    }
    return MORIG_OK;
}

int morig_refine_interpolate(void* values, int32_t elt_size, int64_t row_len, const int64_t* parents, int64_t row0, int64_t row1, int64_t n_rows,
                             void* stream) {
    if ((elt_size != 4 && elt_size != 8) || row_len < 0 || n_rows < 0 || row0 < 0 || row1 < row0 || row1 > n_rows) return MORIG_E_INVALID;
    if (row_len > 0 && n_rows > (0x7fffffffffffffffLL / 16) / row_len) return MORIG_E_INVALID;      // byte offsets stay in 63 bits
    if (row1 == row0 || row_len == 0) return MORIG_OK;
    if (!values || !parents) return MORIG_E_INVALID;
    const bool wide = ((row_len * elt_size) % 16 == 0) && ((uintptr_t)values & 15) == 0;
    const long long per_row = wide ? row_len * elt_size / 16 : row_len;
    const long long n_work = (row1 - row0) * per_row;
    if (n_work > (0x7fffffffLL - 256) * 256) return MORIG_E_INVALID;                                // the grid
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_REFINE_INTERPOLATE, s, 2.0 * (double)(row1 - row0) * (double)row_len, 3.0 * (double)(row1 - row0) * (double)row_len * elt_size);
    const int grid = cdiv(n_work, 256);
    const long long* par = (const long long*)parents;
    if (elt_size == 4 && wide) rf_interpolate_kernel<float, 4><<<grid, 256, 0, s>>>((float*)values, per_row, par, row0, n_work);
    else if (elt_size == 4) rf_interpolate_kernel<float, 1><<<grid, 256, 0, s>>>((float*)values, per_row, par, row0, n_work);
    else if (wide) rf_interpolate_kernel<double, 2><<<grid, 256, 0, s>>>((double*)values, per_row, par, row0, n_work);
    else rf_interpolate_kernel<double, 1><<<grid, 256, 0, s>>>((double*)values, per_row, par, row0, n_work);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
