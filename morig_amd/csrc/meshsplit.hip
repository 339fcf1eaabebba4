// Splitting non-manifold edges and pinched vertices (morig_amd/meshprep.py split_nonmanifold) for a ragged batch of
// CLEANED meshes: every FAN of faces around a vertex gets its own copy of that vertex. The idiom is meshfix.hip's: the caller sorts the
// face edge records of morig_meshfix_edge_records (torch.sort), a kernel reads the runs. Integers only; the only atomics are an integer
// minimum and an integer add, whose result does not depend on order. Nothing depends on one workgroup seeing another's store inside a
// launch.
//
// links   one thread per sorted record. It reads at most two records on either side (orient_core.h run_shape), so a run of any length,
//         across any workgroup boundary, costs every record the same. A run of two links the corners of its two faces at the low end of
//         the edge (first record) and at the high end (second record), in the key layout of morig_meshcheck_cc_round, which then labels
//         the 3 F corner nodes unchanged. The first record of a run of three or more is a non-manifold edge.
// fans    one thread per node: a node that is its own label is a fan; it lowers ``first`` of its vertex and counts itself there.
// apply   one thread per node and one per input row: the output index of every corner, and the output vertices with their source.
#include "common.h"

#include "fan_core.h"

namespace morig {

namespace {

using namespace morig_topo;
using namespace morig_fan;

__global__ void __launch_bounds__(256) ms_links_kernel(const long long* __restrict__ keys, const int* __restrict__ vals,
                                                       const long long* __restrict__ order, long long n_records, int n_faces,
                                                       long long* __restrict__ links, int* __restrict__ nm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records) return;
    long long lk = KEY_NONE;
    int many = 0;
    const long long k = keys[i];
    const int val = vals[i];
    if (k != KEY_NONE && k >= 0 && val >= 0 && (val >> 1) < n_faces) {
        int count, pos;
        lk = fan_link(keys, vals, order, i, n_records, n_faces, &count, &pos);
        many = (count >= 3 && pos == 0) ? 1 : 0;
    }
    links[i] = lk;
    nm[i] = many;
}

__global__ void __launch_bounds__(256) ms_fans_kernel(const int* __restrict__ lab, const int* __restrict__ tri, long long n_nodes, int n_rows,
                                                      int* __restrict__ first, int* __restrict__ nfans) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nodes) return;
    const int v = tri[n];
    if (lab[n] != (int)n || v < 0 || v >= n_rows) return;
    atomicMin(first + v, (int)n);
    atomicAdd(nfans + v, 1);
}

// 64-bit words, not doubles: the bits of a coordinate travel as they are (a NaN keeps its payload)
__device__ __forceinline__ void copy_row(const long long* __restrict__ verts, long long from, long long* __restrict__ out, long long to) {
#pragma unroll
    for (int d = 0; d < 3; ++d) out[to * 3 + d] = verts[from * 3 + d];
}

__global__ void __launch_bounds__(256) ms_apply_kernel(const int* __restrict__ lab, const int* __restrict__ tri, const int* __restrict__ first,
                                                       const long long* __restrict__ rank, const int* __restrict__ fptr,
                                                       const int* __restrict__ vptr, const long long* __restrict__ aptr,
                                                       const long long* __restrict__ verts, long long n_nodes, int n_faces, int n_rows,
                                                       int n_meshes, long long n_out_rows, long long* __restrict__ out_faces,
                                                       long long* __restrict__ source, long long* __restrict__ out_verts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n_nodes) {
        long long local = -1;
        const int l = lab[t], v = tri[t];
        if (l >= 0 && l <= t && v >= 0 && v < n_rows) {
            const int b = segment_of(fptr, n_meshes, (int)(t / 3));
            const long long v0 = vptr[b], nv = vptr[b + 1] - v0, before = aptr[b];
            if (first[v] == l) {
                local = v - v0;
            } else {
                local = nv + (rank[l] - 1 - before);
                const long long row = v0 + before + local;
                if (l == t && local >= nv && row >= 0 && row < n_out_rows) {            // the fan's lowest node makes its vertex
                    source[row] = v - v0;
                    copy_row(verts, v, out_verts, row);
                }
            }
        }
        out_faces[t] = local;
    } else if (t - n_nodes < n_rows) {
        const int v = (int)(t - n_nodes);
        const int b = segment_of(vptr, n_meshes, v);
        const long long row = v + aptr[b];
        if (row >= 0 && row < n_out_rows) {
            source[row] = v - vptr[b];
            copy_row(verts, v, out_verts, row);
        }
    }
}

inline bool rows_ok(long long n) { return n >= 0 && n <= 0x7fffffffLL - 256; }

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_meshsplit_links(const int64_t* keys, const int32_t* vals, const int64_t* order, int64_t n_records, int32_t n_faces, int64_t* links,
                          int32_t* nm, void* stream) {
    if (!rows_ok(n_records) || !rows_ok(n_faces) || n_records > 3LL * n_faces) return MORIG_E_INVALID;
    if (n_records == 0) return MORIG_OK;
    if (!keys || !vals || !order || !links || !nm) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHSPLIT_LINKS, s, 0.0, 32.0 * (double)n_records);
    ms_links_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)keys, vals, (const long long*)order, n_records, n_faces, (long long*)links, nm);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshsplit_fans(const int32_t* lab, const int32_t* tri, int32_t n_faces, int32_t n_rows, int32_t* first, int32_t* nfans, void* stream) {
    if (n_faces < 0 || n_faces > (0x7fffffff - 256) / 3 || !rows_ok(n_rows)) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!first || !nfans || (n_faces > 0 && (!lab || !tri))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)first, 0x7fffffff, (size_t)n_rows, s));
    MORIG_HIP_TRY(hipMemsetAsync(nfans, 0, (size_t)n_rows * sizeof(int32_t), s));
    if (n_faces == 0) return MORIG_OK;
    const long long n_nodes = 3LL * n_faces;
    ProfScope ps(K_MESHSPLIT_LINKS, s, 0.0, 8.0 * (double)n_nodes + 8.0 * (double)n_rows);
    ms_fans_kernel<<<cdiv(n_nodes, 256), 256, 0, s>>>(lab, tri, n_nodes, n_rows, first, nfans);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshsplit_apply(const int32_t* lab, const int32_t* tri, const int32_t* first, const int64_t* rank, int32_t n_faces, const int32_t* fptr,
                          const int32_t* vptr, const int64_t* aptr, int32_t n_meshes, const double* verts, int32_t n_rows, int64_t n_out_rows,
                          int64_t* out_faces, int64_t* source, double* out_verts, void* stream) {
    if (n_faces < 0 || n_faces > (0x7fffffff - 256) / 3 || !rows_ok(n_rows) || n_meshes < 0 || !rows_ok(n_out_rows)) return MORIG_E_INVALID;
    if (n_out_rows < n_rows || n_out_rows - n_rows > 3LL * n_faces || !rows_ok(3LL * n_faces + n_rows)) return MORIG_E_INVALID;
    if (n_meshes == 0 || (n_faces == 0 && n_rows == 0)) return MORIG_OK;
    if (!fptr || !vptr || !aptr || (n_faces > 0 && (!lab || !tri || !first || !rank || !out_faces || n_rows == 0)) ||
        (n_rows > 0 && (!verts || !source || !out_verts)))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n_nodes = 3LL * n_faces;
    ProfScope ps(K_MESHSPLIT_APPLY, s, 0.0, 32.0 * (double)n_nodes + 56.0 * (double)n_out_rows);
    ms_apply_kernel<<<cdiv(n_nodes + n_rows, 256), 256, 0, s>>>(lab, tri, first, (const long long*)rank, fptr, vptr, (const long long*)aptr,
                                                                (const long long*)verts, n_nodes, n_faces, n_rows, n_meshes, n_out_rows,
                                                                (long long*)out_faces, (long long*)source, (long long*)out_verts);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
