// The tolerance weld (morig_amd/meshprep.py diagnose / clean / repair with weld_tol) for a ragged batch: the nodes
// -- the finite representatives of the exact weld -- within a tolerance of each other are linked, the links go through the component
// rounds of meshcheck.hip, and the classes leave with their lowest row as representative. The module's idiom is meshcheck.hip's: a
// kernel emits 64-bit keys, the caller sorts them (torch.sort), a kernel reads the sorted runs. Integers or float64 in the written
// order (contraction off); the only atomics are integer minima and maxima, whose result does not depend on order: two runs give the
// same bits, a mesh alone gives the bits it gives inside a batch. Nothing depends on one workgroup seeing another's store inside a
// launch. The links are DEFINED by the test over all pairs of nodes; the grid only finds them (proxweld_core.h has the argument).
//
// cell keys     three launches: the box of the finite rows of every mesh (integer min / max on the order-preserving coordinate keys,
//               reduced over the workgroup or the wave first where that lies in one mesh), the frame of every mesh (its low corner and cell side),
//               then one thread per row: the packed cell of a node, INT64_MAX for every other row.
// count links   one thread per position of the rows sorted by (mesh, cell key): the walk over the nine key ranges of the 3 x 3 x 3
//               neighbourhood -- the three z-neighbours of a cell row are one contiguous key range, found by binary search inside the
//               positions of the mesh -- counting the partners with a higher row inside the tolerance. A divergent, latency-bound
//               gather; one thread per node because a cell holds one or two nodes where the tolerance is far below the edge length.
// emit links    the same walk; every node writes its links at its prefix in visiting order as the edge keys that
//               morig_meshcheck_cc_round reads.
// spread        one thread per row: the squared distance to its final representative; the integer maximum of the bit patterns per mesh.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the core header: its functions are compiled under it too

#include "proxweld_core.h"

namespace morig {

namespace {

using namespace morig_topo;
using namespace morig_prox;

constexpr long long BOX_EMPTY_LO = 0x7fffffffffffffffLL, BOX_EMPTY_HI = -0x7fffffffffffffffLL - 1;

__global__ void __launch_bounds__(256) pw_box_init_kernel(long long* __restrict__ box, int n_meshes) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_meshes * 6) box[t] = (t % 6) < 3 ? BOX_EMPTY_LO : BOX_EMPTY_HI;
}

__global__ void __launch_bounds__(256) pw_box_kernel(const double* __restrict__ verts, const int* __restrict__ nonfinite, int n_rows,
                                                     const int* __restrict__ vptr, int n_meshes, long long* __restrict__ box) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    const bool live = v < n_rows;
    int b = -1;
    long long lo[3] = {BOX_EMPTY_LO, BOX_EMPTY_LO, BOX_EMPTY_LO}, hi[3] = {BOX_EMPTY_HI, BOX_EMPTY_HI, BOX_EMPTY_HI};
    bool has = false;
    if (live) {
        b = segment_of(vptr, n_meshes, v);
        if (!nonfinite[v]) {
            has = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) lo[c] = hi[c] = coord_key(verts[(size_t)v * 3 + c]);
        }
    }
    // one set of atomics per workgroup where all its live rows lie in one mesh (the four waves meet in LDS), else one per wave where
    // the wave lies in one mesh, else one per finite row
    int bl = live ? b : 0x7fffffff, bh = b;
    long long wlo[3] = {lo[0], lo[1], lo[2]}, whi[3] = {hi[0], hi[1], hi[2]};
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) {
        const int ol = __shfl_xor(bl, h), oh = __shfl_xor(bh, h);
        bl = ol < bl ? ol : bl;
        bh = oh > bh ? oh : bh;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long a = __shfl_xor(wlo[c], h), z = __shfl_xor(whi[c], h);
            wlo[c] = a < wlo[c] ? a : wlo[c];
            whi[c] = z > whi[c] ? z : whi[c];
        }
    }
    __shared__ long long part[4][6];
    __shared__ int span[4][2];
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { part[wave][c] = wlo[c]; part[wave][3 + c] = whi[c]; }
        span[wave][0] = bl;
        span[wave][1] = bh;
    }
    __syncthreads();
    int gl = span[0][0], gh = span[0][1];                                               // a wave without a live row changes neither
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        gl = span[w][0] < gl ? span[w][0] : gl;
        gh = span[w][1] > gh ? span[w][1] : gh;
    }
    if (gl == gh) {
        if (threadIdx.x < 6 && gh >= 0) {                                               // thread c folds column c of the four waves
            const int c = (int)threadIdx.x;
            long long x = part[0][c];
#pragma unroll
            for (int w = 1; w < 4; ++w) x = c < 3 ? (part[w][c] < x ? part[w][c] : x) : (part[w][c] > x ? part[w][c] : x);
            if (c < 3) { if (x != BOX_EMPTY_LO) atomicMin(box + (size_t)gh * 6 + c, x); }
            else if (x != BOX_EMPTY_HI) atomicMax(box + (size_t)gh * 6 + c, x);
        }
    } else if (bl == bh) {
        if ((threadIdx.x & 63) == 0 && bh >= 0 && wlo[0] != BOX_EMPTY_LO)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                atomicMin(box + (size_t)bh * 6 + c, wlo[c]);
                atomicMax(box + (size_t)bh * 6 + 3 + c, whi[c]);
            }
    } else if (has) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(box + (size_t)b * 6 + c, lo[c]);
            atomicMax(box + (size_t)b * 6 + 3 + c, hi[c]);
        }
    }
}

// frame [n_meshes][4]: the low corner and the cell side; a mesh without a finite row: (0, 0, 0, 1)
__global__ void __launch_bounds__(256) pw_frame_kernel(const long long* __restrict__ box, const double* __restrict__ eps, int n_meshes,
                                                       double* __restrict__ frame) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_meshes) return;
    double lo[3] = {0.0, 0.0, 0.0}, extent = 0.0;
    if (box[(size_t)b * 6] != BOX_EMPTY_LO) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = key_coord(box[(size_t)b * 6 + c]);
            const double e = key_coord(box[(size_t)b * 6 + 3 + c]) - lo[c];
            extent = e > extent ? e : extent;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) frame[(size_t)b * 4 + c] = lo[c];
    frame[(size_t)b * 4 + 3] = cell_side(eps[b], extent);
}

__global__ void __launch_bounds__(256) pw_cell_keys_kernel(const double* __restrict__ verts, const int* __restrict__ nonfinite,
                                                           const int* __restrict__ rep, int n_rows, const int* __restrict__ vptr, int n_meshes,
                                                           const double* __restrict__ frame, long long* __restrict__ keys) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    long long key = KEY_NONE;
    if (!nonfinite[v] && rep[v] == v) {
        const int b = segment_of(vptr, n_meshes, v);
        const double h = frame[(size_t)b * 4 + 3];
        long long cell[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) cell[c] = cell_coord(verts[(size_t)v * 3 + c], frame[(size_t)b * 4 + c], h);
        key = cell_key(cell[0], cell[1], cell[2]);
    }
    keys[v] = key;
}

// the positions [lo, hi) of the mesh of sorted position i, inside [0, n_rows)
__device__ __forceinline__ int mesh_range(const int* __restrict__ vptr, int n_meshes, int n_rows, int i, long long& lo, long long& hi) {
    const int b = segment_of(vptr, n_meshes, i);
    lo = vptr[b];
    hi = vptr[b + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_rows ? n_rows : hi;
    return b;
}

__global__ void __launch_bounds__(256) pw_count_links_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                             const double* __restrict__ pos, int n_rows, const int* __restrict__ vptr,
                                                             int n_meshes, const double* __restrict__ eps2, int* __restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    long long lo, hi;
    const int b = mesh_range(vptr, n_meshes, n_rows, i, lo, hi);
    int n = 0;
    if (i >= lo && i < hi) walk_links(keys, order, pos, n_rows, i, lo, hi, eps2[b], [&](long long) { ++n; });
    count[i] = n;
}

// lrank: the inclusive prefix sum of count
__global__ void __launch_bounds__(256) pw_emit_links_kernel(const long long* __restrict__ keys, const long long* __restrict__ order,
                                                            const double* __restrict__ pos, int n_rows, const int* __restrict__ vptr,
                                                            int n_meshes, const double* __restrict__ eps2, const int* __restrict__ count,
                                                            const long long* __restrict__ lrank, long long n_links,
                                                            long long* __restrict__ links) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int mine = count[i];
    if (mine <= 0) return;
    long long lo, hi;
    const int b = mesh_range(vptr, n_meshes, n_rows, i, lo, hi);
    if (i < lo || i >= hi) return;
    const long long row = order[i], at = lrank[i] - mine;
    int n = 0;
    walk_links(keys, order, pos, n_rows, i, lo, hi, eps2[b], [&](long long other) {
        if (n < mine && at >= 0 && at + n < n_links) links[at + n] = edge_key(row, other);
        ++n;
    });
}

__global__ void __launch_bounds__(256) pw_spread_kernel(const double* __restrict__ verts, const int* __restrict__ rep,
                                                        const int* __restrict__ nonfinite, int n_rows, const int* __restrict__ vptr,
                                                        int n_meshes, long long* __restrict__ maxbits) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    const bool live = v < n_rows;
    int b = -1;
    long long top = -1;
    if (live) {
        b = segment_of(vptr, n_meshes, v);
        const int r = rep[v];
        if (r >= 0 && r < n_rows && r != v && !nonfinite[v] && !nonfinite[r])
            top = morig_split::len2_image(morig_split::len2(verts + (size_t)v * 3, verts + (size_t)r * 3));
    }
    // one atomic per wave where all its live rows lie in one mesh, else one per row
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

inline bool rows_ok(long long n) { return n >= 0 && n <= 0x7fffffffLL - 256; }

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_proxweld_cell_keys(const double* verts, const int32_t* nonfinite, const int32_t* rep, int32_t n_rows, const int32_t* vptr,
                             int32_t n_meshes, const double* eps, int64_t* box, double* frame, int64_t* keys, void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0 || n_meshes > (0x7fffffff - 256) / 6) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!vptr || !eps || !box || !frame || (n_rows > 0 && (!verts || !nonfinite || !rep || !keys))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_PROXWELD_KEYS, s, 0.0, 64.0 * (double)n_rows + 88.0 * (double)n_meshes);
    pw_box_init_kernel<<<cdiv(n_meshes * 6, 256), 256, 0, s>>>((long long*)box, n_meshes);
    MORIG_LAUNCH_CHECK();
    if (n_rows > 0) {
        pw_box_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, nonfinite, n_rows, vptr, n_meshes, (long long*)box);
        MORIG_LAUNCH_CHECK();
    }
    pw_frame_kernel<<<cdiv(n_meshes, 256), 256, 0, s>>>((const long long*)box, eps, n_meshes, frame);
    MORIG_LAUNCH_CHECK();
    if (n_rows > 0) {
        pw_cell_keys_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, nonfinite, rep, n_rows, vptr, n_meshes, frame, (long long*)keys);
        MORIG_LAUNCH_CHECK();
    }
    return MORIG_OK;
}

int morig_proxweld_count_links(const int64_t* keys, const int64_t* order, const double* pos, int32_t n_rows, const int32_t* vptr,
                               int32_t n_meshes, const double* eps2, int32_t* count, void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0) return MORIG_OK;
    if (!keys || !order || !pos || !vptr || !eps2 || !count) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_PROXWELD_LINKS, s, 0.0, 44.0 * (double)n_rows);
    pw_count_links_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>((const long long*)keys, (const long long*)order, pos, n_rows, vptr, n_meshes, eps2, count);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_proxweld_emit_links(const int64_t* keys, const int64_t* order, const double* pos, int32_t n_rows, const int32_t* vptr,
                              int32_t n_meshes, const double* eps2, const int32_t* count, const int64_t* lrank, int64_t n_links,
                              int64_t* links, void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0 || !rows_ok(n_links)) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0 || n_links == 0) return MORIG_OK;
    if (!keys || !order || !pos || !vptr || !eps2 || !count || !lrank || !links) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_PROXWELD_LINKS, s, 0.0, 56.0 * (double)n_rows + 8.0 * (double)n_links);
    MORIG_HIP_TRY(hipMemsetAsync(links, 0xff, (size_t)n_links * sizeof(int64_t), s));      // -1: a key the component round skips
    pw_emit_links_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>((const long long*)keys, (const long long*)order, pos, n_rows, vptr, n_meshes, eps2, count,
                                                           (const long long*)lrank, n_links, (long long*)links);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_proxweld_spread(const double* verts, const int32_t* rep, const int32_t* nonfinite, int32_t n_rows, const int32_t* vptr,
                          int32_t n_meshes, int64_t* maxbits, void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!vptr || !maxbits || (n_rows > 0 && (!verts || !rep || !nonfinite))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(maxbits, 0, (size_t)n_meshes * sizeof(int64_t), s));
    if (n_rows == 0) return MORIG_OK;
    ProfScope ps(K_PROXWELD_SPREAD, s, 8.0 * (double)n_rows, 56.0 * (double)n_rows);
    pw_spread_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, rep, nonfinite, n_rows, vptr, n_meshes, (long long*)maxbits);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
