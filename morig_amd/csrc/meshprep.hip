// The mesh front end (morig_amd/meshprep.py): from (vertices, faces) of a ragged batch of meshes to what the other
// stages take -- normalised vertices, the 1-ring edges, surface samples with normals, and the solid voxel grid. Everything is float64 in
// the written order of operations (contraction off) or integer; the only atomics are integer atomicOr on bitsets, whose result does not
// depend on order: two runs give the same bits, and a mesh alone gives the bits it gives inside a batch.
//
// bbox       one workgroup per mesh: minimum and maximum per axis (exact in any order).
// affine     one thread per vertex: (v - t) * s, the reference's normalize, or (v - t) / s * dims, the grid coordinate of the voxeliser.
// edge keys  one thread per face: its six directed pairs as 64-bit keys (vertex << 32 | neighbour, rows of the batch); a pair of equal
//            indices or an index outside its mesh becomes the sentinel that sorts last. The caller sorts; edge_flags marks the first
//            key of every run, edge_compact scatters the marked keys to their rank as rows local to the mesh.
// surface    one wave per triangle, lanes striding over the voxels of its clamped bounding box, the 13-axis test of tribox_core.h per
//            voxel, atomicOr into the mesh's bitset: rows along z of 3 words.
// fill       one workgroup of 1024 threads per mesh. `reached` (the same row layout) lives in LDS, seeded from the six grid faces; a thread
//            owns rows (x, y) and sweeps them in place: row |= rows at x - 1, x + 1, y - 1, y + 1, then its closure along z through
//            non-surface bits (an occluded fill by doubling, carries between the three words included), all & ~surface. Bits only get set
//            and the fixed point -- the voxels reachable from outside -- is unique, so any interleaving ends on the same grid. Every
//            sweep but the last sets a bit, so dims^3 sweeps bound the loop; past it the status word is set and the kernel ends.
// area cdf   one wave per mesh: triangle areas, summed in ascending face order (lane after lane by shuffles: numpy's cumsum).
// samples    one thread per candidate: inverse CDF (the first face whose cumulative area exceeds u0 * total), barycentrics
//            (1 - sqrt u, sqrt u (1 - v), sqrt u v), the point and the unit normal of its triangle.
#include "common.h"
#include "tribox_core.h"

#pragma clang fp contract(off)

namespace morig {

namespace {

constexpr int FILL_THREADS = 1024;
constexpr int ROW_WORDS = MORIG_VOXEL_ROW_WORDS;
constexpr long long EDGE_SENTINEL = 0x7fffffffffffffffLL;

// ------------------------------------------------------------------------------------------------------------------------ bbox, affine
__global__ void __launch_bounds__(256) bbox_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, double* __restrict__ bbox) {
    const int b = blockIdx.x, v0 = vptr[b], v1 = vptr[b + 1];
    __shared__ double lo[3][256], hi[3][256];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = v0 + (int)threadIdx.x; v < v1; v += 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = verts[(size_t)v * 3 + c];
            mn[c] = x < mn[c] ? x : mn[c];
            mx[c] = x > mx[c] ? x : mx[c];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c][threadIdx.x] = mn[c]; hi[c][threadIdx.x] = mx[c]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double a = lo[c][threadIdx.x + s], z = hi[c][threadIdx.x + s];
                if (a < lo[c][threadIdx.x]) lo[c][threadIdx.x] = a;
                if (z > hi[c][threadIdx.x]) hi[c][threadIdx.x] = z;
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) { bbox[(size_t)b * 6 + threadIdx.x] = lo[threadIdx.x][0]; bbox[(size_t)b * 6 + 3 + threadIdx.x] = hi[threadIdx.x][0]; }
}

__global__ void __launch_bounds__(256) affine_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ vptr, int n_meshes,
                                                     const double* __restrict__ frame, int mode, double mul, double* __restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int b = segment_of(vptr, n_meshes, v);
    const double s = frame[(size_t)b * 4 + 3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double d = verts[(size_t)v * 3 + c] - frame[(size_t)b * 4 + c];
        out[(size_t)v * 3 + c] = mode == MORIG_MESH_NORMALIZE ? d * s : d / s * mul;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ 1-ring edges
__global__ void __launch_bounds__(256) edge_keys_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                        const int* __restrict__ vptr, int n_meshes, long long* __restrict__ keys) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    const long long v0 = vptr[b], nv = vptr[b + 1] - vptr[b];
    long long id[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = faces[(size_t)f * 3 + c];
    int slot = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (i == j) continue;
            const bool ok = id[i] != id[j] && id[i] >= 0 && id[i] < nv && id[j] >= 0 && id[j] < nv;
            keys[(size_t)f * 6 + slot] = ok ? (((v0 + id[i]) << 32) | (v0 + id[j])) : EDGE_SENTINEL;
            ++slot;
        }
}

__global__ void __launch_bounds__(256) edge_flags_kernel(const long long* __restrict__ keys, long long n, int* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long k = keys[i];
    flags[i] = (k != EDGE_SENTINEL && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// rank: the inclusive prefix sum of flags
__global__ void __launch_bounds__(256) edge_compact_kernel(const long long* __restrict__ keys, const int* __restrict__ flags,
                                                           const long long* __restrict__ rank, long long n, const int* __restrict__ vptr,
                                                           int n_meshes, long long n_edges, long long* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    const long long at = rank[i] - 1;
    if (at < 0 || at >= n_edges) return;
    const long long v = keys[i] >> 32, w = keys[i] & 0xffffffffLL;
    const long long v0 = vptr[segment_of(vptr, n_meshes, v)];
    out[at] = v - v0;
    out[n_edges + at] = w - v0;
}

// ------------------------------------------------------------------------------------------------------------------------ surface
__global__ void __launch_bounds__(256) voxel_surface_kernel(const double* __restrict__ grid, const int* __restrict__ faces, int n_faces,
                                                            const int* __restrict__ fptr, const int* __restrict__ vptr, int n_meshes, int dims,
                                                            unsigned* __restrict__ surface) {
    const int f = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    const int v0 = vptr[b], nv = vptr[b + 1] - v0;
    int id[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) id[c] = faces[(size_t)f * 3 + c];
    if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= nv || id[1] >= nv || id[2] >= nv) return;        // never followed
    morig_tribox::Tri t;
    morig_tribox::prepare(grid + (size_t)(v0 + id[0]) * 3, grid + (size_t)(v0 + id[1]) * 3, grid + (size_t)(v0 + id[2]) * 3, t);
    // the closed cube [i, i + 1] meets [mn, mx] for ceil(mn) - 1 <= i <= floor(mx); a coordinate that is no number ends the wave here
    int lo[3], ext[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double mn = fmin(fmin(t.v[0][c], t.v[1][c]), t.v[2][c]), mx = fmax(fmax(t.v[0][c], t.v[1][c]), t.v[2][c]);
        if (!(mn - mn == 0.0) || !(mx - mx == 0.0)) return;                        // inf or nan in any vertex
        const double a = fmax(ceil(mn) - 1.0, 0.0), z = fmin(floor(mx), (double)(dims - 1));
        if (!(a <= z)) return;
        lo[c] = (int)a;
        ext[c] = (int)z - lo[c] + 1;
    }
    const long long count = (long long)ext[0] * ext[1] * ext[2];
    unsigned* rows = surface + (size_t)b * dims * dims * ROW_WORDS;
    for (long long q = lane; q < count; q += 64) {
        const int k = lo[2] + (int)(q % ext[2]);
        const long long r = q / ext[2];
        const int j = lo[1] + (int)(r % ext[1]), i = lo[0] + (int)(r / ext[1]);
        if (morig_tribox::overlaps(t, i, j, k)) atomicOr(rows + ((size_t)i * dims + j) * ROW_WORDS + (k >> 5), 1u << (k & 31));
    }
}

// ------------------------------------------------------------------------------------------------------------------------ fill
struct Row { unsigned w[ROW_WORDS]; };

__device__ __forceinline__ Row row_or(Row a, Row b) { for (int i = 0; i < ROW_WORDS; ++i) a.w[i] |= b.w[i]; return a; }
__device__ __forceinline__ Row row_and(Row a, Row b) { for (int i = 0; i < ROW_WORDS; ++i) a.w[i] &= b.w[i]; return a; }
template <int K> __device__ __forceinline__ Row row_up(Row a) {                       // towards higher z
    constexpr int q = K / 32, r = K % 32;
    Row o;
#pragma unroll
    for (int i = 0; i < ROW_WORDS; ++i) {
        const unsigned x = i - q >= 0 ? a.w[i - q >= 0 ? i - q : 0] : 0u, y = i - q - 1 >= 0 ? a.w[i - q - 1 >= 0 ? i - q - 1 : 0] : 0u;
        o.w[i] = r ? ((x << r) | (y >> ((32 - r) & 31))) : x;
    }
    return o;
}
template <int K> __device__ __forceinline__ Row row_down(Row a) {                     // towards lower z
    constexpr int q = K / 32, r = K % 32;
    Row o;
#pragma unroll
    for (int i = 0; i < ROW_WORDS; ++i) {
        const unsigned x = i + q < ROW_WORDS ? a.w[i + q < ROW_WORDS ? i + q : 0] : 0u;
        const unsigned y = i + q + 1 < ROW_WORDS ? a.w[i + q + 1 < ROW_WORDS ? i + q + 1 : 0] : 0u;
        o.w[i] = r ? ((x >> r) | (y << ((32 - r) & 31))) : x;
    }
    return o;
}
// every free bit connected to a bit of g through free bits (g is a subset of free): the occluded fill by doubling, both directions
template <int K> __device__ __forceinline__ void fill_step(Row& up, Row& pu, Row& dn, Row& pd) {
    up = row_or(up, row_and(pu, row_up<K>(up)));
    pu = row_and(pu, row_up<K>(pu));
    dn = row_or(dn, row_and(pd, row_down<K>(dn)));
    pd = row_and(pd, row_down<K>(pd));
}
__device__ __forceinline__ Row z_closure(Row g, Row free) {
    Row up = g, pu = free, dn = g, pd = free;
    fill_step<1>(up, pu, dn, pd);
    fill_step<2>(up, pu, dn, pd);
    fill_step<4>(up, pu, dn, pd);
    fill_step<8>(up, pu, dn, pd);
    fill_step<16>(up, pu, dn, pd);
    fill_step<32>(up, pu, dn, pd);
    fill_step<64>(up, pu, dn, pd);
    return row_or(up, dn);
}

__device__ __forceinline__ Row load_row(const unsigned* p) { Row r; for (int i = 0; i < ROW_WORDS; ++i) r.w[i] = p[i]; return r; }

__global__ void __launch_bounds__(FILL_THREADS) voxel_fill_kernel(const unsigned* __restrict__ surface, int dims, unsigned char* __restrict__ solid,
                                                                   int* __restrict__ info) {
    extern __shared__ unsigned reached[];                                             // [dims * dims][ROW_WORDS]
    const int b = blockIdx.x, n_rows = dims * dims;
    const unsigned* surf = surface + (size_t)b * n_rows * ROW_WORDS;
    Row valid;                                                                         // bits 0 .. dims - 1
#pragma unroll
    for (int i = 0; i < ROW_WORDS; ++i) {
        const int left = dims - 32 * i;
        valid.w[i] = left >= 32 ? 0xffffffffu : (left > 0 ? ((1u << left) - 1u) : 0u);
    }
    Row ends;                                                                          // bits 0 and dims - 1
#pragma unroll
    for (int i = 0; i < ROW_WORDS; ++i) ends.w[i] = (i == 0 ? 1u : 0u) | (((dims - 1) >> 5) == i ? (1u << ((dims - 1) & 31)) : 0u);
    for (int row = threadIdx.x; row < n_rows; row += FILL_THREADS) {
        const int x = row / dims, y = row - x * dims;
        const bool face = x == 0 || y == 0 || x == dims - 1 || y == dims - 1;
        const Row s = load_row(surf + (size_t)row * ROW_WORDS);
#pragma unroll
        for (int i = 0; i < ROW_WORDS; ++i) reached[row * ROW_WORDS + i] = (face ? valid.w[i] : ends.w[i]) & ~s.w[i];
    }
    __syncthreads();
    const long long bound = (long long)dims * dims * dims;
    long long sweeps = 0;
    int status = MORIG_VOXEL_OK;
    for (;;) {
        int changed = 0;
        for (int row = threadIdx.x; row < n_rows; row += FILL_THREADS) {
            const int x = row / dims, y = row - x * dims;
            const Row s = load_row(surf + (size_t)row * ROW_WORDS);
            Row free;
#pragma unroll
            for (int i = 0; i < ROW_WORDS; ++i) free.w[i] = valid.w[i] & ~s.w[i];
            const Row own = load_row(reached + row * ROW_WORDS);
            Row g = own;
            if (x > 0) g = row_or(g, load_row(reached + (row - dims) * ROW_WORDS));
            if (x < dims - 1) g = row_or(g, load_row(reached + (row + dims) * ROW_WORDS));
            if (y > 0) g = row_or(g, load_row(reached + (row - 1) * ROW_WORDS));
            if (y < dims - 1) g = row_or(g, load_row(reached + (row + 1) * ROW_WORDS));
            g = z_closure(row_and(g, free), free);
#pragma unroll
            for (int i = 0; i < ROW_WORDS; ++i)
                if (g.w[i] != own.w[i]) { reached[row * ROW_WORDS + i] = g.w[i]; changed = 1; }
        }
        ++sweeps;
        if (!__syncthreads_or(changed)) break;
        if (sweeps >= bound) { status = MORIG_VOXEL_SWEEP_BOUND; break; }               // uniform: every thread counts the same sweeps
    }
    unsigned char* out = solid + (size_t)b * n_rows * dims;
    for (int row = threadIdx.x; row < n_rows; row += FILL_THREADS)
        for (int k = 0; k < dims; ++k) out[(size_t)row * dims + k] = ((reached[row * ROW_WORDS + (k >> 5)] >> (k & 31)) & 1u) ? 0 : 1;
    if (threadIdx.x == 0) { info[b * 2] = status; info[b * 2 + 1] = (int)(sweeps > 0x7fffffffLL ? 0x7fffffffLL : sweeps); }
}

// ------------------------------------------------------------------------------------------------------------------------ sampling
__device__ __forceinline__ void tri_normal(const double* __restrict__ verts, int a, int b, int c, double* n, double& len) {
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { e1[d] = verts[(size_t)b * 3 + d] - verts[(size_t)a * 3 + d]; e2[d] = verts[(size_t)c * 3 + d] - verts[(size_t)a * 3 + d]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}

__global__ void __launch_bounds__(64) area_cdf_kernel(const double* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ fptr,
                                                      const int* __restrict__ vptr, double* __restrict__ cum) {
    const int b = blockIdx.x, lane = threadIdx.x, f0 = fptr[b], f1 = fptr[b + 1], v0 = vptr[b], nv = vptr[b + 1] - v0;
    double total = 0.0;
    for (int base = f0; base < f1; base += 64) {
        const int f = base + lane;
        double area = 0.0;
        if (f < f1) {
            const int a = faces[(size_t)f * 3], bb = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
            if (a >= 0 && bb >= 0 && c >= 0 && a < nv && bb < nv && c < nv) {
                double n[3], len;
                tri_normal(verts, v0 + a, v0 + bb, v0 + c, n, len);
                area = 0.5 * len;
            }
        }
        double mine = 0.0;
        for (int l = 0; l < 64; ++l) {                                                 // ascending face order, one addition per face
            total = total + __shfl(area, l, 64);
            if (l == lane) mine = total;
        }
        if (f < f1) cum[f] = mine;
    }
}

__global__ void __launch_bounds__(256) surface_samples_kernel(const double* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ fptr,
                                                              const int* __restrict__ vptr, int n_meshes, const double* __restrict__ cum,
                                                              const double* __restrict__ uniforms, const int* __restrict__ cptr, int n_cand,
                                                              double* __restrict__ pts, double* __restrict__ normals, int* __restrict__ tri) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_cand) return;
    const int b = segment_of(cptr, n_meshes, q);
    const int f0 = fptr[b], nf = fptr[b + 1] - f0, v0 = vptr[b], nv = vptr[b + 1] - v0;
    double p[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    int chosen = -1;
    if (nf > 0) {
        const double t = uniforms[(size_t)q * 3] * cum[f0 + nf - 1];
        int lo = 0, hi = nf;                                                           // searchsorted(side = "right"): the first face with cum > t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[f0 + mid] > t) hi = mid; else lo = mid + 1;
        }
        chosen = lo < nf ? lo : nf - 1;
        const int a = faces[(size_t)(f0 + chosen) * 3], bb = faces[(size_t)(f0 + chosen) * 3 + 1], c = faces[(size_t)(f0 + chosen) * 3 + 2];
        if (a >= 0 && bb >= 0 && c >= 0 && a < nv && bb < nv && c < nv) {
            const double su = sqrt(uniforms[(size_t)q * 3 + 1]), v = uniforms[(size_t)q * 3 + 2];
            const double w0 = 1.0 - su, w1 = su * (1.0 - v), w2 = su * v;
            double len;
            tri_normal(verts, v0 + a, v0 + bb, v0 + c, n, len);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                p[d] = (w0 * verts[(size_t)(v0 + a) * 3 + d] + w1 * verts[(size_t)(v0 + bb) * 3 + d]) + w2 * verts[(size_t)(v0 + c) * 3 + d];
                n[d] = n[d] / len;
            }
        } else {
            chosen = -1;
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { pts[(size_t)q * 3 + d] = p[d]; normals[(size_t)q * 3 + d] = n[d]; }
    tri[q] = chosen;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_mesh_bbox(const double* verts, const int32_t* vptr, int32_t n_meshes, double* bbox, void* stream) {
    if (n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!verts || !vptr || !bbox) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 0.0);
    bbox_kernel<<<n_meshes, 256, 0, s>>>(verts, vptr, bbox);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_mesh_affine(const double* verts, int32_t n_rows, const int32_t* vptr, int32_t n_meshes, const double* frame, int32_t mode, double mul,
                      double* out, void* stream) {
    if (n_rows < 0 || n_meshes < 0 || (mode != MORIG_MESH_NORMALIZE && mode != MORIG_MESH_GRID)) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!verts || !vptr || !frame || !out || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 48.0 * (double)n_rows);
    affine_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(verts, n_rows, vptr, n_meshes, frame, mode, mul, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_tpl_edge_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int64_t* keys,
                        void* stream) {
    if (n_faces < 0 || n_meshes < 0 || n_faces > (1 << 28)) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !keys || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 60.0 * (double)n_faces);
    edge_keys_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, (long long*)keys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_tpl_edge_flags(const int64_t* keys, int64_t n_keys, int32_t* flags, void* stream) {
    if (n_keys < 0 || n_keys > ((int64_t)1 << 31) - 256) return MORIG_E_INVALID;
    if (n_keys == 0) return MORIG_OK;
    if (!keys || !flags) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 12.0 * (double)n_keys);
    edge_flags_kernel<<<cdiv(n_keys, 256), 256, 0, s>>>((const long long*)keys, n_keys, flags);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_tpl_edge_compact(const int64_t* keys, const int32_t* flags, const int64_t* rank, int64_t n_keys, const int32_t* vptr, int32_t n_meshes,
                           int64_t n_edges, int64_t* out, void* stream) {
    if (n_keys < 0 || n_keys > ((int64_t)1 << 31) - 256 || n_edges < 0 || n_edges > n_keys || n_meshes < 0) return MORIG_E_INVALID;
    if (n_keys == 0 || n_edges == 0) return MORIG_OK;
    if (!keys || !flags || !rank || !vptr || !out || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 20.0 * (double)n_keys + 16.0 * (double)n_edges);
    edge_compact_kernel<<<cdiv(n_keys, 256), 256, 0, s>>>((const long long*)keys, flags, (const long long*)rank, n_keys, vptr, n_meshes, n_edges,
                                                          (long long*)out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_voxel_surface(const double* grid, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes,
                        int32_t dims, uint32_t* surface, void* stream) {
    if (n_faces < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (dims < 1 || dims > MORIG_VOXEL_MAX_DIMS) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0) return MORIG_OK;
    if (!surface || !fptr || !vptr || (n_faces > 0 && (!grid || !faces))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(surface, 0, (size_t)n_meshes * dims * dims * ROW_WORDS * sizeof(uint32_t), s));
    if (n_faces == 0) return MORIG_OK;
    ProfScope ps(K_VOXEL_SURFACE, s, 0.0, 0.0);
    voxel_surface_kernel<<<cdiv(n_faces, 4), 256, 0, s>>>(grid, faces, n_faces, fptr, vptr, n_meshes, dims, surface);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_voxel_fill(const uint32_t* surface, int32_t n_meshes, int32_t dims, uint8_t* solid, int32_t* info, void* stream) {
    if (n_meshes < 0) return MORIG_E_INVALID;
    if (dims < 1 || dims > MORIG_VOXEL_MAX_DIMS) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0) return MORIG_OK;
    if (!surface || !solid || !info) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)dims * dims * ROW_WORDS * sizeof(uint32_t);             // 110 592 bytes at dims = 96
    MORIG_HIP_TRY(hipFuncSetAttribute((const void*)voxel_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ProfScope ps(K_VOXEL_FILL, s, 0.0, 0.0);
    voxel_fill_kernel<<<n_meshes, FILL_THREADS, lds, s>>>(surface, dims, solid, info);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_tri_area_cdf(const double* verts, const int32_t* faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, double* cum,
                       void* stream) {
    if (n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!fptr || !vptr) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 0.0);
    area_cdf_kernel<<<n_meshes, 64, 0, s>>>(verts, faces, fptr, vptr, cum);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_surface_samples(const double* verts, const int32_t* faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const double* cum,
                          const double* uniforms, const int32_t* cptr, int32_t n_cand, double* pts, double* normals, int32_t* tri, void* stream) {
    if (n_meshes < 0 || n_cand < 0) return MORIG_E_INVALID;
    if (n_cand == 0) return MORIG_OK;
    if (!fptr || !vptr || !uniforms || !cptr || !pts || !normals || !tri || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESH_PREP, s, 0.0, 0.0);
    surface_samples_kernel<<<cdiv(n_cand, 256), 256, 0, s>>>(verts, faces, fptr, vptr, n_meshes, cum, uniforms, cptr, n_cand, pts, normals, tri);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
