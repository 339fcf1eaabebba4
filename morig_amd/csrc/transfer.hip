// Rig transfer between meshes of the same shape (morig_amd/transfer.py): the reference's transfer_rig_to_remesh
// (data_proc/common_ops.py:229-259) for a ragged batch, and the closest-surface-point blend of skin rows. Everything is float64 in the
// written order of operations (contraction off) or integer; the only atomics are integer ORs and ADDs into the status words: two runs
// give the same bits, and a mesh alone gives the bits it gives inside a batch.
//
// keys        one thread per face: the directed (vertex, neighbour) pairs of the flood as 64-bit keys ((row of v) << 32 | n), 6 per face
//             ("faces") or 15 ("reference": for the corner position c at which v stands, the three vertices of face NUMBER c as well, the
//             reference's indexing quirk); a pair with v == n, an index outside the mesh or a face number outside it is INT64_MAX. The host
//             sorts the keys; duplicates stay (a duplicate never wins a strict `<` and never lowers a fill time).
// coincide    one thread per remeshed vertex; the original vertices of its mesh pass through LDS in tiles of 256. Per vertex the lowest
//             original vertex at squared distance 0 (-1: none) and the lowest one at the smallest squared distance (-1: no original).
// flood       one workgroup per mesh. Fill times T (0: coincident) in LDS, relaxed in place to the fixed point of
//             T[v] = min over neighbours u of T[u] + (T[u] == 0 or u > v ? 1 : 0): a shortest path with weights 0 / 1, so any order of
//             relaxation ends in the same T. The parent of v is its closest neighbour among those filled when the loop visits v --
//             T[u] == 0, T[u] < T[v], or T[u] == T[v] and u < v -- under a strict `<` on the correctly rounded root in ascending neighbour
//             order from 1e8; pointer jumping in place then carries every vertex to its coincident ancestor.
// rows        one thread per destination vertex: the gathered row (remesh) or (b0 S[f0] + b1 S[f1]) + b2 S[f2] (blend) per joint, the
//             row sum in ascending joint order, then row / (sum + 1e-8).
// closest     one thread per destination vertex; the source triangles pass through LDS in tiles of 256 faces, nine doubles each, every
//             thread reads the same triangle at the same time (a broadcast, no bank conflict); pointtri_core.h per pair.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the rule header: the pragma holds from here on

#include "pointtri_core.h"

namespace morig {

namespace {

constexpr int TILE = MORIG_TRANSFER_BLOCK;     // vertices per workgroup, original vertices / faces per LDS tile
constexpr int FLOOD_THREADS = 1024;
constexpr int MAX_FLOOD = MORIG_TRANSFER_MAX_FLOOD;
constexpr unsigned short T_INF = 0xffff;
constexpr long long NO_KEY = 0x7fffffffffffffffLL;
constexpr double COORD_LIMIT = 1e7;

__device__ __forceinline__ bool coord_ok(double x) { return x >= -COORD_LIMIT && x <= COORD_LIMIT; }       // false for NaN and the infinities

// ------------------------------------------------------------------------------------------------------------------------ keys
__global__ void __launch_bounds__(256) transfer_keys_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                            const int* __restrict__ vptr, int n_meshes, int per_face,
                                                            long long* __restrict__ keys, int* __restrict__ status) {
    const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (f >= n_faces) return;
    const int b = segment_of(fptr, n_meshes, f);
    const int f0 = fptr[b], nf = fptr[b + 1] - f0, v0 = vptr[b], nv = vptr[b + 1] - v0;
    long long* out = keys + (size_t)f * per_face;
    int id[3];
    bool bad = !(f0 <= f && f < f0 + nf);
#pragma unroll
    for (int k = 0; k < 3; ++k) { id[k] = faces[(size_t)f * 3 + k]; bad = bad || id[k] < 0 || id[k] >= nv; }
    if (bad) {
        for (int k = 0; k < per_face; ++k) out[k] = NO_KEY;
        atomicOr(status, MORIG_TRANSFER_BAD_FACE);
        return;
    }
    int at = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 1; j < 3; ++j) {
            const int n = id[(k + j) % 3];
            out[at++] = n != id[k] ? ((long long)(v0 + id[k]) << 32) | (long long)n : NO_KEY;
        }
    if (per_face == 15)
#pragma unroll
        for (int c = 0; c < 3; ++c)                                                     // v = id[c] stands at corner position c: face number c too
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                long long key = NO_KEY;
                if (c < nf) {
                    const int n = faces[((size_t)f0 + c) * 3 + j];
                    if (n >= 0 && n < nv && n != id[c]) key = ((long long)(v0 + id[c]) << 32) | (long long)n;
                }
                out[at++] = key;
            }
}

// ------------------------------------------------------------------------------------------------------------------------ coincide
__global__ void __launch_bounds__(TILE) transfer_coincide_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ blk_ptr,
                                                                 int n_meshes, const double* __restrict__ ori, const int* __restrict__ optr,
                                                                 int* __restrict__ coin, int* __restrict__ near, int* __restrict__ status) {
    __shared__ double s_o[TILE][3];
    const BlockRow at = block_row(blk_ptr, n_meshes, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const int b = at.seg, v0 = vptr[b], nv = vptr[b + 1] - v0, o0 = optr[b], no = optr[b + 1] - o0;
    const long long lv = at.row;
    const bool live = lv >= 0 && lv < nv;
    double p[3] = {0.0, 0.0, 0.0};
    bool bad = false;
    if (live)
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = verts[((size_t)v0 + lv) * 3 + c]; bad = bad || !coord_ok(p[c]); }
    int first = -1, best = -1;
    double bd = INFINITY;
    for (int base = 0; base < no; base += TILE) {
        __syncthreads();
        const int i = base + (int)threadIdx.x;
        if (i < no)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x = ori[((size_t)o0 + i) * 3 + c];
                s_o[threadIdx.x][c] = x;
                bad = bad || (lv == (long long)threadIdx.x && !coord_ok(x));            // the first workgroup of the mesh checks its originals
            }
        __syncthreads();
        const int m = min(TILE, no - base);
        if (live)
            for (int k = 0; k < m; ++k) {
                const double d = morig_pointtri::dist2(p, s_o[k]);
                if (d < bd) { bd = d; best = base + k; }                                // strict: the lowest index among equals
                if (d == 0.0 && first < 0) first = base + k;
            }
    }
    if (bad) atomicOr(status, MORIG_TRANSFER_BAD_COORD);
    if (live) { coin[(size_t)v0 + lv] = first; near[(size_t)v0 + lv] = best; }
}

// the originals of a mesh without remeshed vertices are in no workgroup above: their coordinates are never read, so nothing checks them

// ------------------------------------------------------------------------------------------------------------------------ flood
__global__ void __launch_bounds__(FLOOD_THREADS) transfer_flood_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ rowptr,
                                                                       const long long* __restrict__ keys, const int* __restrict__ coin,
                                                                       const int* __restrict__ near, int nearest, int* __restrict__ source,
                                                                       int* __restrict__ sweep, int* __restrict__ status) {
    __shared__ unsigned short s_T[MAX_FLOOD];
    __shared__ int s_p[MAX_FLOOD];
    const int b = blockIdx.x;
    const int v0 = vptr[b];
    const int nv = min(vptr[b + 1] - v0, MAX_FLOOD);                                   // the entry point refuses more before the launch
    const int tid = threadIdx.x;
    for (int v = tid; v < nv; v += FLOOD_THREADS) s_T[v] = coin[(size_t)v0 + v] >= 0 ? 0 : T_INF;
    __syncthreads();
    int changed;
    do {                                                                                // label-correcting relaxation, in place
        changed = 0;
        for (int v = tid; v < nv; v += FLOOD_THREADS) {
            const unsigned tv = s_T[v];
            if (tv == 0) continue;
            unsigned best = tv;
            const int e1 = rowptr[(size_t)v0 + v + 1];
            for (int e = rowptr[(size_t)v0 + v]; e < e1; ++e) {
                const int u = (int)(keys[e] & 0xffffffffLL);
                if (u < 0 || u >= nv) continue;
                const unsigned tu = s_T[u];
                if (tu == T_INF) continue;
                const unsigned cand = tu + ((tu == 0 || u > v) ? 1u : 0u);
                best = min(best, cand);
            }
            if (best < tv) { s_T[v] = (unsigned short)best; changed = 1; }
        }
    } while (__syncthreads_or(changed));
    for (int v = tid; v < nv; v += FLOOD_THREADS) {                                     // parents
        const unsigned tv = s_T[v];
        int parent = v;
        if (tv != 0 && tv != T_INF) {
            double p[3], q[3], closest = 1e8;
            int nn = -1;
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = verts[((size_t)v0 + v) * 3 + c];
            const int e1 = rowptr[(size_t)v0 + v + 1];
            for (int e = rowptr[(size_t)v0 + v]; e < e1; ++e) {
                const int u = (int)(keys[e] & 0xffffffffLL);
                if (u < 0 || u >= nv) continue;
                const unsigned tu = s_T[u];
                if (!(tu == 0 || tu < tv || (tu == tv && u < v))) continue;             // not filled when the loop visits v
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = verts[((size_t)v0 + u) * 3 + c];
                const double d = sqrt(morig_pointtri::dist2(p, q));
                if (d < closest) { closest = d; nn = u; }
            }
            if (nn >= 0) parent = nn;                                                   // always: the coordinates are bounded by 1e7
        }
        s_p[v] = parent;
    }
    __syncthreads();
    do {                                                                                // pointer jumping, in place: s_p[v] stays an ancestor of v
        changed = 0;
        for (int v = tid; v < nv; v += FLOOD_THREADS) {
            const int a = s_p[v], g = s_p[a];
            if (g != a) { s_p[v] = g; changed = 1; }
        }
    } while (__syncthreads_or(changed));
    int lost = 0;
    for (int v = tid; v < nv; v += FLOOD_THREADS) {
        const int root = s_p[v];
        const unsigned tv = s_T[v];
        int src = s_T[root] == 0 ? coin[(size_t)v0 + root] : -1;
        if (tv == T_INF && nearest) src = near[(size_t)v0 + v];
        source[(size_t)v0 + v] = src;
        sweep[(size_t)v0 + v] = tv == T_INF ? -1 : (int)tv;
        lost += src < 0 ? 1 : 0;
    }
    if (lost) atomicAdd(status + 1 + b, lost);                                          // integers: the order of the additions is free
}

// ------------------------------------------------------------------------------------------------------------------------ rows
// BLEND false: row = S[source]; true: (b0 S[f0] + b1 S[f1]) + b2 S[f2]. A vertex without a row (source or face < 0) gets zeros.
template <bool BLEND>
__global__ void __launch_bounds__(TILE) transfer_rows_kernel(const double* __restrict__ skins, const int* __restrict__ sptr, const int* __restrict__ joints,
                                                             const int* __restrict__ svptr, const int* __restrict__ faces, const int* __restrict__ fptr,
                                                             const int* __restrict__ vptr, const int* __restrict__ blk_ptr, int n_meshes,
                                                             const int* __restrict__ pick, const double* __restrict__ bary,
                                                             double* __restrict__ out, const int* __restrict__ out_ptr) {
    const BlockRow at = block_row(blk_ptr, n_meshes, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const int b = at.seg, v0 = vptr[b], nv = vptr[b + 1] - v0, J = joints[b], ns = svptr[b + 1] - svptr[b];
    const long long lv = at.row;
    if (!(lv >= 0 && lv < nv) || J <= 0) return;
    const double* S = skins + sptr[b];
    double* row = out + (size_t)out_ptr[b] + (size_t)lv * J;
    const int k = pick[(size_t)v0 + lv];
    int r[3] = {0, 0, 0};
    double w[3] = {0.0, 0.0, 0.0};
    bool have = k >= 0 && ns > 0;
    if (BLEND) {
        have = have && k < fptr[b + 1] - fptr[b];
        if (have)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r[c] = min(max(faces[((size_t)fptr[b] + k) * 3 + c], 0), ns - 1);       // as the closest-point kernel clamped it
                w[c] = bary[((size_t)v0 + lv) * 3 + c];
            }
    } else if (have) {
        r[0] = min(k, ns - 1);
    }
    if (!have) {
        for (int j = 0; j < J; ++j) row[j] = 0.0;
        return;
    }
    double sum = 0.0;
    for (int j = 0; j < J; ++j) {
        double x;
        if (BLEND) x = (w[0] * S[(size_t)r[0] * J + j] + w[1] * S[(size_t)r[1] * J + j]) + w[2] * S[(size_t)r[2] * J + j];
        else x = S[(size_t)r[0] * J + j];
        row[j] = x;
        sum += x;
    }
    const double den = sum + 1e-8;
    for (int j = 0; j < J; ++j) row[j] = row[j] / den;
}

// ------------------------------------------------------------------------------------------------------------------------ closest
__global__ void __launch_bounds__(TILE) transfer_closest_kernel(const double* __restrict__ dst, const int* __restrict__ dptr, const int* __restrict__ blk_ptr,
                                                                int n_meshes, const double* __restrict__ verts, const int* __restrict__ vptr,
                                                                const int* __restrict__ faces, const int* __restrict__ fptr, int* __restrict__ face_out,
                                                                double* __restrict__ bary_out, double* __restrict__ dist_out, int* __restrict__ status) {
    __shared__ double s_t[TILE][9];
    const BlockRow at = block_row(blk_ptr, n_meshes, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const int b = at.seg, d0 = dptr[b], nd = dptr[b + 1] - d0, v0 = vptr[b], nv = vptr[b + 1] - v0, f0 = fptr[b];
    const int nf = nv >= 1 ? fptr[b + 1] - f0 : 0;                                     // faces of a mesh without vertices name nothing
    const long long lv = at.row;
    const bool live = lv >= 0 && lv < nd;
    double p[3] = {0.0, 0.0, 0.0};
    if (live)
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = dst[((size_t)d0 + lv) * 3 + c];
    bool bad = fptr[b + 1] - f0 > 0 && nv < 1;
    int bf = -1;
    double bd = INFINITY, bb[3] = {NAN, NAN, NAN};
    for (int base = 0; base < nf; base += TILE) {
        __syncthreads();
        const int i = base + (int)threadIdx.x;
        if (i < nf)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int raw = faces[((size_t)f0 + i) * 3 + k];
                const int id = min(max(raw, 0), nv - 1);
                bad = bad || id != raw;
#pragma unroll
                for (int c = 0; c < 3; ++c) s_t[threadIdx.x][k * 3 + c] = verts[((size_t)v0 + id) * 3 + c];
            }
        __syncthreads();
        const int m = min(TILE, nf - base);
        if (live)
            for (int k = 0; k < m; ++k) {
                double q[3];
                const double* t = s_t[k];
                morig_pointtri::closest_bary(p, t, t + 3, t + 6, q);
                const double d = morig_pointtri::bary_dist2(p, t, t + 3, t + 6, q);
                if (d < bd) { bd = d; bf = base + k; bb[0] = q[0]; bb[1] = q[1]; bb[2] = q[2]; }      // strict: the lowest face among equals
            }
    }
    if (bad) atomicOr(status, MORIG_TRANSFER_BAD_FACE);
    if (live && nf == 0) atomicOr(status, MORIG_TRANSFER_NO_FACES);
    if (!live) return;
    face_out[(size_t)d0 + lv] = bf;
#pragma unroll
    for (int c = 0; c < 3; ++c) bary_out[((size_t)d0 + lv) * 3 + c] = bb[c];
    dist_out[(size_t)d0 + lv] = bf >= 0 ? sqrt(bd) : NAN;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_transfer_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int32_t per_face,
                        int64_t* keys, int32_t* status, void* stream) {
    if (n_faces < 0 || n_meshes < 0 || (per_face != 6 && per_face != 15)) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !keys || !status || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_TRANSFER_FLOOD, s, 0.0, 0.0);
    transfer_keys_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, per_face, (long long*)keys, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_transfer_coincide(const double* verts, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* ori,
                            const int32_t* optr, int32_t* coincident, int32_t* nearest, int32_t* status, void* stream) {
    if (n_meshes < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!verts || !vptr || !blk_ptr || !optr || !coincident || !nearest || !status || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_TRANSFER_PAIRS, s, 0.0, 0.0);
    transfer_coincide_kernel<<<n_blocks, TILE, 0, s>>>(verts, vptr, blk_ptr, n_meshes, ori, optr, coincident, nearest, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_transfer_flood(const double* verts, const int32_t* vptr, int32_t n_meshes, int32_t max_verts, const int32_t* rowptr, const int64_t* keys,
                         const int32_t* coincident, const int32_t* nearest, int32_t use_nearest, int32_t* source, int32_t* sweep, int32_t* status,
                         void* stream) {
    if (n_meshes < 0 || max_verts < 0) return MORIG_E_INVALID;
    if (max_verts > MORIG_TRANSFER_MAX_FLOOD) return MORIG_E_UNSUPPORTED;
    if (n_meshes == 0 || max_verts == 0) return MORIG_OK;
    if (!verts || !vptr || !rowptr || !coincident || !nearest || !source || !sweep || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_TRANSFER_FLOOD, s, 0.0, 0.0);
    transfer_flood_kernel<<<n_meshes, FLOOD_THREADS, 0, s>>>(verts, vptr, rowptr, (const long long*)keys, coincident, nearest, use_nearest ? 1 : 0,
                                                            source, sweep, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_transfer_rows(const double* skins, const int32_t* skin_ptr, const int32_t* joints, const int32_t* src_vptr, const int32_t* faces,
                        const int32_t* fptr, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const int32_t* pick,
                        const double* bary, double* out, const int32_t* out_ptr, void* stream) {
    if (n_meshes < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!skin_ptr || !joints || !src_vptr || !vptr || !blk_ptr || !pick || !out_ptr || n_meshes == 0) return MORIG_E_INVALID;
    if (bary && (!faces || !fptr)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_TRANSFER_ROWS, s, 0.0, 0.0);
    if (bary) transfer_rows_kernel<true><<<n_blocks, TILE, 0, s>>>(skins, skin_ptr, joints, src_vptr, faces, fptr, vptr, blk_ptr, n_meshes, pick, bary, out, out_ptr);
    else transfer_rows_kernel<false><<<n_blocks, TILE, 0, s>>>(skins, skin_ptr, joints, src_vptr, faces, fptr, vptr, blk_ptr, n_meshes, pick, bary, out, out_ptr);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_transfer_closest(const double* dst, const int32_t* dptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* verts,
                           const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t* face, double* bary, double* distance,
                           int32_t* status, void* stream) {
    if (n_meshes < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!dst || !dptr || !blk_ptr || !vptr || !fptr || !face || !bary || !distance || !status || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_TRANSFER_PAIRS, s, 0.0, 0.0);
    transfer_closest_kernel<<<n_blocks, TILE, 0, s>>>(dst, dptr, blk_ptr, n_meshes, verts, vptr, faces, fptr, face, bary, distance, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
