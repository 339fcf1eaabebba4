// Mesh repair (morig_amd/meshprep.py repair) for a ragged batch of CLEANED meshes: a consistent orientation per
// component, the boundary loops, and a centroid fan for every simple loop. The idiom is meshcheck.hip's: a kernel emits 64-bit keys, the
// caller sorts them (torch.sort), a kernel reads the runs. Integers or float64 in the written order (contraction off); the only atomics
// are integer ones (OR, add, min) and relaxed stores of 1, whose result does not depend on order. Nothing depends on one workgroup
// seeing another's store inside a launch.
//
// edge records   one thread per face: its corners as rows of the batch and three (undirected key, face << 1 | dir) records.
// links          one thread per sorted record. It reads at most two records on either side (orient_core.h run_shape), so a run of any
//                length, across any workgroup boundary, costs every record the same. A run of two is a link: its records emit the two
//                edges of the double cover (node 2 face + sign), in the key layout of morig_meshcheck_cc_round, which then labels the
//                2 F cover nodes unchanged. A record in any other run marks its face open; a run of one is a boundary half-edge.
// orient stats   one thread per face: root face and parity from the label of its node 2f; an open face marks its root.
// signed volume  one wave per component over its faces in ascending order: lane l adds the terms l, l + 64, ..., lane 0 folds the 64 sums
//                (topo_core.h fold_lanes); the face counts of the component and of its parity class 1 ride along as integers.
// orient apply   one thread per face: the decision of its component (orient_core.h flip_class), the face local to its mesh with corners
//                1 and 2 exchanged where it flips; the thread of a root face writes the component's report bits.
// boundary init  two launches: the directed half-edges after the flips with the degrees of their ends and nxt[from] = min to; then the
//                class, the initial label and the initial pointer of every row.
// loop round     one round of pointer doubling, from one pair of arrays into another.
// loop centroid  one wave per selected loop over its rows in ascending order, three lane sums folded as above.
// fill mark/emit which rows begin a fan face, then the fan faces at their prefix-sum ranks.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the core headers: their functions are compiled under it too

#include "orient_core.h"

namespace morig {

namespace {

using namespace morig_topo;
using namespace morig_orient;

__global__ void __launch_bounds__(256) mf_edge_records_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                              const int* __restrict__ vptr, int n_meshes, int n_rows, int* __restrict__ tri,
                                                              long long* __restrict__ keys, int* __restrict__ vals, int* __restrict__ status) {
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
        r[c] = (long long)v0 + id;
    }
    ok = ok && r[0] != r[1] && r[1] != r[2] && r[0] != r[2];
    if (!ok) atomicOr(status, MORIG_MESHCHECK_BAD_FACE);                               // never followed
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long a = r[c], d = r[(c + 1) % 3];
        tri[(size_t)f * 3 + c] = ok ? (int)a : -1;
        keys[(size_t)f * 3 + c] = ok ? record_key(a, d) : KEY_NONE;
        vals[(size_t)f * 3 + c] = ok ? record_val(f, a, d) : -1;
    }
}

__global__ void __launch_bounds__(256) mf_links_kernel(const long long* __restrict__ keys, const int* __restrict__ vals, long long n_records,
                                                       int n_faces, long long* __restrict__ cover, int* __restrict__ face_open,
                                                       int* __restrict__ bflag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records) return;
    long long ck = KEY_NONE;
    int boundary = 0;
    const long long k = keys[i];
    const int val = vals[i];
    const long long f = val >> 1;
    if (k != KEY_NONE && k >= 0 && val >= 0 && f < n_faces) {
        int count;
        ck = link_cover(keys, vals, i, n_records, n_faces, &count);
        if (count != 2) atomicOr(face_open + f, 1);
        boundary = count == 1 ? 1 : 0;
    }
    cover[i] = ck;
    bflag[i] = boundary;
}

__global__ void __launch_bounds__(256) mf_orient_stats_kernel(const int* __restrict__ lab, const int* __restrict__ face_open, int n_faces,
                                                              int* __restrict__ root, int* __restrict__ parity, long long* __restrict__ face_root,
                                                              int* __restrict__ root_open) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int l = lab[(size_t)2 * f];
    if (l < 0 || (l >> 1) > f) l = 2 * f;                                              // a label is at most its node
    const int r = l >> 1;
    root[f] = r;
    parity[f] = l & 1;
    face_root[f] = r;
    // every writer stores the same 1: a relaxed atomic STORE, not a read-modify-write (a component's faces all name one word)
    if (face_open[f]) __hip_atomic_store(root_open + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The terms of U faces of one lane, with the sign of their parity (ok = false: the face is not followed). The loads are made for all U
// faces before anything is decided on their values -- an index out of range is replaced by 0, not branched on --, so that the three
// dependent loads (order -> tri -> verts) of the U faces are in flight together; n_rows > 0 and n_faces > 0.
template <int U>
__device__ __forceinline__ void volume_terms(const double* __restrict__ verts, int n_rows, const int* __restrict__ tri, const int* __restrict__ parity,
                                             int n_faces, const long long* __restrict__ order, long long k, double* t, int* p, bool* ok) {
    long long f[U];
    int a[U], b[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        f[u] = order[k + 64 * u];
        ok[u] = f[u] >= 0 && f[u] < n_faces;
        f[u] = ok[u] ? f[u] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        a[u] = tri[(size_t)f[u] * 3];
        b[u] = tri[(size_t)f[u] * 3 + 1];
        d[u] = tri[(size_t)f[u] * 3 + 2];
        p[u] = parity[f[u]] & 1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        ok[u] = ok[u] && a[u] >= 0 && b[u] >= 0 && d[u] >= 0 && a[u] < n_rows && b[u] < n_rows && d[u] < n_rows;
        a[u] = ok[u] ? a[u] : 0;
        b[u] = ok[u] ? b[u] : 0;
        d[u] = ok[u] ? d[u] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const double x = signed_term(verts + (size_t)a[u] * 3, verts + (size_t)b[u] * 3, verts + (size_t)d[u] * 3);
        t[u] = p[u] ? -x : x;
    }
}

__global__ void __launch_bounds__(256) mf_signed_volume_kernel(const double* __restrict__ verts, int n_rows, const int* __restrict__ tri,
                                                               const int* __restrict__ parity, int n_faces, const long long* __restrict__ order,
                                                               const long long* __restrict__ kptr, const long long* __restrict__ roots,
                                                               int n_comps, double* __restrict__ vol, int* __restrict__ cnt,
                                                               int* __restrict__ cnt1) {
    __shared__ double sums[4][64];
    __shared__ int ones[4][64];
    const int wave = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    const bool live = c < n_comps;
    long long k0 = live ? kptr[c] : 0, k1 = live ? kptr[c + 1] : 0;
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > n_faces ? n_faces : k1;
    double s = 0.0;
    int n1 = 0;
    long long k = k0 + lane;
    // four faces of the lane at a time: their loads (order -> tri -> verts) do not depend on one another, only the additions do, and
    // those stay in ascending order
    for (; k + 3 * 64 < k1; k += 4 * 64) {
        double t[4];
        int p[4];
        bool ok[4];
        volume_terms<4>(verts, n_rows, tri, parity, n_faces, order, k, t, p, ok);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) { s = s + t[u]; n1 += p[u]; }
    }
    for (; k < k1; k += 64) {
        double t;
        int p;
        bool ok;
        volume_terms<1>(verts, n_rows, tri, parity, n_faces, order, k, &t, &p, &ok);
        if (ok) { s = s + t; n1 += p; }
    }
    sums[wave][lane] = s;
    ones[wave][lane] = n1;
    __syncthreads();
    if (lane == 0 && live) {
        const long long r = roots[c];
        if (r >= 0 && r < n_faces) {
            int total = 0;
            for (int l = 0; l < 64; ++l) total += ones[wave][l];
            vol[r] = fold_lanes(sums[wave]);
            cnt[r] = (int)(k1 > k0 ? k1 - k0 : 0);
            cnt1[r] = total;
        }
    }
}

__global__ void __launch_bounds__(256) mf_orient_apply_kernel(const int* __restrict__ tri, int n_faces, const int* __restrict__ fptr,
                                                              const int* __restrict__ vptr, int n_meshes, const int* __restrict__ lab,
                                                              const int* __restrict__ root, const int* __restrict__ parity,
                                                              const int* __restrict__ root_open, const double* __restrict__ vol,
                                                              const int* __restrict__ cnt, const int* __restrict__ cnt1,
                                                              long long* __restrict__ out_faces, int* __restrict__ flipped,
                                                              int* __restrict__ rootinfo) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int r = root[f];
    if (r < 0 || r >= n_faces) r = f;
    const bool nonorientable = lab[(size_t)2 * r] == lab[(size_t)2 * r + 1], open = root_open[r] != 0;
    bool by_volume;
    const int cls = flip_class(nonorientable, open, vol[r], cnt[r], cnt1[r], &by_volume);
    const int flip = (cls >= 0 && (parity[f] & 1) == cls) ? 1 : 0;
    const int v0 = vptr[segment_of(fptr, n_meshes, f)];
    const int a = tri[(size_t)f * 3], b = tri[(size_t)f * 3 + 1], d = tri[(size_t)f * 3 + 2];
    out_faces[(size_t)f * 3] = a < 0 ? -1 : a - v0;
    out_faces[(size_t)f * 3 + 1] = a < 0 ? -1 : (flip ? d : b) - v0;
    out_faces[(size_t)f * 3 + 2] = a < 0 ? -1 : (flip ? b : d) - v0;
    flipped[f] = flip;
    rootinfo[f] = r == f ? root_info(nonorientable, open, vol[r], cnt[r], cnt1[r]) : 0;
}

__global__ void __launch_bounds__(256) mf_boundary_edges_kernel(const long long* __restrict__ keys, const int* __restrict__ vals,
                                                                const int* __restrict__ bflag, long long n_records,
                                                                const int* __restrict__ flipped, int n_faces, int n_rows, int* __restrict__ hfrom,
                                                                int* __restrict__ hto, int* __restrict__ outdeg, int* __restrict__ indeg,
                                                                int* __restrict__ nxt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_records) return;
    int from = -1, to = -1;
    const long long k = keys[i];
    const int val = vals[i];
    if (bflag[i] && k != KEY_NONE && k >= 0 && val >= 0 && (val >> 1) < n_faces) {
        const long long lo = k >> 32, hi = k & 0xffffffffLL;
        if (lo < n_rows && hi < n_rows) {
            const bool forward = ((val & 1) != 0) != (flipped[val >> 1] != 0);
            from = (int)(forward ? lo : hi);
            to = (int)(forward ? hi : lo);
            atomicAdd(outdeg + from, 1);
            atomicAdd(indeg + to, 1);
            atomicMin(nxt + from, to);
        }
    }
    hfrom[i] = from;
    hto[i] = to;
}

__global__ void __launch_bounds__(256) mf_boundary_verts_kernel(const int* __restrict__ outdeg, const int* __restrict__ indeg, int n_rows,
                                                                int* __restrict__ nxt, int* __restrict__ lab, int* __restrict__ vclass) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int o = outdeg[v], n = indeg[v], to = nxt[v];
    const bool regular = o == 1 && n == 1 && to >= 0 && to < n_rows;
    vclass[v] = regular ? MORIG_MESHFIX_REGULAR : ((o != 0 || n != 0) ? MORIG_MESHFIX_TANGLED : 0);
    lab[v] = regular ? v : -1;
    if (!regular) nxt[v] = v;
}

__global__ void __launch_bounds__(256) mf_loop_round_kernel(const int* __restrict__ lab, const int* __restrict__ nxt, int n_rows,
                                                            int* __restrict__ lab2, int* __restrict__ nxt2) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    int n = nxt[v];
    if (n < 0 || n >= n_rows) n = v;
    int nn = nxt[n];
    if (nn < 0 || nn >= n_rows) nn = n;
    lab2[v] = min(lab[v], lab[n]);
    nxt2[v] = nn;
}

__global__ void __launch_bounds__(256) mf_loop_centroid_kernel(const double* __restrict__ verts, int n_rows, const long long* __restrict__ order,
                                                               const long long* __restrict__ lptr, int n_loops, const long long* __restrict__ sel,
                                                               int n_sel, double* __restrict__ centroid) {
    __shared__ double sums[4][3][64];
    const int wave = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    const long long c = q < n_sel ? sel[q] : -1;
    const bool live = c >= 0 && c < n_loops;
    long long k0 = live ? lptr[c] : 0, k1 = live ? lptr[c + 1] : 0;
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > n_rows ? n_rows : k1;
    double s[3] = {0.0, 0.0, 0.0};
    for (long long k = k0 + lane; k < k1; k += 64) {
        const long long v = order[k];
        if (v < 0 || v >= n_rows) continue;
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] = s[d] + verts[(size_t)v * 3 + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) sums[wave][d][lane] = s[d];
    __syncthreads();
    if (lane == 0 && q < n_sel) {
        const double len = (double)(k1 > k0 ? k1 - k0 : 0);
#pragma unroll
        for (int d = 0; d < 3; ++d) centroid[(size_t)q * 3 + d] = fold_lanes(sums[wave][d]) / len;
    }
}

__global__ void __launch_bounds__(256) mf_fill_mark_kernel(const int* __restrict__ vclass, const int* __restrict__ lab, const int* __restrict__ slot,
                                                           int n_rows, int* __restrict__ emit) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int l = lab[v];
    emit[v] = (vclass[v] == MORIG_MESHFIX_REGULAR && l >= 0 && l < n_rows && slot[l] >= 0) ? 1 : 0;
}

__global__ void __launch_bounds__(256) mf_fill_emit_kernel(const int* __restrict__ nxt0, const int* __restrict__ emit, const long long* __restrict__ erank,
                                                           const int* __restrict__ lab, const int* __restrict__ slot, const int* __restrict__ vptr,
                                                           const long long* __restrict__ sptr, int n_rows, int n_meshes, long long n_out,
                                                           long long* __restrict__ out_faces) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows || !emit[v]) return;
    const long long at = erank[v] - 1;
    const int l = lab[v];
    if (at < 0 || at >= n_out || l < 0 || l >= n_rows) return;
    const int b = segment_of(vptr, n_meshes, v);
    const long long v0 = vptr[b], nv = vptr[b + 1] - v0;
    out_faces[(size_t)at * 3] = (long long)nxt0[v] - v0;
    out_faces[(size_t)at * 3 + 1] = (long long)v - v0;
    out_faces[(size_t)at * 3 + 2] = nv + slot[l] - sptr[b];
}

inline bool rows_ok(long long n) { return n >= 0 && n <= 0x7fffffffLL - 256; }

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_meshfix_edge_records(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int32_t n_rows,
                               int32_t* tri, int64_t* keys, int32_t* vals, int32_t* status, void* stream) {
    if (n_faces < 0 || n_faces > (0x7fffffff - 256) / 8 || !rows_ok(n_rows) || n_meshes < 0) return MORIG_E_INVALID;   // 2 F nodes + 6 F keys per round
    if (n_meshes == 0 || n_faces == 0) return MORIG_OK;
    if (!faces || !fptr || !vptr || !tri || !keys || !vals || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_ORIENT, s, 0.0, 84.0 * (double)n_faces);
    mf_edge_records_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, vptr, n_meshes, n_rows, tri, (long long*)keys, vals, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_links(const int64_t* keys, const int32_t* vals, int64_t n_records, int32_t n_faces, int64_t* cover, int32_t* face_open,
                        int32_t* bflag, void* stream) {
    if (!rows_ok(n_records) || !rows_ok(n_faces)) return MORIG_E_INVALID;
    if (n_records == 0 && n_faces == 0) return MORIG_OK;
    if ((n_faces > 0 && !face_open) || (n_records > 0 && (!keys || !vals || !cover || !bflag || n_faces == 0))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (n_faces > 0) MORIG_HIP_TRY(hipMemsetAsync(face_open, 0, (size_t)n_faces * sizeof(int32_t), s));
    if (n_records == 0) return MORIG_OK;
    ProfScope ps(K_MESHFIX_ORIENT, s, 0.0, 32.0 * (double)n_records);
    mf_links_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)keys, vals, n_records, n_faces, (long long*)cover, face_open, bflag);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_orient_stats(const int32_t* lab, const int32_t* face_open, int32_t n_faces, int32_t* root, int32_t* parity, int64_t* face_root,
                               int32_t* root_open, void* stream) {
    if (n_faces < 0 || n_faces > (0x7fffffff - 256) / 2) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!lab || !face_open || !root || !parity || !face_root || !root_open) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(root_open, 0, (size_t)n_faces * sizeof(int32_t), s));
    ProfScope ps(K_MESHFIX_ORIENT, s, 0.0, 28.0 * (double)n_faces);
    mf_orient_stats_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(lab, face_open, n_faces, root, parity, (long long*)face_root, root_open);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_signed_volume(const double* verts, int32_t n_rows, const int32_t* tri, const int32_t* parity, int32_t n_faces,
                                const int64_t* order, const int64_t* kptr, const int64_t* roots, int32_t n_comps, double* vol, int32_t* cnt,
                                int32_t* cnt1, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_faces) || !rows_ok(n_comps) || n_comps > n_faces) return MORIG_E_INVALID;
    if (n_faces == 0) return MORIG_OK;
    if (!vol || !cnt || !cnt1 || (n_comps > 0 && (!verts || !tri || !parity || !order || !kptr || !roots || n_rows == 0))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(vol, 0, (size_t)n_faces * sizeof(double), s));
    MORIG_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)n_faces * sizeof(int32_t), s));
    MORIG_HIP_TRY(hipMemsetAsync(cnt1, 0, (size_t)n_faces * sizeof(int32_t), s));
    if (n_comps == 0) return MORIG_OK;
    ProfScope ps(K_MESHFIX_ORIENT, s, 27.0 * (double)n_faces, 96.0 * (double)n_faces);
    mf_signed_volume_kernel<<<cdiv(n_comps, 4), 256, 0, s>>>(verts, n_rows, tri, parity, n_faces, (const long long*)order, (const long long*)kptr,
                                                             (const long long*)roots, n_comps, vol, cnt, cnt1);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_orient_apply(const int32_t* tri, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* lab,
                               const int32_t* root, const int32_t* parity, const int32_t* root_open, const double* vol, const int32_t* cnt,
                               const int32_t* cnt1, int64_t* out_faces, int32_t* flipped, int32_t* rootinfo, void* stream) {
    if (n_faces < 0 || n_faces > (0x7fffffff - 256) / 2 || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_faces == 0) return MORIG_OK;
    if (!tri || !fptr || !vptr || !lab || !root || !parity || !root_open || !vol || !cnt || !cnt1 || !out_faces || !flipped || !rootinfo)
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_ORIENT, s, 0.0, 80.0 * (double)n_faces);
    mf_orient_apply_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(tri, n_faces, fptr, vptr, n_meshes, lab, root, parity, root_open, vol, cnt, cnt1,
                                                              (long long*)out_faces, flipped, rootinfo);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_boundary_init(const int64_t* keys, const int32_t* vals, const int32_t* bflag, int64_t n_records, const int32_t* flipped,
                                int32_t n_faces, int32_t n_rows, int32_t* hfrom, int32_t* hto, int32_t* outdeg, int32_t* indeg, int32_t* nxt,
                                int32_t* lab, int32_t* vclass, void* stream) {
    if (!rows_ok(n_records) || !rows_ok(n_faces) || !rows_ok(n_rows)) return MORIG_E_INVALID;
    if (n_records == 0 && n_rows == 0) return MORIG_OK;
    if ((n_rows > 0 && (!outdeg || !indeg || !nxt || !lab || !vclass)) ||
        (n_records > 0 && (!keys || !vals || !bflag || !flipped || !hfrom || !hto || n_faces == 0 || n_rows == 0)))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_LOOPS, s, 0.0, 28.0 * (double)n_records + 24.0 * (double)n_rows);
    if (n_rows > 0) {
        MORIG_HIP_TRY(hipMemsetAsync(outdeg, 0, (size_t)n_rows * sizeof(int32_t), s));
        MORIG_HIP_TRY(hipMemsetAsync(indeg, 0, (size_t)n_rows * sizeof(int32_t), s));
        MORIG_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)nxt, 0x7fffffff, (size_t)n_rows, s));
    }
    if (n_records > 0) {
        mf_boundary_edges_kernel<<<cdiv(n_records, 256), 256, 0, s>>>((const long long*)keys, vals, bflag, n_records, flipped, n_faces, n_rows, hfrom,
                                                                      hto, outdeg, indeg, nxt);
        MORIG_LAUNCH_CHECK();
    }
    if (n_rows > 0) {
        mf_boundary_verts_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(outdeg, indeg, n_rows, nxt, lab, vclass);
        MORIG_LAUNCH_CHECK();
    }
    return MORIG_OK;
}

int morig_meshfix_loop_round(const int32_t* lab, const int32_t* nxt, int32_t n_rows, int32_t* lab2, int32_t* nxt2, void* stream) {
    if (!rows_ok(n_rows)) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!lab || !nxt || !lab2 || !nxt2 || lab == lab2 || nxt == nxt2) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_LOOPS, s, 0.0, 24.0 * (double)n_rows);
    mf_loop_round_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(lab, nxt, n_rows, lab2, nxt2);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_loop_centroid(const double* verts, int32_t n_rows, const int64_t* order, const int64_t* lptr, int32_t n_loops, const int64_t* sel,
                                int32_t n_sel, double* centroid, void* stream) {
    if (!rows_ok(n_rows) || !rows_ok(n_loops) || !rows_ok(n_sel) || n_sel > n_loops) return MORIG_E_INVALID;
    if (n_sel == 0) return MORIG_OK;
    if (!verts || !order || !lptr || !sel || !centroid) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_FILL, s, 0.0, 32.0 * (double)n_rows);
    mf_loop_centroid_kernel<<<cdiv(n_sel, 4), 256, 0, s>>>(verts, n_rows, (const long long*)order, (const long long*)lptr, n_loops, (const long long*)sel,
                                                           n_sel, centroid);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_fill_mark(const int32_t* vclass, const int32_t* lab, const int32_t* slot, int32_t n_rows, int32_t* emit, void* stream) {
    if (!rows_ok(n_rows)) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!vclass || !lab || !slot || !emit) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_FILL, s, 0.0, 16.0 * (double)n_rows);
    mf_fill_mark_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(vclass, lab, slot, n_rows, emit);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_meshfix_fill_emit(const int32_t* nxt0, const int32_t* emit, const int64_t* erank, const int32_t* lab, const int32_t* slot,
                            const int32_t* vptr, const int64_t* sptr, int32_t n_rows, int32_t n_meshes, int64_t n_out, int64_t* out_faces,
                            void* stream) {
    if (!rows_ok(n_rows) || n_meshes < 0 || n_out < 0 || n_out > n_rows) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0 || n_out == 0) return MORIG_OK;
    if (!nxt0 || !emit || !erank || !lab || !slot || !vptr || !sptr || !out_faces) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MESHFIX_FILL, s, 0.0, 16.0 * (double)n_rows + 40.0 * (double)n_out);
    mf_fill_emit_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(nxt0, emit, (const long long*)erank, lab, slot, vptr, (const long long*)sptr, n_rows, n_meshes,
                                                          n_out, (long long*)out_faces);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
