// Local rigid motion of a deforming mesh (morig_amd/local_motion.py): the reference's get_gt_rotation_icp
// (data_proc/common_ops.py:47-78) for a ragged batch and whole clips. Everything is float64 in the written order of operations
// (contraction off) or integer; the only atomics are integer ORs into LDS bitsets and integer ORs / ADDs into the status words: two runs
// give the same bits, and a mesh alone gives the bits it gives inside a batch.
//
// patches   one wave per vertex, launched twice (count, then fill; the host's scan goes between). The reference's two rounds of "union
//           of my members' lists" over the one-ring are the end points of the walks of EXACTLY four edges from v: S0 = {v},
//           S(k + 1) = the neighbours of S(k), in two LDS bitsets per wave that change roles (integer atomicOr: a set, so the order of
//           arrival is free). On a mesh whose every edge lies in a proper triangle that is breadth-first depth <= 4 with v included; on
//           an edge of a degenerate face (a, a, b) alone it is not, and the walks are what the reference computes. The one-ring comes as
//           the sorted keys of morig_transfer_keys (6 per face; duplicates stay, a set absorbs them) with their row pointer. S4 is then
//           read in ascending words, 64 words a pass: per non-empty word 32 lanes take one member each, compute its distance, and
//           ballots count it under the three rungs (count) or compact the members under the chosen rung in ascending index (fill).
//           A vertex in no face keeps the patch {v} and is counted in status[1].
// fit       one lane per (vertex, frame), flat index v * T + t: in a clip a wave spans consecutive frames of one vertex, so the patch
//           ids and the rest points are wave-uniform and the target loads run along the frames. localfit_core.h per lane.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the rule headers: the pragma holds from here on

#include "localfit_core.h"

namespace morig {

namespace {

constexpr int PATCH_WAVES = 4;                 // vertices per workgroup of the patch kernel
constexpr int MAX_VERTS = MORIG_LOCAL_MAX_VERTS;
constexpr int FIT_BLOCK = 256;

__device__ __forceinline__ bool finite3(const double* p) {
    return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0;             // false for NaN and the infinities
}

// ------------------------------------------------------------------------------------------------------------------------ patches
// FILL false: counts[v], rung[v] written. FILL true: counts is the exclusive prefix sum [n_verts + 1] of the first pass, rung is read,
// ids written. words: 32-bit words per bitset, >= ceil(the largest mesh / 32); dynamic LDS = PATCH_WAVES * 2 * words words.
template <bool FILL>
__global__ void __launch_bounds__(PATCH_WAVES * 64) local_patches_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, int n_meshes,
                                                                          int n_verts, const int* __restrict__ rowptr,
                                                                          const long long* __restrict__ keys, double r0, double r1, double r2,
                                                                          int words, int* __restrict__ counts, int* __restrict__ rung,
                                                                          int* __restrict__ ids, int* __restrict__ status) {
    extern __shared__ unsigned s_bits[];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int gv = (int)blockIdx.x * PATCH_WAVES + wave;
    const bool live = gv < n_verts;
    unsigned* cur = s_bits + (size_t)wave * 2 * words;
    unsigned* nxt = cur + words;
    int v0 = 0, nv = 0, v = 0, W = 0;
    if (live) {
        const int b = segment_of(vptr, n_meshes, gv);
        v0 = vptr[b];
        nv = min(vptr[b + 1] - v0, MAX_VERTS);                                          // the entry point refuses more before the launch
        v = gv - v0;
        W = min((nv + 31) >> 5, words);
        if (v0 < 0 || v < 0 || v >= nv || (v >> 5) >= W || (long long)v0 + nv > n_verts) { nv = 0; W = 0; }      // a bad vptr: nothing to walk
    }
    for (int w = lane; w < W; w += 64) { cur[w] = 0u; nxt[w] = 0u; }
    __syncthreads();
    if (W > 0 && lane == 0) cur[v >> 5] = 1u << (v & 31);
    __syncthreads();
    for (int level = 0; level < 4; ++level) {
        for (int w = lane; w < W; w += 64) {
            unsigned bits = cur[w];
            while (bits) {
                const int u = w * 32 + __ffs((int)bits) - 1;
                bits &= bits - 1u;
                if (u >= nv) continue;
                const int e1 = rowptr[(size_t)v0 + u + 1];
                for (int e = rowptr[(size_t)v0 + u]; e < e1; ++e) {
                    const int n = (int)(keys[e] & 0xffffffffLL);
                    if (n >= 0 && n < nv && (n >> 5) < W) atomicOr(&nxt[n >> 5], 1u << (n & 31));
                }
            }
        }
        __syncthreads();
        for (int w = lane; w < W; w += 64) cur[w] = 0u;
        __syncthreads();
        unsigned* t = cur; cur = nxt; nxt = t;
    }
    const bool lone = W > 0 && rowptr[(size_t)gv + 1] == rowptr[(size_t)gv];           // in no face: the reference raises; here {v}
    if (lone && lane == 0) cur[v >> 5] = 1u << (v & 31);
    __syncthreads();
    if (W == 0) {
        if (live && !FILL && lane == 0) { counts[gv] = 0; rung[gv] = 2; }
        return;
    }
    double p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = verts[((size_t)v0 + v) * 3 + c];
    int c0 = 0, c1 = 0, c2 = 0;
    int at = 0, end = 0;
    double rsel = 0.0;
    if (FILL) {
        const int r = rung[gv];
        rsel = r == 0 ? r0 : (r == 1 ? r1 : r2);
        at = counts[gv];
        end = counts[gv + 1];
    }
    for (int w0 = 0; w0 < W; w0 += 64) {
        const unsigned word = w0 + lane < W ? cur[w0 + lane] : 0u;
        unsigned long long nz = __ballot(word != 0u);
        while (nz) {                                                                    // wave-uniform: nz is a ballot
            const int l = __ffsll((long long)nz) - 1;
            nz &= nz - 1ull;
            const unsigned bits = (unsigned)__shfl((int)word, l);
            const int u = (w0 + l) * 32 + lane;
            const bool member = lane < 32 && ((bits >> (lane & 31)) & 1u) && u < nv;
            double d = INFINITY;
            if (member) {
                double q[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) q[c] = verts[((size_t)v0 + u) * 3 + c];
                d = morig_localfit::dist(p, q);
            }
            if (!FILL) {
                c0 += __popcll(__ballot(member && d < r0));
                c1 += __popcll(__ballot(member && d < r1));
                c2 += __popcll(__ballot(member && d < r2));
            } else {
                const bool take = member && d < rsel;
                const unsigned long long mask = __ballot(take);
                const int slot = at + __popcll(mask & ((1ull << lane) - 1ull));
                if (take && slot < end) ids[slot] = u;
                at += __popcll(mask);
            }
        }
    }
    if (!FILL && lane == 0) {
        const int r = morig_localfit::choose_rung(c0, c1, c2);
        counts[gv] = r == 0 ? c0 : (r == 1 ? c1 : c2);
        rung[gv] = r;
        if (lone) atomicAdd(status + 1, 1);                                             // integers: the order of the additions is free
        if (!finite3(p)) atomicOr(status, MORIG_LOCAL_BAD_COORD);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ fit
template <typename T>
__global__ void __launch_bounds__(FIT_BLOCK) local_fit_kernel(const double* __restrict__ verts0, const T* __restrict__ traj, const int* __restrict__ vptr,
                                                              int n_meshes, int n_verts, int frames, const int* __restrict__ pptr,
                                                              const int* __restrict__ ids, int n_ids, double* __restrict__ rot6d,
                                                              double* __restrict__ trans, double* __restrict__ gap, double* __restrict__ residual,
                                                              int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * FIT_BLOCK + threadIdx.x;
    if (i >= (long long)n_verts * frames) return;
    const int gv = (int)(i / frames), t = (int)(i - (long long)gv * frames);
    const int b = segment_of(vptr, n_meshes, gv);
    const int v0 = vptr[b];
    int nv = vptr[b + 1] - v0;
    if (v0 < 0 || gv < v0 || (long long)v0 + nv > n_verts) nv = 0;                      // a vptr that does not ascend: nothing to read
    int e0 = pptr[gv], n = pptr[gv + 1] - e0;
    if (e0 < 0 || n < 0 || (long long)e0 + n > n_ids) { e0 = 0; n = 0; }
    double r6[6], tr[3], g, res;
    int bad = 0;
    morig_localfit::fit<T>(ids + e0, n, nv, verts0 + (size_t)v0 * 3, traj + ((size_t)v0 * frames + t) * 3, (long long)frames * 3, r6, tr, &g, &res, &bad);
    double2* r2 = reinterpret_cast<double2*>(rot6d + (size_t)i * 6);                    // 48 bytes a fit: 16-byte aligned
    r2[0] = make_double2(r6[0], r6[1]);
    r2[1] = make_double2(r6[2], r6[3]);
    r2[2] = make_double2(r6[4], r6[5]);
#pragma unroll
    for (int c = 0; c < 3; ++c) trans[(size_t)i * 3 + c] = tr[c];
    gap[i] = g;
    residual[i] = res;
    if (bad) atomicOr(status, MORIG_LOCAL_BAD_ID);
    if (n == 0 && t == 0) atomicAdd(status + 2, 1);
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_local_patches(const double* verts, const int32_t* vptr, int32_t n_meshes, int32_t n_verts, int32_t max_verts, const int32_t* rowptr,
                        const int64_t* keys, double rung0, double rung1, double rung2, int32_t* counts, int32_t* rung, int32_t* ids, int32_t* status,
                        void* stream) {
    if (n_meshes < 0 || n_verts < 0 || max_verts < 0) return MORIG_E_INVALID;
    if (max_verts > MORIG_LOCAL_MAX_VERTS) return MORIG_E_UNSUPPORTED;
    if (n_verts == 0) return MORIG_OK;
    if (!verts || !vptr || !rowptr || !counts || !rung || !status || n_meshes == 0 || max_verts == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int words = cdiv(max_verts, 32);
    const size_t lds = (size_t)PATCH_WAVES * 2 * words * sizeof(unsigned);              // at most 32 KiB
    const int grid = cdiv(n_verts, PATCH_WAVES);
    ProfScope ps(K_MISC, s, 0.0, 0.0);
    if (ids)
        local_patches_kernel<true><<<grid, PATCH_WAVES * 64, lds, s>>>(verts, vptr, n_meshes, n_verts, rowptr, (const long long*)keys, rung0, rung1, rung2,
                                                                       words, counts, rung, ids, status);
    else
        local_patches_kernel<false><<<grid, PATCH_WAVES * 64, lds, s>>>(verts, vptr, n_meshes, n_verts, rowptr, (const long long*)keys, rung0, rung1, rung2,
                                                                        words, counts, rung, ids, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_local_fit(const double* verts0, const void* traj, int32_t traj_is_f32, const int32_t* vptr, int32_t n_meshes, int32_t n_verts, int32_t frames,
                    const int32_t* patch_ptr, const int32_t* ids, int32_t n_ids, double* rot6d, double* trans, double* gap, double* residual,
                    int32_t* status, void* stream) {
    if (n_meshes < 0 || n_verts < 0 || frames < 0 || n_ids < 0) return MORIG_E_INVALID;
    const long long n_fits = (long long)n_verts * frames;
    if (n_fits > 0x7fffffffLL / 6) return MORIG_E_UNSUPPORTED;
    if (n_fits == 0) return MORIG_OK;
    if (!verts0 || !traj || !vptr || !patch_ptr || !rot6d || !trans || !gap || !residual || !status || n_meshes == 0) return MORIG_E_INVALID;
    if (n_ids > 0 && !ids) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_MISC, s, 0.0, 88.0 * (double)n_fits);
    const int grid = cdiv(n_fits, FIT_BLOCK);
    if (traj_is_f32)
        local_fit_kernel<float><<<grid, FIT_BLOCK, 0, s>>>(verts0, (const float*)traj, vptr, n_meshes, n_verts, frames, patch_ptr, ids, n_ids, rot6d, trans,
                                                           gap, residual, status);
    else
        local_fit_kernel<double><<<grid, FIT_BLOCK, 0, s>>>(verts0, (const double*)traj, vptr, n_meshes, n_verts, frames, patch_ptr, ids, n_ids, rot6d,
                                                            trans, gap, residual, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
