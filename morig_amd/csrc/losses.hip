// Training losses (models/customized_losses.py: infoNCE :107-134, multi_pos_infoNCE :137-158, chamfer_distance_with_average :231-251),
// batched over the pairs / meshes of a batch, forward and backward. No floating-point atomics anywhere: every sum runs in a fixed order,
// two runs on the same inputs give the same bits. The only atomics are integer ones (status bits, 64-bit arg-min keys).
//
// infoNCE      The logits of a pair are a GEMM (correspondence rows x keys, K = 64) that is never written to memory. It runs on the exact
//              float32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit an fmaf chain), as cosine_knn_kernel (deform.hip) runs its similarity:
//              a wave OWNS 32 columns of the tile (their features stay in registers) and STREAMS the other side 32 rows at a time.
//              forward: owned = correspondence rows (gathered anchors), streamed = the pair's keys; a lane keeps the running maximum and
//              sum of its column (log-sum-exp), the two lanes of a column merge at the end. backward: the tile is recomputed from lse,
//              G = (softmax - onehot) * coef leaves the accumulator registers in exactly the layout the B operand of the second product
//              needs, d(owned)^T += streamed^T G, the streamed rows transposed through the wave's LDS slab. The same kernel runs with the
//              roles swapped for the key side (owned = 32 keys, streamed = all correspondence rows of the pair).
// multi-pos    one wave per sampled row: its 200 negatives and 10 positives are 210 dot products, wave reductions only. backward: the row's
//              coefficients go into a dense G row (a thread owns columns: duplicates are added in slot order), then (G + G^T) F per mesh.
// chamfer      one workgroup per 256 vertices of a mesh, the mesh's joints in LDS; both arg-mins through 64-bit keys (distance bits above
//              the index: the smallest index wins a tie).
#include "common.h"

namespace morig {

// status bits (include/morig_hip.h)
constexpr int ST_INDEX = MORIG_LOSS_ST_INDEX, ST_UNSORTED = MORIG_LOSS_ST_UNSORTED, ST_SEGMENT = MORIG_LOSS_ST_SEGMENT, ST_SIZE = MORIG_LOSS_ST_SIZE;
constexpr int ST_FATAL = ST_UNSORTED | ST_SEGMENT;          // the segment offsets cannot be trusted: nothing is read through them

// ---------------------------------------------------------------------------------------------------
// ptr[g] = first row of segment g of a sorted batch vector, ptr[S] = n. One thread per boundary.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_ptr_kernel(const long long* __restrict__ batch, int n, int S, int* __restrict__ ptr,
                                                      int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    const long long prev = i == 0 ? -1 : batch[i - 1];
    const long long cur = i == n ? S : batch[i];
    if (i < n && (cur < 0 || cur >= S)) { atomicOr(status, ST_SEGMENT); return; }
    if (i > 0 && (prev < 0 || prev >= S)) return;                     // flagged by the thread of row i - 1
    if (cur < prev) { atomicOr(status, ST_UNSORTED); return; }
    for (long long g = prev + 1; g <= cur; ++g) ptr[g] = i;
}

// out[0] = scale * sum v[0 .. n) (fp64, fixed order), NaN when a status bit is set. One workgroup.
__global__ __launch_bounds__(256) void sum_scale_kernel(const float* __restrict__ v, int n, double scale, float* __restrict__ out,
                                                        const int* __restrict__ status) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
    s = block_sum256(s, sh);
    if (threadIdx.x == 0) out[0] = *status ? NAN : (float)(s * scale);
}

// ===================================================================================================
// infoNCE
// ===================================================================================================
constexpr int NCE_C = 64;
constexpr int NCE_LD = 68;                               // LDS row stride of the transposing slab (floats; 16-byte aligned rows)

struct NceDir {
    const float* anchor; int ld_a; const int* ptr_a;       // the matrix the correspondence rows gather their anchors from
    const float* key; int ld_k; const int* ptr_k;          // the matrix whose rows of the pair are the classes
    const long long* corr; const int* ptr_c;               // [rows][2]: (anchor, label), local to the pair
    int row_off;                                           // this direction's offset in lse / row_loss / d_rows
    float* d_key;                                          // backward: [rows of key][64]
};
struct NceParams {
    NceDir d[2];                                           // 0: v2p (anchor = vertices, keys = points), 1: p2v
    int B; float tau;
    float* lse; float* row_loss; float* loss; const float* upstream; float* d_rows;
    int* status;
};

// the 32 features [32 hi, 32 hi + 32) of a row: contraction step s of the 32x32x2 MFMA pairs feature s (k = 0, lanes 0..31) with feature
// 32 + s (k = 1, lanes 32..63) -- any pairing is a valid contraction order as long as both operands use it
__device__ __forceinline__ void nce_load32(const float* __restrict__ p, float (&v)[32]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
        v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
    }
}
// acc[r] = <streamed row (r & 3) + 8 (r >> 2) + 4 hi, owned row (lane & 31)>
__device__ __forceinline__ f32x16 nce_tile(const float (&streamed)[32], const float (&owned)[32]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(streamed[s], owned[s], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ int nce_rowmap(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void nce_fwd_kernel(const NceParams p) {
    if (*p.status & ST_FATAL) return;
    const int dir = blockIdx.z, b = blockIdx.y;
    const NceDir& d = p.d[dir];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    const int cs = d.ptr_c[b], ce = d.ptr_c[b + 1];
    const int r0 = cs + (blockIdx.x * 4 + wave) * 32;
    if (r0 >= ce) return;                                 // wave-uniform; the kernel has no block barrier
    const int as = d.ptr_a[b], na = d.ptr_a[b + 1] - as, ks = d.ptr_k[b], nk = d.ptr_k[b + 1] - ks;
    const int row = r0 + l31;
    const bool live = row < ce;
    const int rr = live ? row : ce - 1;
    // a pair without v2p rows contributes nothing, its p2v rows included (customized_losses.py:115-117)
    const bool skipped = dir == 1 && p.d[0].ptr_c[b + 1] == p.d[0].ptr_c[b];
    if (skipped || na <= 0 || nk <= 0) {
        if (!skipped && hi == 0 && live) atomicOr(p.status, ST_INDEX);       // rows that point into an empty set
        if (hi == 0 && live) { p.lse[d.row_off + row] = 0.f; p.row_loss[d.row_off + row] = 0.f; }
        return;
    }
    long long ai = d.corr[2 * (size_t)rr], li = d.corr[2 * (size_t)rr + 1];
    if (live && hi == 0 && (ai < 0 || ai >= na || li < 0 || li >= nk)) atomicOr(p.status, ST_INDEX);
    ai = clampll(ai, 0, na - 1); li = clampll(li, 0, nk - 1);
    float own[32];
    nce_load32(d.anchor + (size_t)(as + ai) * d.ld_a + 32 * hi, own);
    const float tau = p.tau;
    const int label = (int)li;
    float m = -INFINITY, s = 0.f, pos = 0.f;
    for (int base = 0; base < nk; base += 32) {
        float str[32];
        nce_load32(d.key + (size_t)(ks + min(base + l31, nk - 1)) * d.ld_k + 32 * hi, str);
        f32x16 acc = nce_tile(str, own);
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = base + nce_rowmap(r, hi);
            const float v = k < nk ? acc[r] / tau : -INFINITY;
            if (k == label) pos = v;
            acc[r] = v;
            tm = fmaxf(tm, v);
        }
        if (tm > -INFINITY) {                              // the running maximum: logits reach +-100 at tau = 0.01
            const float mn = fmaxf(m, tm);
            float add = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) add += expf(acc[r] - mn);
            s = s * expf(m - mn) + add;
            m = mn;
        }
    }
    // the two lanes of a column hold interleaved key rows: merge, lower half first
    const float om = __shfl_xor(m, 32), os = __shfl_xor(s, 32), op = __shfl_xor(pos, 32);
    if (hi == 0 && live) {
        const float M = fmaxf(m, om);
        const float S = s * expf(m - M) + os * expf(om - M);      // a half without a valid key: s = 0, m = -inf
        const float lse = M + logf(S);
        p.lse[d.row_off + row] = lse;
        p.row_loss[d.row_off + row] = lse - (pos + op);
    }
}

// sum over pairs of [mean of the v2p rows + mean of the p2v rows] / pairs, the skipped pairs left out. One workgroup, fp64, fixed order.
__global__ __launch_bounds__(256) void nce_reduce_kernel(const NceParams p) {
    __shared__ double sh[256];
    if (*p.status) { if (threadIdx.x == 0) p.loss[0] = NAN; return; }
    double total = 0.0;
    for (int b = 0; b < p.B; ++b) {
        if (p.d[0].ptr_c[b + 1] == p.d[0].ptr_c[b]) continue;
        for (int dir = 0; dir < 2; ++dir) {
            const int cs = p.d[dir].ptr_c[b], ce = p.d[dir].ptr_c[b + 1];
            if (ce <= cs) continue;
            double s = 0.0;
            for (int i = cs + threadIdx.x; i < ce; i += 256) s += (double)p.row_loss[p.d[dir].row_off + i];
            total += block_sum256(s, sh) / (double)(ce - cs);
        }
    }
    if (threadIdx.x == 0) p.loss[0] = (float)(total / (double)p.B);
}

// OWN_ROWS: a wave owns 32 correspondence rows and streams the pair's keys      -> d_rows[row][64] = sum_k G[row][k] key[k]
// else    : a wave owns 32 keys and streams the pair's correspondence rows      -> d_key[key][64]  = sum_r G[r][key] anchor[r]
// G[r][k] = (exp(logit - lse[r]) - [label[r] == k]) * upstream / (tau * rows * pairs)
template <bool OWN_ROWS>
__global__ __launch_bounds__(256) void nce_bwd_kernel(const NceParams p) {
    __shared__ __attribute__((aligned(16))) float sh_all[4][32 * NCE_LD];
    if (*p.status & ST_FATAL) return;
    const int dir = blockIdx.z, b = blockIdx.y;
    const NceDir& d = p.d[dir];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    float* sh = sh_all[wave];
    const int cs = d.ptr_c[b], nrows = d.ptr_c[b + 1] - cs;
    const int as = d.ptr_a[b], na = d.ptr_a[b + 1] - as, ks = d.ptr_k[b], nk = d.ptr_k[b + 1] - ks;
    const int n_own = OWN_ROWS ? nrows : nk, n_str = OWN_ROWS ? nk : nrows;
    const int o0 = (blockIdx.x * 4 + wave) * 32;
    if (o0 >= n_own) return;                              // wave-uniform; LDS slabs are per wave, no block barrier
    const int o = o0 + l31;
    const bool live = o < n_own;
    float* out = OWN_ROWS ? p.d_rows + (size_t)(d.row_off + cs + o) * NCE_C : d.d_key + (size_t)(ks + o) * NCE_C;
    const bool skipped = dir == 1 && p.d[0].ptr_c[b + 1] == p.d[0].ptr_c[b];
    if (skipped || n_str <= 0 || na <= 0 || nk <= 0) {
        if (live) {
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<f32x4*>(out + 32 * hi + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    const float tau = p.tau;
    const float coef = p.upstream[0] / (tau * (float)nrows * (float)p.B);
    const int oc = live ? o : n_own - 1;
    float own[32];
    float own_lse = 0.f; int own_label = -1;
    if (OWN_ROWS) {
        const size_t rr = (size_t)(cs + oc);
        const long long ai = clampll(d.corr[2 * rr], 0, na - 1);
        own_label = (int)clampll(d.corr[2 * rr + 1], 0, nk - 1);
        own_lse = p.lse[d.row_off + rr];
        nce_load32(d.anchor + (size_t)(as + ai) * d.ld_a + 32 * hi, own);
    } else {
        nce_load32(d.key + (size_t)(ks + oc) * d.ld_k + 32 * hi, own);
    }
    f32x16 g0, g1;                                     // d(owned)^T: features 0..31 / 32..63 (rows) x owned (columns)
#pragma unroll
    for (int r = 0; r < 16; ++r) { g0[r] = 0.f; g1[r] = 0.f; }
    for (int base = 0; base < n_str; base += 32) {
        const int t = min(base + l31, n_str - 1);
        const float* srow;
        if (OWN_ROWS) srow = d.key + (size_t)(ks + t) * d.ld_k;
        else srow = d.anchor + (size_t)(as + clampll(d.corr[2 * (size_t)(cs + t)], 0, na - 1)) * d.ld_a;
        float str[32];
        nce_load32(srow + 32 * hi, str);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            *reinterpret_cast<f32x4*>(sh + l31 * NCE_LD + 32 * hi + 4 * q) = f32x4{str[4 * q], str[4 * q + 1], str[4 * q + 2], str[4 * q + 3]};
        f32x16 acc = nce_tile(str, own);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tr = base + nce_rowmap(r, hi);
            float g = 0.f;
            if (tr < n_str) {
                if (OWN_ROWS) {
                    g = (expf(acc[r] / tau - own_lse) - (tr == own_label ? 1.f : 0.f)) * coef;
                } else {
                    const size_t rr = (size_t)(cs + tr);
                    const int lab = (int)clampll(d.corr[2 * rr + 1], 0, nk - 1);
                    g = (expf(acc[r] / tau - p.lse[d.row_off + rr]) - (lab == o ? 1.f : 0.f)) * coef;
                }
            }
            acc[r] = g;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // step s contracts streamed rows rowmap(s, 0) (k = 0) and rowmap(s, 1) (k = 1): acc[s] IS the B operand
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float* srcrow = sh + nce_rowmap(s, hi) * NCE_LD + l31;
            g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(srcrow[0], acc[s], g0, 0, 0, 0);
            g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(srcrow[32], acc[s], g1, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (live) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<f32x4*>(out + 8 * q + 4 * hi) = f32x4{g0[4 * q], g0[4 * q + 1], g0[4 * q + 2], g0[4 * q + 3]};
            *reinterpret_cast<f32x4*>(out + 32 + 8 * q + 4 * hi) = f32x4{g1[4 * q], g1[4 * q + 1], g1[4 * q + 2], g1[4 * q + 3]};
        }
    }
}

// grad[v] = (sum of d_rows over the correspondence rows whose anchor is v, in row order) + d_key[v]; 16 threads per row
__global__ __launch_bounds__(256) void nce_combine_kernel(const float* __restrict__ d_rows, const int* __restrict__ rowptr,
                                                          const int* __restrict__ order, const float* __restrict__ d_key, int n,
                                                          float* __restrict__ grad, int ldg) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int v = t >> 4, q = t & 15;
    if (v >= n) return;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = rowptr[v]; k < rowptr[v + 1]; ++k) s += *reinterpret_cast<const f32x4*>(d_rows + (size_t)order[k] * NCE_C + 4 * q);
    s += *reinterpret_cast<const f32x4*>(d_key + (size_t)v * NCE_C + 4 * q);
    float* o = grad + (size_t)v * ldg + 4 * q;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
}

// ===================================================================================================
// multi-positive infoNCE on gathered sample rows F [meshes * S][ldf]
// ===================================================================================================
constexpr int MP_MAX_POS = 64, MP_MAX_NEG = 256;

__device__ __forceinline__ float mp_dot(const float* __restrict__ a, const float* __restrict__ b, int D) {
    float s = 0.f;
    for (int c = 0; c < D; c += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a + c), y = *reinterpret_cast<const f32x4*>(b + c);
        s = fmaf(x[0], y[0], s); s = fmaf(x[1], y[1], s); s = fmaf(x[2], y[2], s); s = fmaf(x[3], y[3], s);
    }
    return s;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int mp_id(const int* __restrict__ ids, size_t at, int S, int* status) {
    int id = ids[at];
    if (id < 0 || id >= S) { atomicOr(status, ST_INDEX); id = id < 0 ? 0 : S - 1; }
    return id;
}

// one wave per sampled row: neg_max / neg_sum = running maximum and sum of exp over its negatives,
// row_loss = (1 / n_pos) sum_j [log(exp(p_j) + sum_negs exp(n)) - p_j]
__global__ __launch_bounds__(256) void multipos_fwd_kernel(const float* __restrict__ F, int ldf, int D, const int* __restrict__ pos, int n_pos,
                                                           const int* __restrict__ neg, int n_neg, int S, int n_rows,
                                                           float* __restrict__ neg_max, float* __restrict__ neg_sum,
                                                           float* __restrict__ row_loss, int* __restrict__ status) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float* Fm = F + (size_t)(row / S) * S * ldf;
    const float* fr = F + (size_t)row * ldf;
    float v[MP_MAX_NEG / 64];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MP_MAX_NEG / 64; ++k) {
        const int slot = lane + 64 * k;
        v[k] = -INFINITY;
        if (slot < n_neg) v[k] = mp_dot(fr, Fm + (size_t)mp_id(neg, (size_t)row * n_neg + slot, S, status) * ldf, D);
        m = fmaxf(m, v[k]);
    }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MP_MAX_NEG / 64; ++k) if (lane + 64 * k < n_neg) s += expf(v[k] - m);
    s = wave_sum(s);
    float t = 0.f;
    if (lane < n_pos) {
        const float pj = mp_dot(fr, Fm + (size_t)mp_id(pos, (size_t)row * n_pos + lane, S, status) * ldf, D);
        const float mm = fmaxf(m, pj);
        t = logf(expf(pj - mm) + s * expf(m - mm)) + mm - pj;
    }
    t = wave_sum(t);
    if (lane == 0) { neg_max[row] = m; neg_sum[row] = s; row_loss[row] = t / (float)n_pos; }
}

// one workgroup per sampled row r: G[r][c] = sum of the coefficients of the slots that drew c (positives, then negatives, slot order);
// coefficient of positive j: (softmax_j(p_j) - 1) * w, of negative k: sum_j softmax_j(n_k) * w, w = upstream / (n_pos * S * meshes)
__global__ __launch_bounds__(256) void multipos_g_kernel(const float* __restrict__ F, int ldf, int D, const int* __restrict__ pos, int n_pos,
                                                         const int* __restrict__ neg, int n_neg, int S, int n_rows,
                                                         const float* __restrict__ neg_max, const float* __restrict__ neg_sum,
                                                         const float* __restrict__ upstream, float* __restrict__ G, int* __restrict__ status) {
    __shared__ int s_id[MP_MAX_POS + MP_MAX_NEG];
    __shared__ float s_c[MP_MAX_POS + MP_MAX_NEG];
    __shared__ float s_w[MP_MAX_POS];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* Fm = F + (size_t)(row / S) * S * ldf;
    const float* fr = F + (size_t)row * ldf;
    const float m = neg_max[row], s = neg_sum[row];
    const float w = upstream[0] / ((float)n_pos * (float)S * (float)(n_rows / S));
    if (tid < n_pos) {
        const int id = mp_id(pos, (size_t)row * n_pos + tid, S, status);
        const float pj = mp_dot(fr, Fm + (size_t)id * ldf, D);
        const float mm = fmaxf(m, pj);
        const float ep = expf(pj - mm), den = ep + s * expf(m - mm);
        s_id[tid] = id; s_c[tid] = (ep / den - 1.f) * w; s_w[tid] = expf(m - mm) / den;
    }
    __syncthreads();
    if (tid < n_neg) {
        const int id = mp_id(neg, (size_t)row * n_neg + tid, S, status);
        const float nk = mp_dot(fr, Fm + (size_t)id * ldf, D);
        float ws = 0.f;
        for (int j = 0; j < n_pos; ++j) ws += s_w[j];
        s_id[n_pos + tid] = id; s_c[n_pos + tid] = expf(nk - m) * ws * w;
    }
    __syncthreads();
    for (int c = tid; c < S; c += 256) {
        float g = 0.f;
        for (int k = 0; k < n_pos + n_neg; ++k) if (s_id[k] == c) g += s_c[k];
        G[(size_t)row * S + c] = g;
    }
}

// grad[rows[m S + i]] = sum_k (G_m[i][k] + G_m[k][i]) F_m[k]: a sampled row receives gradient as a row and as a column of the products.
// workgroup = 64 sample rows (lanes) x feature quads (wave w owns quads w, w + 4, ...); both 64 x 64 tiles of G go through LDS
__global__ __launch_bounds__(256) void multipos_apply_kernel(const float* __restrict__ G, const float* __restrict__ F, int ldf, int D, int S,
                                                             const int* __restrict__ rows, float* __restrict__ grad, int ldg) {
    __shared__ float sA[64 * 65], sB[64 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mesh = blockIdx.y, i0 = blockIdx.x * 64;
    const float* Gm = G + (size_t)mesh * S * S;
    const float* Fm = F + (size_t)mesh * S * ldf;
    const int nq = D >> 2;
    float acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a) { acc[a][0] = 0.f; acc[a][1] = 0.f; acc[a][2] = 0.f; acc[a][3] = 0.f; }
    for (int kb = 0; kb < S; kb += 64) {
        for (int r = wave; r < 64; r += 4) {
            sA[r * 65 + lane] = (i0 + r < S && kb + lane < S) ? Gm[(size_t)(i0 + r) * S + kb + lane] : 0.f;     // G[i0 + r][kb + lane]
            sB[r * 64 + lane] = (kb + r < S && i0 + lane < S) ? Gm[(size_t)(kb + r) * S + i0 + lane] : 0.f;     // G[kb + r][i0 + lane]
        }
        __syncthreads();
        const int kn = min(64, S - kb);
        for (int kk = 0; kk < kn; ++kk) {
            const float g = sA[lane * 65 + kk] + sB[kk * 64 + lane];
            const float* fk = Fm + (size_t)(kb + kk) * ldf;
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const int q = wave + 4 * a;
                if (q < nq) {
                    const f32x4 f = *reinterpret_cast<const f32x4*>(fk + 4 * q);
                    acc[a][0] = fmaf(g, f[0], acc[a][0]); acc[a][1] = fmaf(g, f[1], acc[a][1]);
                    acc[a][2] = fmaf(g, f[2], acc[a][2]); acc[a][3] = fmaf(g, f[3], acc[a][3]);
                }
            }
        }
        __syncthreads();
    }
    if (i0 + lane < S) {
        float* o = grad + (size_t)rows[mesh * S + i0 + lane] * ldg;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int q = wave + 4 * a;
            if (q < nq) { o[4 * q] = acc[a][0]; o[4 * q + 1] = acc[a][1]; o[4 * q + 2] = acc[a][2]; o[4 * q + 3] = acc[a][3]; }
        }
    }
}

// ===================================================================================================
// chamfer: mean over meshes of 0.5 (mean_i min_j |p_i - q_j| + mean_j min_i |p_i - q_j|)
// ===================================================================================================
constexpr int CH_MAX_Q = MORIG_CHAMFER_MAX_JOINTS;
typedef unsigned long long u64;

__device__ __forceinline__ float ch_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(256) void chamfer_fwd_kernel(const float* __restrict__ p, const float* __restrict__ q, const int* __restrict__ ptr_p,
                                                          const int* __restrict__ ptr_q, int* __restrict__ arg1, float* __restrict__ d1,
                                                          u64* __restrict__ key2, int* __restrict__ status) {
    __shared__ float sq[CH_MAX_Q * 3];
    __shared__ u64 sk[CH_MAX_Q];
    if (*status & ST_FATAL) return;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ps = ptr_p[b], np = ptr_p[b + 1] - ps, qs = ptr_q[b], nq = ptr_q[b + 1] - qs;
    const int i = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= np) return;                    // block-uniform
    if (nq > CH_MAX_Q) { if (tid == 0) atomicOr(status, ST_SIZE); return; }
    for (int j = tid; j < nq * 3; j += 256) sq[j] = q[(size_t)qs * 3 + j];
    for (int j = tid; j < nq; j += 256) sk[j] = ~0ull;
    __syncthreads();
    if (i < np) {
        const float px = p[(size_t)(ps + i) * 3], py = p[(size_t)(ps + i) * 3 + 1], pz = p[(size_t)(ps + i) * 3 + 2];
        u64 best = ~0ull;
        for (int j = 0; j < nq; ++j) {
            const u64 bits = (u64)__float_as_uint(ch_dist(px, py, pz, sq[3 * j], sq[3 * j + 1], sq[3 * j + 2])) << 32;
            const u64 kj = bits | (unsigned)j;
            best = kj < best ? kj : best;
            atomicMin(&sk[j], bits | (unsigned)i);
        }
        arg1[ps + i] = (int)(unsigned)(best & 0xffffffffull);
        d1[ps + i] = __uint_as_float((unsigned)(best >> 32));
    }
    __syncthreads();
    for (int j = tid; j < nq; j += 256) atomicMin(&key2[qs + j], sk[j]);
}

__global__ __launch_bounds__(256) void chamfer_reduce_kernel(const float* __restrict__ d1, const u64* __restrict__ key2, const int* __restrict__ ptr_p,
                                                             const int* __restrict__ ptr_q, int B, float* __restrict__ loss,
                                                             const int* __restrict__ status) {
    __shared__ double sh[256];
    if (*status) { if (threadIdx.x == 0) loss[0] = NAN; return; }
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        const int ps = ptr_p[b], pe = ptr_p[b + 1], qs = ptr_q[b], qe = ptr_q[b + 1];
        double s1 = 0.0, s2 = 0.0;
        for (int i = ps + threadIdx.x; i < pe; i += 256) s1 += (double)d1[i];
        for (int j = qs + threadIdx.x; j < qe; j += 256) s2 += (double)__uint_as_float((unsigned)(key2[j] >> 32));
        s1 = block_sum256(s1, sh);
        s2 = block_sum256(s2, sh);
        total += 0.5 * (s1 / (double)(pe - ps) + s2 / (double)(qe - qs));     // an empty side: 0 / 0 = NaN, as the mean of nothing
    }
    if (threadIdx.x == 0) loss[0] = (float)(total / (double)B);
}

// gradient of the vertices: towards their nearest joint, plus -- for the vertices that are some joint's nearest -- those joints in index order
__global__ __launch_bounds__(256) void chamfer_bwd_p_kernel(const float* __restrict__ p, const float* __restrict__ q, const int* __restrict__ ptr_p,
                                                            const int* __restrict__ ptr_q, int B, const int* __restrict__ arg1,
                                                            const float* __restrict__ d1, const u64* __restrict__ key2,
                                                            const float* __restrict__ upstream, float* __restrict__ gp,
                                                            const int* __restrict__ status) {
    __shared__ float sq[CH_MAX_Q * 3];
    __shared__ float sd2[CH_MAX_Q];
    __shared__ int sa2[CH_MAX_Q];
    if (*status) return;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ps = ptr_p[b], np = ptr_p[b + 1] - ps, qs = ptr_q[b], nq = ptr_q[b + 1] - qs;
    const int i = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= np) return;
    for (int j = tid; j < nq * 3; j += 256) sq[j] = q[(size_t)qs * 3 + j];
    for (int j = tid; j < nq; j += 256) { const u64 k = key2[qs + j]; sa2[j] = (int)(unsigned)(k & 0xffffffffull); sd2[j] = __uint_as_float((unsigned)(k >> 32)); }
    __syncthreads();
    if (i >= np) return;
    const float up = upstream[0];
    const float w1 = up * 0.5f / ((float)B * (float)np), w2 = up * 0.5f / ((float)B * (float)nq);
    const float px = p[(size_t)(ps + i) * 3], py = p[(size_t)(ps + i) * 3 + 1], pz = p[(size_t)(ps + i) * 3 + 2];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const int a = arg1[ps + i];
    const float d = d1[ps + i];
    if (a >= 0 && a < nq && d > 0.f) {                     // a zero distance has a zero gradient, as torch's norm
        const float f = w1 / d;
        gx = f * (px - sq[3 * a]); gy = f * (py - sq[3 * a + 1]); gz = f * (pz - sq[3 * a + 2]);
    }
    for (int j = 0; j < nq; ++j)
        if (sa2[j] == i && sd2[j] > 0.f) {
            const float f = w2 / sd2[j];
            gx += f * (px - sq[3 * j]); gy += f * (py - sq[3 * j + 1]); gz += f * (pz - sq[3 * j + 2]);
        }
    gp[(size_t)(ps + i) * 3] = gx; gp[(size_t)(ps + i) * 3 + 1] = gy; gp[(size_t)(ps + i) * 3 + 2] = gz;
}

// gradient of the joints: one workgroup per mesh, a thread owns joints; its own nearest vertex first, then the vertices whose nearest joint
// it is, in vertex order (256 vertices at a time through LDS)
__global__ __launch_bounds__(256) void chamfer_bwd_q_kernel(const float* __restrict__ p, const float* __restrict__ q, const int* __restrict__ ptr_p,
                                                            const int* __restrict__ ptr_q, int B, const int* __restrict__ arg1,
                                                            const float* __restrict__ d1, const u64* __restrict__ key2,
                                                            const float* __restrict__ upstream, float* __restrict__ gq,
                                                            const int* __restrict__ status) {
    __shared__ float sp[256 * 3];
    __shared__ float sd[256];
    __shared__ int sa[256];
    if (*status) return;
    constexpr int OWN = CH_MAX_Q / 256;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ps = ptr_p[b], np = ptr_p[b + 1] - ps, qs = ptr_q[b], nq = ptr_q[b + 1] - qs;
    if (np <= 0) return;
    const float up = upstream[0];
    const float w1 = up * 0.5f / ((float)B * (float)np), w2 = up * 0.5f / ((float)B * (float)nq);
    float qx[OWN], qy[OWN], qz[OWN], gx[OWN], gy[OWN], gz[OWN];
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        const int j = tid + 256 * o;
        qx[o] = qy[o] = qz[o] = gx[o] = gy[o] = gz[o] = 0.f;
        if (j < nq) {
            qx[o] = q[(size_t)(qs + j) * 3]; qy[o] = q[(size_t)(qs + j) * 3 + 1]; qz[o] = q[(size_t)(qs + j) * 3 + 2];
            const u64 k = key2[qs + j];
            const int i2 = (int)(unsigned)(k & 0xffffffffull);
            const float d2 = __uint_as_float((unsigned)(k >> 32));
            if (i2 >= 0 && i2 < np && d2 > 0.f) {
                const float f = w2 / d2;
                gx[o] = -f * (p[(size_t)(ps + i2) * 3] - qx[o]); gy[o] = -f * (p[(size_t)(ps + i2) * 3 + 1] - qy[o]);
                gz[o] = -f * (p[(size_t)(ps + i2) * 3 + 2] - qz[o]);
            }
        }
    }
    for (int base = 0; base < np; base += 256) {
        const int n = min(256, np - base);
        if (tid < n) {
            sa[tid] = arg1[ps + base + tid]; sd[tid] = d1[ps + base + tid];
            sp[3 * tid] = p[(size_t)(ps + base + tid) * 3]; sp[3 * tid + 1] = p[(size_t)(ps + base + tid) * 3 + 1];
            sp[3 * tid + 2] = p[(size_t)(ps + base + tid) * 3 + 2];
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const int a = sa[t];
#pragma unroll
            for (int o = 0; o < OWN; ++o)
                if (a == tid + 256 * o && sd[t] > 0.f) {
                    const float f = w1 / sd[t];
                    gx[o] -= f * (sp[3 * t] - qx[o]); gy[o] -= f * (sp[3 * t + 1] - qy[o]); gz[o] -= f * (sp[3 * t + 2] - qz[o]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 0; o < OWN; ++o) {
        const int j = tid + 256 * o;
        if (j < nq) { gq[(size_t)(qs + j) * 3] = gx[o]; gq[(size_t)(qs + j) * 3 + 1] = gy[o]; gq[(size_t)(qs + j) * 3 + 2] = gz[o]; }
    }
}

}  // namespace morig

using namespace morig;

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int morig_loss_segment_ptr(const int64_t* batch, int32_t n, int32_t n_segments, int32_t* ptr, int32_t* status, void* stream) {
    if ((!batch && n > 0) || !ptr || !status || n < 0 || n_segments <= 0) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_CSR, s, 0.0, 0.0);
    hipLaunchKernelGGL(seg_ptr_kernel, dim3(cdiv((long)n + 1, 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(batch), n, n_segments,
                       ptr, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

static_assert(sizeof(morig_nce_args) == MORIG_NCE_STRUCT_BYTES, "include/morig_hip.h states the size");

static int nce_params(const morig_nce_args* args, bool backward, morig_nce_args& a, NceParams& p) {
    if (!take_args(args, a, MORIG_NCE_STRUCT_BYTES)) return MORIG_E_INVALID;
    if (a.n_pairs <= 0 || a.n_vtx < 0 || a.n_pts < 0 || a.n_v2p < 0 || a.n_p2v < 0 || !(a.tau > 0.f)) return MORIG_E_INVALID;
    if (a.C != NCE_C) return MORIG_E_UNSUPPORTED;
    if (!a.ptr_vtx || !a.ptr_pts || !a.ptr_v2p || !a.ptr_p2v || !a.lse || !a.status) return MORIG_E_INVALID;
    if ((a.n_vtx > 0 && !a.vtx) || (a.n_pts > 0 && !a.pts) || (a.n_v2p > 0 && !a.corr_v2p) || (a.n_p2v > 0 && !a.corr_p2v)) return MORIG_E_INVALID;
    if (a.ld_vtx < NCE_C || a.ld_pts < NCE_C || (a.ld_vtx & 3) || (a.ld_pts & 3) || !al16(a.vtx) || !al16(a.pts)) return MORIG_E_INVALID;
    if (!backward && (!a.row_loss || !a.loss)) return MORIG_E_INVALID;
    if (backward) {
        if (!a.upstream || !a.d_rows || !a.d_key_pts || !a.d_key_vtx || !a.rowptr_vtx || !a.rowptr_pts) return MORIG_E_INVALID;
        // a direction without rows has nothing to order, a side without rows no gradient to receive: those may be null
        if ((a.n_v2p > 0 && !a.order_v2p) || (a.n_p2v > 0 && !a.order_p2v) || (a.n_vtx > 0 && !a.grad_vtx) || (a.n_pts > 0 && !a.grad_pts))
            return MORIG_E_INVALID;
        if (a.ld_gv < NCE_C || a.ld_gp < NCE_C || !al16(a.d_rows) || !al16(a.d_key_pts) || !al16(a.d_key_vtx)) return MORIG_E_INVALID;
    }
    p.d[0] = NceDir{a.vtx, a.ld_vtx, a.ptr_vtx, a.pts, a.ld_pts, a.ptr_pts, reinterpret_cast<const long long*>(a.corr_v2p), a.ptr_v2p, 0, a.d_key_pts};
    p.d[1] = NceDir{a.pts, a.ld_pts, a.ptr_pts, a.vtx, a.ld_vtx, a.ptr_vtx, reinterpret_cast<const long long*>(a.corr_p2v), a.ptr_p2v, a.n_v2p, a.d_key_vtx};
    p.B = a.n_pairs; p.tau = a.tau;
    p.lse = a.lse; p.row_loss = a.row_loss; p.loss = a.loss; p.upstream = a.upstream; p.d_rows = a.d_rows; p.status = a.status;
    return MORIG_OK;
}

extern "C" int morig_infonce_forward(const morig_nce_args* args, void* stream) {
    morig_nce_args a; NceParams p;
    const int st = nce_params(args, false, a, p);
    if (st != MORIG_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int max_rows = a.n_v2p > a.n_p2v ? a.n_v2p : a.n_p2v;
    {
        ProfScope ps(K_LOSS_NCE_FWD, s, 2.0 * NCE_C * ((double)a.n_v2p * a.n_pts + (double)a.n_p2v * a.n_vtx) / a.n_pairs, 0.0);
        if (max_rows > 0) hipLaunchKernelGGL(nce_fwd_kernel, dim3(cdiv(max_rows, 128), a.n_pairs, 2), dim3(256), 0, s, p);
        MORIG_LAUNCH_CHECK();
    }
    ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
    hipLaunchKernelGGL(nce_reduce_kernel, dim3(1), dim3(256), 0, s, p);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_infonce_backward(const morig_nce_args* args, void* stream) {
    morig_nce_args a; NceParams p;
    const int st = nce_params(args, true, a, p);
    if (st != MORIG_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int max_rows = a.n_v2p > a.n_p2v ? a.n_v2p : a.n_p2v, max_keys = a.n_vtx > a.n_pts ? a.n_vtx : a.n_pts;
    {
        ProfScope ps(K_LOSS_NCE_BWD, s, 8.0 * NCE_C * ((double)a.n_v2p * a.n_pts + (double)a.n_p2v * a.n_vtx) / a.n_pairs, 0.0);
        if (max_rows > 0) hipLaunchKernelGGL(nce_bwd_kernel<true>, dim3(cdiv(max_rows, 128), a.n_pairs, 2), dim3(256), 0, s, p);
        if (max_keys > 0) hipLaunchKernelGGL(nce_bwd_kernel<false>, dim3(cdiv(max_keys, 128), a.n_pairs, 2), dim3(256), 0, s, p);
        MORIG_LAUNCH_CHECK();
    }
    ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
    if (a.n_vtx > 0)
        hipLaunchKernelGGL(nce_combine_kernel, dim3(cdiv((long)a.n_vtx * 16, 256)), dim3(256), 0, s, a.d_rows, a.rowptr_vtx, a.order_v2p,
                           a.d_key_vtx, a.n_vtx, a.grad_vtx, a.ld_gv);
    if (a.n_pts > 0)
        hipLaunchKernelGGL(nce_combine_kernel, dim3(cdiv((long)a.n_pts * 16, 256)), dim3(256), 0, s, a.d_rows + (size_t)a.n_v2p * NCE_C,
                           a.rowptr_pts, a.order_p2v, a.d_key_pts, a.n_pts, a.grad_pts, a.ld_gp);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

static int multipos_check(const float* F, int ldf, int D, const int32_t* pos, int n_pos, const int32_t* neg, int n_neg, int n_meshes, int S) {
    if (!F || !pos || !neg || n_meshes <= 0 || S <= 0) return MORIG_E_INVALID;
    if (D < 4 || D > 128 || (D & 3) || n_pos < 1 || n_pos > MP_MAX_POS || n_neg < 0 || n_neg > MP_MAX_NEG) return MORIG_E_UNSUPPORTED;
    if (ldf < D || (ldf & 3) || !al16(F)) return MORIG_E_INVALID;
    if ((long)n_meshes * S > 0x7fffffffL / (S > 128 ? S : 128)) return MORIG_E_UNSUPPORTED;
    return MORIG_OK;
}

extern "C" int morig_multipos_forward(const float* F, int32_t ldf, int32_t D, const int32_t* pos_ids, int32_t n_pos, const int32_t* neg_ids,
                                      int32_t n_neg, int32_t n_meshes, int32_t n_sample, float* neg_max, float* neg_sum, float* row_loss,
                                      float* loss, int32_t* status, void* stream) {
    const int st = multipos_check(F, ldf, D, pos_ids, n_pos, neg_ids, n_neg, n_meshes, n_sample);
    if (st != MORIG_OK) return st;
    if (!neg_max || !neg_sum || !row_loss || !loss || !status) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_rows = n_meshes * n_sample;
    {
        ProfScope ps(K_LOSS_MULTIPOS, s, 2.0 * D * (n_pos + n_neg) * (double)n_rows, 0.0);
        hipLaunchKernelGGL(multipos_fwd_kernel, dim3(cdiv(n_rows, 4)), dim3(256), 0, s, F, ldf, D, pos_ids, n_pos, neg_ids, n_neg, n_sample,
                           n_rows, neg_max, neg_sum, row_loss, status);
        MORIG_LAUNCH_CHECK();
    }
    ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, row_loss, n_rows, 1.0 / (double)n_rows, loss, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_multipos_backward(const float* F, int32_t ldf, int32_t D, const int32_t* pos_ids, int32_t n_pos, const int32_t* neg_ids,
                                       int32_t n_neg, int32_t n_meshes, int32_t n_sample, const float* neg_max, const float* neg_sum,
                                       const float* upstream, float* G, const int32_t* rows, float* grad, int32_t ld_grad, int32_t* status,
                                       void* stream) {
    const int st = multipos_check(F, ldf, D, pos_ids, n_pos, neg_ids, n_neg, n_meshes, n_sample);
    if (st != MORIG_OK) return st;
    if (!neg_max || !neg_sum || !upstream || !G || !rows || !grad || !status || ld_grad < D) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n_rows = n_meshes * n_sample;
    ProfScope ps(K_LOSS_MULTIPOS, s, 2.0 * D * (n_pos + n_neg) * (double)n_rows + 2.0 * D * (double)n_rows * n_sample, 0.0);
    hipLaunchKernelGGL(multipos_g_kernel, dim3(n_rows), dim3(256), 0, s, F, ldf, D, pos_ids, n_pos, neg_ids, n_neg, n_sample, n_rows, neg_max,
                       neg_sum, upstream, G, status);
    hipLaunchKernelGGL(multipos_apply_kernel, dim3(cdiv(n_sample, 64), n_meshes), dim3(256), 0, s, G, F, ldf, D, n_sample, rows, grad, ld_grad);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_chamfer_forward(const float* p, const float* q, const int32_t* ptr_p, const int32_t* ptr_q, int32_t n_meshes, int32_t n_p,
                                     int32_t n_q, int32_t* arg1, float* d1, uint64_t* key2, float* loss, int32_t* status, void* stream) {
    if (!p || !q || !ptr_p || !ptr_q || !arg1 || !d1 || !key2 || !loss || !status || n_meshes <= 0 || n_p <= 0 || n_q <= 0) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_LOSS_CHAMFER, s, 0.0, 0.0);
    MORIG_HIP_TRY(hipMemsetAsync(key2, 0xff, sizeof(uint64_t) * (size_t)n_q, s));
    hipLaunchKernelGGL(chamfer_fwd_kernel, dim3(cdiv(n_p, 256), n_meshes), dim3(256), 0, s, p, q, ptr_p, ptr_q, arg1, d1,
                       reinterpret_cast<u64*>(key2), status);
    hipLaunchKernelGGL(chamfer_reduce_kernel, dim3(1), dim3(256), 0, s, d1, reinterpret_cast<const u64*>(key2), ptr_p, ptr_q, n_meshes, loss, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_chamfer_backward(const float* p, const float* q, const int32_t* ptr_p, const int32_t* ptr_q, int32_t n_meshes, int32_t n_p,
                                      int32_t n_q, const int32_t* arg1, const float* d1, const uint64_t* key2, const float* upstream, float* grad_p,
                                      float* grad_q, const int32_t* status, void* stream) {
    if (!p || !q || !ptr_p || !ptr_q || !arg1 || !d1 || !key2 || !upstream || !grad_p || !grad_q || !status || n_meshes <= 0 || n_p <= 0 || n_q <= 0)
        return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_LOSS_CHAMFER, s, 0.0, 0.0);
    hipLaunchKernelGGL(chamfer_bwd_p_kernel, dim3(cdiv(n_p, 256), n_meshes), dim3(256), 0, s, p, q, ptr_p, ptr_q, n_meshes, arg1, d1,
                       reinterpret_cast<const u64*>(key2), upstream, grad_p, status);
    hipLaunchKernelGGL(chamfer_bwd_q_kernel, dim3(n_meshes), dim3(256), 0, s, p, q, ptr_p, ptr_q, n_meshes, arg1, d1,
                       reinterpret_cast<const u64*>(key2), upstream, grad_q, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
