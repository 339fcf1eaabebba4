// Tracking without a rig (morig_amd/piecewise.py): the reference's Piecewise_RANSAC (utils/piecewise_ransac.py:12-45, :78-92) and its
// KernelKMeans (utils/kernel_kmeans.py:11-27, :40-49, :67-98) for a ragged batch. Everything is float64 with a fixed order of every
// sum and no floating-point atomics: two runs give the same bits, and a mesh alone gives the bits it gives inside a batch.
//
// vote     one wave per (problem, hypothesis). A problem is a segment with >= 4 handles; its handles are rows of the batch's vertex
//          arrays, listed in CSR form. Every lane fits the rigid motion of the hypothesis' three samples (redundantly: 64 identical
//          results, no broadcast), then the lanes stride over the handles: lane l sums the distances of handles l, l + 64, ... in that
//          order and counts those below the inlier distance; a fixed shuffle tree adds the 64 partials.
// fit      one workgroup per problem. Thread 0 replays the reference's two running selections over the hypotheses (largest count: the
//          first wins, and it must exceed 0; smallest sum: the first wins, starting from 1e10). On the refit branch the chosen
//          hypothesis is recomputed by the SAME device function, so the inlier set is the counted one bit for bit; the centroids, the
//          covariance and the translation are thread partials in index order under a fixed tree.
// apply    one thread per vertex of the batch: R v + t of its problem, or the target vertex where its segment has < 4 handles.
// kmeans   one workgroup per mesh with the whole loop inside. The centres live in LDS (embedding centres in float64 holding
//          float32-rounded values when X is float32). A cluster's mean is taken by ONE wave that walks the mesh's labels in ascending
//          vertex order (ballot per 64 vertices), lane j adding dimension j: the reference's order of additions, with no sort scratch.
#include "common.h"
#include "kabsch_core.h"

#pragma clang fp contract(off)

namespace morig {

namespace {

struct Rigid { double R[9]; double t[3]; };

__device__ __forceinline__ void load3(const double* __restrict__ a, int row, double* p) {
    p[0] = a[(size_t)row * 3]; p[1] = a[(size_t)row * 3 + 1]; p[2] = a[(size_t)row * 3 + 2];
}

// np.matmul(v, R.T) + t for one row
__device__ __forceinline__ void rigid_apply(const Rigid& g, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = ((v[0] * g.R[3 * i] + v[1] * g.R[3 * i + 1]) + v[2] * g.R[3 * i + 2]) + g.t[i];
}

// the fit to three rows (icp of the reference on src_pts[sample_id], tar_pts[sample_id])
__device__ void rigid_fit3(const double* __restrict__ src, const double* __restrict__ dst, int g0, int g1, int g2, Rigid& out) {
    double s[3][3], d[3][3], sm[3], dm[3], M[9];
    load3(src, g0, s[0]); load3(src, g1, s[1]); load3(src, g2, s[2]);
    load3(dst, g0, d[0]); load3(dst, g1, d[1]); load3(dst, g2, d[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) { sm[i] = ((s[0][i] + s[1][i]) + s[2][i]) / 3.0; dm[i] = ((d[0][i] + d[1][i]) + d[2][i]) / 3.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = ((d[0][i] - dm[i]) * (s[0][j] - sm[j]) + (d[1][i] - dm[i]) * (s[1][j] - sm[j])) + (d[2][i] - dm[i]) * (s[2][j] - sm[j]);
    morig_kabsch::rotation(M, out.R);
    out.t[0] = out.t[1] = out.t[2] = 0.0;
    double r[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rigid_apply(out, s[k], r[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) out.t[i] = (((d[0][i] - r[0][i]) + (d[1][i] - r[1][i])) + (d[2][i] - r[2][i])) / 3.0;
}

__device__ __forceinline__ double handle_dist(const Rigid& g, const double* __restrict__ src, const double* __restrict__ dst, int row) {
    double v[3], w[3], p[3];
    load3(src, row, v); load3(dst, row, w);
    rigid_apply(g, v, p);
    const double dx = p[0] - w[0], dy = p[1] - w[1], dz = p[2] - w[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// the handle range of problem p, clipped to the handle array; false when the table is not a range
__device__ __forceinline__ bool handle_range(const int* __restrict__ hptr, int p, int n_handles, int& h0, int& nh) {
    h0 = hptr[p];
    const int h1 = hptr[p + 1];
    nh = h1 - h0;
    return h0 >= 0 && h1 <= n_handles && nh >= 0;
}

// the three sampled rows of hypothesis `it`; false when a sample or a handle leaves its array
__device__ __forceinline__ bool sample_rows(const int* __restrict__ handles, const int* __restrict__ samples, int p, int it, int n_iter, int h0, int nh,
                                            int n_rows, int* g) {
    const int* s = samples + ((size_t)p * n_iter + it) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = s[k];
        if (i < 0 || i >= nh) return false;
        g[k] = handles[h0 + i];
        if (g[k] < 0 || g[k] >= n_rows) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void ransac_vote_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n_rows,
                                                          const int* __restrict__ handles, int n_handles, const int* __restrict__ hptr,
                                                          int n_problems, const int* __restrict__ samples, int n_iter, double inlier_dist,
                                                          int* __restrict__ count, double* __restrict__ dsum) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);             // wave-uniform
    if (w >= (long long)n_problems * n_iter) return;
    const int p = (int)(w / n_iter), it = (int)(w - (long long)p * n_iter);
    int h0, nh, g[3];
    const bool ok = handle_range(hptr, p, n_handles, h0, nh) && sample_rows(handles, samples, p, it, n_iter, h0, nh, n_rows, g);
    if (!ok) {                                                                     // never chosen: no inlier, no sum below 1e10
        if (lane == 0) { count[w] = 0; dsum[w] = __builtin_huge_val(); }
        return;
    }
    Rigid fit;
    rigid_fit3(src, dst, g[0], g[1], g[2], fit);
    int c = 0;
    double part = 0.0;
    for (int h = lane; h < nh; h += 64) {
        const int row = handles[h0 + h];
        if (row < 0 || row >= n_rows) continue;
        const double dd = handle_dist(fit, src, dst, row);
        c += dd < inlier_dist ? 1 : 0;
        part += dd;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { part += __shfl_down(part, o, 64); c += __shfl_down(c, o, 64); }
    if (lane == 0) { count[w] = c; dsum[w] = part; }
}

constexpr int FIT_THREADS = 256;

static_assert(FIT_THREADS == 256, "ransac_fit_kernel sums with block_sum256");

__global__ __launch_bounds__(FIT_THREADS) void ransac_fit_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n_rows,
                                                                 const int* __restrict__ handles, int n_handles, const int* __restrict__ hptr,
                                                                 int n_problems, const int* __restrict__ samples, int n_iter,
                                                                 const int* __restrict__ count, const double* __restrict__ dsum,
                                                                 double inlier_dist, double refit_share, int* __restrict__ chosen,
                                                                 int* __restrict__ best_count, int* __restrict__ flag, double* __restrict__ Rt) {
    __shared__ double sh[FIT_THREADS];
    __shared__ int pick[3];
    const int p = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        int max_inlier = 0, by_count = -1, by_sum = -1;
        double error_best = 1e10;
        for (int i = 0; i < n_iter; ++i) {
            const int c = count[(size_t)p * n_iter + i];
            const double e = dsum[(size_t)p * n_iter + i];
            if (c > max_inlier) { max_inlier = c; by_count = i; }
            if (e < error_best) { error_best = e; by_sum = i; }
        }
        pick[0] = by_count; pick[1] = by_sum; pick[2] = max_inlier;
    }
    __syncthreads();
    const int by_count = pick[0], by_sum = pick[1], max_inlier = pick[2];
    int h0, nh, g[3];
    const bool range_ok = handle_range(hptr, p, n_handles, h0, nh);
    // `len(best_inliers) > 0.35 * len(src_pts)`: an integer against a double product
    const bool refit = range_ok && by_count >= 0 && (double)max_inlier > refit_share * (double)nh;
    const int use = refit ? by_count : by_sum;
    int state = refit ? MORIG_RANSAC_REFIT : MORIG_RANSAC_SMALLEST_SUM;
    Rigid fit;
#pragma unroll
    for (int i = 0; i < 9; ++i) fit.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    fit.t[0] = fit.t[1] = fit.t[2] = 0.0;
    if (!range_ok || use < 0 || !sample_rows(handles, samples, p, use, n_iter, h0, nh, n_rows, g)) {
        state = MORIG_RANSAC_NONE;                                                 // the reference ends on R = None here
    } else {
        rigid_fit3(src, dst, g[0], g[1], g[2], fit);
    }
    if (state == MORIG_RANSAC_REFIT) {                                             // workgroup-uniform
        double n = 0.0, s[3] = {0, 0, 0}, d[3] = {0, 0, 0};
        for (int h = t; h < nh; h += FIT_THREADS) {
            const int row = handles[h0 + h];
            if (row < 0 || row >= n_rows) continue;
            if (handle_dist(fit, src, dst, row) < inlier_dist) {
                double v[3], w[3];
                load3(src, row, v); load3(dst, row, w);
                n += 1.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) { s[i] += v[i]; d[i] += w[i]; }
            }
        }
        n = block_sum256(n, sh);
        double sm[3], dm[3], M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 3; ++i) { sm[i] = block_sum256(s[i], sh) / n; dm[i] = block_sum256(d[i], sh) / n; }
        for (int h = t; h < nh; h += FIT_THREADS) {
            const int row = handles[h0 + h];
            if (row < 0 || row >= n_rows) continue;
            if (handle_dist(fit, src, dst, row) < inlier_dist) {
                double v[3], w[3];
                load3(src, row, v); load3(dst, row, w);
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) M[3 * i + j] += (w[i] - dm[i]) * (v[j] - sm[j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = block_sum256(M[i], sh);
        Rigid re;
        morig_kabsch::rotation(M, re.R);
        re.t[0] = re.t[1] = re.t[2] = 0.0;
        double ts[3] = {0, 0, 0};
        for (int h = t; h < nh; h += FIT_THREADS) {                                // the inliers of the HYPOTHESIS (fit), moved by the refit
            const int row = handles[h0 + h];
            if (row < 0 || row >= n_rows) continue;
            if (handle_dist(fit, src, dst, row) < inlier_dist) {
                double v[3], w[3], r[3];
                load3(src, row, v); load3(dst, row, w);
                rigid_apply(re, v, r);
#pragma unroll
                for (int i = 0; i < 3; ++i) ts[i] += w[i] - r[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) re.t[i] = block_sum256(ts[i], sh) / n;
        fit = re;
    }
    if (t == 0) {
        chosen[2 * p] = by_count; chosen[2 * p + 1] = by_sum;
        best_count[p] = max_inlier;
        flag[p] = state;
#pragma unroll
        for (int i = 0; i < 9; ++i) Rt[(size_t)p * 12 + i] = fit.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) Rt[(size_t)p * 12 + 9 + i] = fit.t[i];
    }
}

__global__ __launch_bounds__(256) void ransac_apply_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n_rows,
                                                           const int* __restrict__ problem_of, int n_problems, const int* __restrict__ flag,
                                                           const double* __restrict__ Rt, double* __restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int p = problem_of[v];
    double a[3], o[3];
    if (p < 0 || p >= n_problems) {                                                // a segment with < 4 handles: the target vertex
        load3(dst, v, o);
    } else {
        load3(src, v, a);
        if (flag[p] == MORIG_RANSAC_NONE) {                                        // the caller raises; the vertex stays
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
        } else {
            Rigid g;
#pragma unroll
            for (int i = 0; i < 9; ++i) g.R[i] = Rt[(size_t)p * 12 + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) g.t[i] = Rt[(size_t)p * 12 + 9 + i];
            rigid_apply(g, a, o);
        }
    }
    out[(size_t)v * 3] = o[0]; out[(size_t)v * 3 + 1] = o[1]; out[(size_t)v * 3 + 2] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------------------- k-means
constexpr int KM_THREADS = 1024, KM_WAVES = KM_THREADS / 64;

struct ArgD { double val; int idx; };

// w_euc * |v - c_euc| + max(1 - x . c_emb, 0) / 2, the dot product left to right in float64
template <class T>
__device__ __forceinline__ double km_dist(const T* __restrict__ x, const double* __restrict__ pos, const double* ce, const double* cu, int D,
                                          double w_euc) {
    const double dx = pos[0] - cu[0], dy = pos[1] - cu[1], dz = pos[2] - cu[2];
    const double euc = sqrt((dx * dx + dy * dy) + dz * dz);
    double dot = 0.0;
    for (int j = 0; j < D; ++j) dot += (double)x[j] * ce[j];
    const double emb = fmax(1.0 - dot, 0.0);
    return euc * w_euc + emb / 2.0;
}

// the best (val, idx) of the workgroup to every thread. LARGEST: greater val wins; else smaller val; the smaller idx on a tie.
template <bool LARGEST>
__device__ ArgD block_arg(ArgD mine, double* shv, int* shi) {
    __syncthreads();
    shv[threadIdx.x] = mine.val; shi[threadIdx.x] = mine.idx;
    __syncthreads();
    for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double a = shv[threadIdx.x], b = shv[threadIdx.x + h];
            const int ia = shi[threadIdx.x], ib = shi[threadIdx.x + h];
            const bool take = ib >= 0 && (ia < 0 || (LARGEST ? b > a : b < a) || (b == a && ib < ia));
            if (take) { shv[threadIdx.x] = b; shi[threadIdx.x] = ib; }
        }
        __syncthreads();
    }
    return ArgD{shv[0], shi[0]};
}

__device__ double km_block_sum(double v, double* shv) {
    __syncthreads();
    shv[threadIdx.x] = v;
    __syncthreads();
    for (int h = KM_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) shv[threadIdx.x] += shv[threadIdx.x + h];
        __syncthreads();
    }
    return shv[0];
}

// labels and the fit sum from the centres in LDS: thread partials in vertex order, then the tree. Only clusters with live[k] != 0 compete;
// COMPACT: the label is the cluster's rank among the live ones.
template <class T, bool COMPACT>
__device__ double km_assign(const T* __restrict__ X, const double* __restrict__ pos, int v0, int V, int D, int K, double w_euc, const double* cemb,
                            const double* ceuc, const int* live, int* __restrict__ label, double* shv) {
    double part = 0.0;
    for (int v = threadIdx.x; v < V; v += KM_THREADS) {
        const T* x = X + (size_t)(v0 + v) * D;
        const double* ps = pos + (size_t)(v0 + v) * 3;
        double best = 0.0;
        int arg = -1, rank = 0;
        for (int k = 0; k < K; ++k) {
            if (COMPACT && !live[k]) continue;
            const double dd = km_dist(x, ps, cemb + (size_t)k * D, ceuc + 3 * k, D, w_euc);
            if (arg < 0 || dd < best) { best = dd; arg = COMPACT ? rank : k; }
            ++rank;
        }
        label[v0 + v] = arg;
        part += best;
    }
    return km_block_sum(part, shv);
}

template <class T>
__global__ __launch_bounds__(KM_THREADS) void kmeans_kernel(const T* __restrict__ X, const double* __restrict__ pos, int n_rows, int D,
                                                            const int* __restrict__ vptr, const int* __restrict__ first, int K, int max_iter,
                                                            double w_euc, double tol, int* __restrict__ label, double* __restrict__ mind,
                                                            long long* __restrict__ out_label, int* __restrict__ seeds, int* __restrict__ info,
                                                            int* __restrict__ out_members, double* __restrict__ out_cemb, double* __restrict__ out_ceuc, double* __restrict__ out_fit) {
    extern __shared__ double cemb[];                                               // [K][D]
    __shared__ double ceuc[64 * 3];
    __shared__ double shv[KM_THREADS];
    __shared__ int shi[KM_THREADS];
    __shared__ int seed[64], members[64], live[64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int v0 = vptr[b], V = vptr[b + 1] - v0;
    int* inf = info + 4 * b;                                                       // status, iterations, kept clusters, unused
    if (v0 < 0 || V < 1 || (long long)v0 + V > n_rows) {                           // workgroup-uniform
        if (t == 0) { inf[0] = MORIG_KMEANS_BAD_MESH; inf[1] = 0; inf[2] = 0; inf[3] = 0; }
        return;
    }
    // ---- farthest-point seeds on the positions: squared distances as a left-to-right sum of three squares
    int cur = first[b];
    cur = cur < 0 ? 0 : (cur >= V ? V - 1 : cur);
    for (int k = 0; k < K; ++k) {
        if (t == 0) seed[k] = cur;
        if (k == K - 1) break;
        const double* c = pos + (size_t)(v0 + cur) * 3;
        const double cx = c[0], cy = c[1], cz = c[2];
        ArgD mine = {0.0, -1};
        for (int v = t; v < V; v += KM_THREADS) {
            const double* ps = pos + (size_t)(v0 + v) * 3;
            const double dx = cx - ps[0], dy = cy - ps[1], dz = cz - ps[2];
            double dd = (dx * dx + dy * dy) + dz * dz;
            if (k > 0) dd = fmin(mind[v0 + v], dd);
            mind[v0 + v] = dd;
            if (mine.idx < 0 || dd > mine.val) { mine.val = dd; mine.idx = v; }
        }
        cur = block_arg<true>(mine, shv, shi).idx;
    }
    __syncthreads();
    for (int i = t; i < K * D; i += KM_THREADS) cemb[i] = (double)X[(size_t)(v0 + seed[i / D]) * D + i % D];
    for (int i = t; i < K * 3; i += KM_THREADS) ceuc[i] = pos[(size_t)(v0 + seed[i / 3]) * 3 + i % 3];
    if (t < K) { seeds[(size_t)b * K + t] = seed[t]; live[t] = 1; }
    __syncthreads();
    double fit_last = km_assign<T, false>(X, pos, v0, V, D, K, w_euc, cemb, ceuc, live, label, shv);
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
        __syncthreads();                                                           // the labels of the last assignment are in global memory
        // ---- the update: wave `wave` owns clusters wave, wave + KM_WAVES, ...; nobody else reads or writes their centres in this phase
        for (int k = wave; k < K; k += KM_WAVES) {
            double acc0 = 0.0, acc1 = 0.0, accp = 0.0;                              // dimensions lane, lane + 64; position component lane < 3
            int n = 0;
            for (int c0 = 0; c0 < V; c0 += 64) {                                   // wave-uniform trip count: every lane ballots
                const int v = c0 + lane;
                unsigned long long mask = __ballot(v < V && label[v0 + v] == k);
                n += __popcll(mask);
                while (mask) {                                                     // ascending vertex order
                    const int m = c0 + __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const T* x = X + (size_t)(v0 + m) * D;
                    if (lane < D) acc0 += (double)x[lane];
                    if (lane + 64 < D) acc1 += (double)x[lane + 64];
                    if (lane < 3) accp += pos[(size_t)(v0 + m) * 3 + lane];
                }
            }
            if (n == 0) {                                                          // reseed onto the vertex nearest to the OLD centre (first on ties)
                ArgD mine = {0.0, -1};
                for (int v = lane; v < V; v += 64) {
                    const double dd = km_dist(X + (size_t)(v0 + v) * D, pos + (size_t)(v0 + v) * 3, cemb + (size_t)k * D, ceuc + 3 * k, D, w_euc);
                    if (mine.idx < 0 || dd < mine.val) { mine.val = dd; mine.idx = v; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ov = __shfl_xor(mine.val, o, 64);
                    const int oi = __shfl_xor(mine.idx, o, 64);
                    if (oi >= 0 && (mine.idx < 0 || ov < mine.val || (ov == mine.val && oi < mine.idx))) { mine.val = ov; mine.idx = oi; }
                }
                const T* x = X + (size_t)(v0 + mine.idx) * D;                       // V >= 1: some lane had a vertex
                if (lane < D) cemb[(size_t)k * D + lane] = (double)x[lane];
                if (lane + 64 < D) cemb[(size_t)k * D + lane + 64] = (double)x[lane + 64];
                if (lane < 3) ceuc[3 * k + lane] = pos[(size_t)(v0 + mine.idx) * 3 + lane];
            } else {
                const double cnt = (double)n;
                if (lane < D) cemb[(size_t)k * D + lane] = (double)(T)(acc0 / cnt);  // the centre array has X's type
                if (lane + 64 < D) cemb[(size_t)k * D + lane + 64] = (double)(T)(acc1 / cnt);
                if (lane < 3) ceuc[3 * k + lane] = accp / cnt;
            }
        }
        __syncthreads();
        const double fit_this = km_assign<T, false>(X, pos, v0, V, D, K, w_euc, cemb, ceuc, live, label, shv);
        iters = it + 1;
        const bool stop = fabs(fit_last - fit_this) < tol;
        fit_last = fit_this;                                                       // reported: the fit of the centres that are returned
        if (stop) break;                                                           // workgroup-uniform: every thread holds the same sums
    }
    __syncthreads();
    // ---- the prune: clusters with at most 8 members leave (trailing clusters past bincount's length have none)
    for (int k = wave; k < K; k += KM_WAVES) {
        int n = 0;
        for (int c0 = 0; c0 < V; c0 += 64) {
            const int v = c0 + lane;
            n += __popcll(__ballot(v < V && label[v0 + v] == k));
        }
        if (lane == 0) { members[k] = n; live[k] = n > 8 ? 1 : 0; }
    }
    __syncthreads();
    int kept = 0;
    for (int k = 0; k < K; ++k) kept += live[k];
    for (int i = t; i < K * D; i += KM_THREADS) out_cemb[(size_t)b * K * D + i] = cemb[i];
    for (int i = t; i < K * 3; i += KM_THREADS) out_ceuc[(size_t)b * K * 3 + i] = ceuc[i];
    if (t < K) seeds[(size_t)b * K + t] = seed[t];
    if (kept > 0) km_assign<T, true>(X, pos, v0, V, D, K, w_euc, cemb, ceuc, live, label, shv);
    __syncthreads();
    for (int v = t; v < V; v += KM_THREADS) out_label[v0 + v] = kept > 0 ? (long long)label[v0 + v] : -1;
    if (t == 0) {
        inf[0] = kept > 0 ? MORIG_KMEANS_OK : MORIG_KMEANS_NO_CLUSTER;
        inf[1] = iters; inf[2] = kept; inf[3] = 0;
        out_fit[b] = fit_last;
    }
    if (t < K) out_members[(size_t)b * K + t] = members[t];                         // the member counts the prune saw
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_ransac_vote(const double* src, const double* dst, int32_t n_rows, const int32_t* handles, int32_t n_handles, const int32_t* hptr,
                      int32_t n_problems, const int32_t* samples, int32_t n_iter, double inlier_dist, int32_t* count, double* dsum,
                      void* stream) {
    if (n_rows < 0 || n_handles < 0 || n_problems < 0 || n_iter < 0) return MORIG_E_INVALID;
    const long long waves = (long long)n_problems * n_iter;
    if (waves == 0) return MORIG_OK;
    if (waves > ((long long)1 << 31) - 8) return MORIG_E_INVALID;
    if (!src || !dst || !hptr || !samples || !count || !dsum || (n_handles > 0 && !handles)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RANSAC_VOTE, s, 0.0, 48.0 * (double)n_iter * n_handles);
    ransac_vote_kernel<<<(unsigned)((waves + 3) / 4), 256, 0, s>>>(src, dst, n_rows, handles, n_handles, hptr, n_problems, samples, n_iter,
                                                                   inlier_dist, count, dsum);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_ransac_fit(const double* src, const double* dst, int32_t n_rows, const int32_t* handles, int32_t n_handles, const int32_t* hptr,
                     int32_t n_problems, const int32_t* samples, int32_t n_iter, const int32_t* count, const double* dsum, double inlier_dist,
                     double refit_share, int32_t* chosen, int32_t* best_count, int32_t* flag, double* Rt, void* stream) {
    if (n_rows < 0 || n_handles < 0 || n_problems < 0 || n_iter < 0) return MORIG_E_INVALID;
    if (n_problems == 0) return MORIG_OK;
    if (!src || !dst || !hptr || !chosen || !best_count || !flag || !Rt || (n_handles > 0 && !handles)) return MORIG_E_INVALID;
    if (n_iter > 0 && (!samples || !count || !dsum)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RANSAC_FIT, s, 0.0, 144.0 * (double)n_handles);
    ransac_fit_kernel<<<n_problems, FIT_THREADS, 0, s>>>(src, dst, n_rows, handles, n_handles, hptr, n_problems, samples, n_iter, count, dsum,
                                                         inlier_dist, refit_share, chosen, best_count, flag, Rt);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_ransac_apply(const double* src, const double* dst, int32_t n_rows, const int32_t* problem_of, int32_t n_problems, const int32_t* flag,
                       const double* Rt, double* out, void* stream) {
    if (n_rows < 0 || n_problems < 0) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!src || !dst || !problem_of || !out || (n_problems > 0 && (!flag || !Rt))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RANSAC_APPLY, s, 0.0, 76.0 * (double)n_rows);
    ransac_apply_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(src, dst, n_rows, problem_of, n_problems, flag, Rt, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_kernel_kmeans(const void* X, int32_t x_is_f64, const double* pos, int32_t n_rows, int32_t D, const int32_t* vptr, int32_t n_meshes,
                        const int32_t* first, int32_t n_clusters, int32_t max_iter, double w_euc, double tol, int32_t* label_scratch,
                        double* dist_scratch, int64_t* labels, int32_t* seeds, int32_t* info, int32_t* members, double* centres_emb,
                        double* centres_euc, double* fit, void* stream) {
    if (n_rows < 0 || n_meshes < 0 || D < 1 || n_clusters < 1 || max_iter < 0) return MORIG_E_INVALID;
    if (n_clusters > MORIG_KMEANS_MAX_CLUSTERS || D > MORIG_KMEANS_MAX_DIM) return MORIG_E_UNSUPPORTED;   // before anything is launched
    if (n_meshes == 0) return MORIG_OK;
    if (!X || !pos || !vptr || !first || !label_scratch || !dist_scratch || !labels || !seeds || !info || !members || !centres_emb || !centres_euc || !fit)
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)n_clusters * D * sizeof(double);                     // <= 64 KiB beside 16 KiB of static arrays
    ProfScope ps(K_KMEANS, s, 0.0, 0.0);
    if (x_is_f64) {
        MORIG_HIP_TRY(hipFuncSetAttribute((const void*)kmeans_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kmeans_kernel<double><<<n_meshes, KM_THREADS, lds, s>>>((const double*)X, pos, n_rows, D, vptr, first, n_clusters, max_iter, w_euc, tol,
                                                                label_scratch, dist_scratch, (long long*)labels, seeds, info, members, centres_emb,
                                                                centres_euc, fit);
    } else {
        MORIG_HIP_TRY(hipFuncSetAttribute((const void*)kmeans_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kmeans_kernel<float><<<n_meshes, KM_THREADS, lds, s>>>((const float*)X, pos, n_rows, D, vptr, first, n_clusters, max_iter, w_euc, tol,
                                                               label_scratch, dist_scratch, (long long*)labels, seeds, info, members, centres_emb,
                                                               centres_euc, fit);
    }
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
