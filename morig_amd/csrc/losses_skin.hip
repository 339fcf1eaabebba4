// The losses of training/train_skin.py: log_ratio_loss (models/customized_losses.py:11-44), the masked soft-label cross-entropy of
// train_skin.py:168-174 and cross_entropy_with_probs (:216-228), forward and backward. As in losses.hip there is no floating-point atomic:
// every sum runs in a fixed order and two runs give the same bits.
//
// log-ratio    The reference expands the S = 50 sampled rows of a mesh into all n = S (S - 1) / 2 pairs and forms n x n tables of pair
//              distances. Every entry of those tables is an entry of ONE S x S table: with L[i][j] = log(|f_i - f_j|^2 + eps) -
//              log(|g_i - g_j|^2 + eps) and pairs p = (a_p, b_p), a < b, in lexicographic order, the loss of the mesh is
//                  (1 / (n (n - 1) / 2)) sum_{p < q} (L[a_q][b_p] - L[a_p][b_q])^2.
//              One workgroup per (mesh, feature set): the sampled rows go to LDS, the table is built there in difference form (never
//              |a|^2 + |b|^2 - 2ab: 1 / (dist + eps) amplifies its cancellation), and the 750 000 terms are read from LDS. The table and
//              the feature distances (2 x S x S floats) are kept for the backward, where the thread that OWNS L[i][j] gathers every term
//              that entry takes part in; d f_i = 2 sum_{j != i} (f_i - f_j) (M[i][j] + M[j][i]), M = dL / (dist + eps), the diagonal
//              skipped: M[i][i] is of the order 1 / eps and multiplies an exact zero only in this form.
// skin CE      one thread per vertex; the label sums that decide vert_mask run in index order in plain float32 (no contraction: the mask
//              is an exact-equality test on a rounded sum); numerator and denominator per workgroup in float64,
//              then one workgroup adds the partials in order.
#include "common.h"

namespace morig {

namespace {

constexpr int ST_INDEX = MORIG_LOSS_ST_INDEX;
constexpr int ST_FATAL = MORIG_LOSS_ST_UNSORTED | MORIG_LOSS_ST_SEGMENT;
constexpr int LR_MAX_S = MORIG_LOGRATIO_MAX_SAMPLE;            // 64
constexpr int LR_MAX_W = MORIG_LOGRATIO_MAX_WIDTH;             // 128
constexpr int LR_LD = LR_MAX_W + 4;                            // LDS row stride of the gathered rows (floats; 16-byte aligned rows)
constexpr int LR_TS = LR_MAX_S + 1;                            // LDS row stride of the S x S table
constexpr int LR_MAX_PAIRS = LR_MAX_S * (LR_MAX_S - 1) / 2;
constexpr float LR_EPS = 1e-6f;
constexpr int CE_MAX_K = MORIG_SKIN_CE_MAX_K;                  // 8
constexpr int CEP_MAX_K = MORIG_CE_PROBS_MAX_K;                // 128


struct LrParams {
    const float* feat_all; long ld_all; long set_stride; int n_all;     // set t < n_all: rows of feat_all + t * set_stride
    const float* feat_aggr; long ld_aggr;                               // set n_all (when n_sets == n_all + 1)
    const float* gt; long ld_gt;
    const int* ptr; const int* samples;                                 // [B + 1]; [n_sets][B][S] ids local to the mesh
    int B, S, D, W, n_sets, n_rows;
    int vec_all, vec_aggr, vec_gt;                                      // 16-byte loads allowed
    float* tab;                                                         // [n_sets][B][2][S][S]: L, feature distances
    double* wg_loss;                                                    // [n_sets][B]
    float* loss; const float* upstream;
    float* grad_all; long ldg_all; long gset_stride; float* grad_aggr; long ldg_aggr;
    int* status;
};

// the global rows of the mesh's samples; an id outside the mesh sets ST_INDEX and is clamped, a repeated one sets ST_INDEX
// (its gradient row would be stored twice). Returns false for a mesh without vertices; s_row is visible to the workgroup on return.
__device__ __forceinline__ bool lr_rows(const LrParams& p, int b, int set, int* s_row, bool flag) {
    const int v0 = p.ptr[b], cnt = p.ptr[b + 1] - v0;
    if (cnt <= 0 || v0 < 0 || v0 + cnt > p.n_rows) return false;        // block-uniform
    const int tid = threadIdx.x;
    if (tid < p.S) {
        int id = p.samples[((size_t)set * p.B + b) * p.S + tid];
        if (id < 0 || id >= cnt) { if (flag) atomicOr(p.status, ST_INDEX); id = id < 0 ? 0 : cnt - 1; }
        s_row[tid] = v0 + id;
    }
    __syncthreads();
    if (flag && tid < p.S) {
        bool dup = false;
        for (int j = 0; j < tid; ++j) dup |= s_row[j] == s_row[tid];
        if (dup) atomicOr(p.status, ST_INDEX);
    }
    return true;
}

__device__ __forceinline__ void lr_gather(const float* __restrict__ src, long ld, int width, bool vec, const int* s_row, int S, float* s_buf) {
    if (vec) {
        const int nq = width >> 2;
        for (int e = threadIdx.x; e < S * nq; e += 256) {
            const int i = e / nq, q = e - i * nq;
            *reinterpret_cast<f32x4*>(s_buf + i * LR_LD + 4 * q) = *reinterpret_cast<const f32x4*>(src + (size_t)s_row[i] * ld + 4 * q);
        }
    } else {
        for (int e = threadIdx.x; e < S * width; e += 256) {
            const int i = e / width, c = e - i * width;
            s_buf[i * LR_LD + c] = src[(size_t)s_row[i] * ld + c];
        }
    }
}

// sum_c (x_i[c] - x_j[c])^2, float32, channels in order; symmetric in (i, j) to the bit, exactly 0 on the diagonal
__device__ __forceinline__ float lr_dist(const float* s_buf, int i, int j, int width) {
    const float* a = s_buf + i * LR_LD;
    const float* b = s_buf + j * LR_LD;
    float s = 0.f;
    for (int c = 0; c < width; c += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(a + c), y = *reinterpret_cast<const f32x4*>(b + c);
        const float d0 = x[0] - y[0], d1 = x[1] - y[1], d2 = x[2] - y[2], d3 = x[3] - y[3];
        s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
    }
    return s;
}

__device__ __forceinline__ void lr_set(const LrParams& p, int set, const float*& f, long& ld, bool& vec) {
    if (set < p.n_all) { f = p.feat_all + (size_t)set * p.set_stride; ld = p.ld_all; vec = p.vec_all; }
    else { f = p.feat_aggr; ld = p.ld_aggr; vec = p.vec_aggr; }
}

__global__ __launch_bounds__(256) void logratio_fwd_kernel(const LrParams p) {
    __shared__ __attribute__((aligned(16))) float s_buf[LR_MAX_S * LR_LD];
    __shared__ float s_tab[LR_MAX_S * LR_TS];
    __shared__ unsigned short s_pair[LR_MAX_PAIRS];
    __shared__ double s_red[256];
    __shared__ int s_row[LR_MAX_S];
    const int b = blockIdx.x, set = blockIdx.y, tid = threadIdx.x, S = p.S;
    double* out = p.wg_loss + (size_t)set * p.B + b;
    if (*p.status & ST_FATAL) { if (tid == 0) *out = 0.0; return; }
    if (!lr_rows(p, b, set, s_row, true)) { if (tid == 0) *out = 0.0; return; }       // a mesh without vertices adds nothing
    const float* f; long ld; bool vec;
    lr_set(p, set, f, ld, vec);
    float* tab = p.tab + ((size_t)set * p.B + b) * 2 * S * S;
    lr_gather(f, ld, p.D, vec, s_row, S, s_buf);
    if (tid < S)                                             // pair (a, b), a < b, at its place in lexicographic order
        for (int k = tid + 1; k < S; ++k) s_pair[tid * (2 * S - tid - 1) / 2 + (k - tid - 1)] = (unsigned short)((tid << 8) | k);
    __syncthreads();
    for (int e = tid; e < S * S; e += 256) {
        const int i = e / S, j = e - i * S;
        const float d = lr_dist(s_buf, i, j, p.D);
        tab[S * S + e] = d;
        s_tab[i * LR_TS + j] = logf(d + LR_EPS);
    }
    __syncthreads();
    lr_gather(p.gt, p.ld_gt, p.W, p.vec_gt, s_row, S, s_buf);
    __syncthreads();
    for (int e = tid; e < S * S; e += 256) {                 // the thread that wrote the feature term of an entry completes it
        const int i = e / S, j = e - i * S;
        const float l = s_tab[i * LR_TS + j] - logf(lr_dist(s_buf, i, j, p.W) + LR_EPS);
        s_tab[i * LR_TS + j] = l;
        tab[e] = l;
    }
    __syncthreads();
    // sum over p < q: for p = (a, b) the later pairs are (a, b') with b' > b, then (a', b') with a' > a; L[a'][b] is fixed over b'.
    // p runs over the threads in a folded order (the work of a pair falls with its index); the inner sums are float32 over at most
    // S terms, everything above them float64
    const int n = S * (S - 1) / 2;
    double acc = 0.0;
    for (int base = 0, round = 0; base < n; base += 256, ++round) {
        const int pi = base + ((round & 1) ? 255 - tid : tid);
        if (pi >= n) continue;
        const int a = s_pair[pi] >> 8, bb = s_pair[pi] & 255;
        const float* row_a = s_tab + a * LR_TS;
        for (int a2 = a; a2 < S - 1; ++a2) {
            const float fixed = s_tab[a2 * LR_TS + bb];
            float part = 0.f;
            for (int b2 = (a2 == a ? bb : a2) + 1; b2 < S; ++b2) {
                const float r = fixed - row_a[b2];
                part += r * r;
            }
            acc += (double)part;
        }
    }
    acc = block_sum256(acc, s_red);
    if (tid == 0) *out = acc / (0.5 * (double)n * (double)(n - 1));
}

// loss = sum over the sets, in set order, of (sum over meshes of the workgroup results) / meshes, float64; NaN when a status bit is set
__global__ __launch_bounds__(256) void logratio_reduce_kernel(const double* __restrict__ wg_loss, int B, int n_sets, float* __restrict__ loss,
                                                              const int* __restrict__ status) {
    __shared__ double sh[256];
    if (*status) { if (threadIdx.x == 0) loss[0] = NAN; return; }
    double total = 0.0;
    for (int s = 0; s < n_sets; ++s) {
        double v = 0.0;
        for (int b = threadIdx.x; b < B; b += 256) v += wg_loss[(size_t)s * B + b];
        total += block_sum256(v, sh) / (double)B;
    }
    if (threadIdx.x == 0) loss[0] = (float)total;
}

__global__ __launch_bounds__(256) void logratio_bwd_kernel(const LrParams p) {
    __shared__ __attribute__((aligned(16))) float s_buf[LR_MAX_S * LR_LD];
    __shared__ float s_tab[LR_MAX_S * LR_TS];
    __shared__ int s_row[LR_MAX_S];
    if (*p.status) return;                                   // the loss is NaN; the gradient stays zero
    const int b = blockIdx.x, set = blockIdx.y, tid = threadIdx.x, S = p.S;
    if (!lr_rows(p, b, set, s_row, false)) return;
    const float* f; long ld; bool vec;
    lr_set(p, set, f, ld, vec);
    const float* tab = p.tab + ((size_t)set * p.B + b) * 2 * S * S;
    for (int e = tid; e < S * S; e += 256) s_tab[(e / S) * LR_TS + (e % S)] = tab[e];
    lr_gather(f, ld, p.D, vec, s_row, S, s_buf);
    __syncthreads();
    const int n = S * (S - 1) / 2;
    // d loss / d r_pq = 2 r_pq w, w = upstream / pairs of pairs; r_pq = L[a_q][b_p] - L[a_p][b_q]. The division by the number of meshes is
    // the LAST operation on a gradient row: a mesh's rows are then the bits of the mesh run alone, divided by the meshes.
    const float w = (float)(2.0 * (double)p.upstream[0] / (0.5 * (double)n * (double)(n - 1)));
    const float meshes = (float)p.B;
    constexpr int OWN = LR_MAX_S * LR_MAX_S / 256;
    float m[OWN];
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int e = tid + 256 * k;
        m[k] = 0.f;
        if (e >= S * S) continue;
        const int i = e / S, j = e - i * S;
        const float lij = s_tab[i * LR_TS + j];
        double acc = 0.0;
        // as L[a_q][b_p]: q = (i, bq), bq > i; p = (ap, j), ap < j; p < q: ap < i, or ap == i and j < bq.   r = L[i][j] - L[ap][bq]
        const int ap_end = min(j, i + 1);
        for (int ap = 0; ap < ap_end; ++ap) {
            const float* row = s_tab + ap * LR_TS;
            float part = 0.f;
            for (int bq = (ap == i ? j : i) + 1; bq < S; ++bq) part += lij - row[bq];
            acc += (double)part;
        }
        // as L[a_p][b_q]: p = (i, bp), bp > i; q = (aq, j), aq < j; p < q: i < aq, or aq == i and bp < j.   r = L[aq][bp] - L[i][j],
        // and d r / d L[i][j] = -1: the term adds L[i][j] - L[aq][bp]
        for (int aq = i; aq < j; ++aq) {
            const float* row = s_tab + aq * LR_TS;
            const int bp_end = aq == i ? j : S;
            float part = 0.f;
            for (int bp = i + 1; bp < bp_end; ++bp) part += lij - row[bp];
            acc += (double)part;
        }
        m[k] = (float)acc * w / (tab[S * S + e] + LR_EPS);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int e = tid + 256 * k;
        if (e < S * S) s_tab[(e / S) * LR_TS + (e % S)] = m[k];
    }
    __syncthreads();
    float* g; long ldg;
    if (set < p.n_all) { g = p.grad_all + (size_t)set * p.gset_stride; ldg = p.ldg_all; }
    else { g = p.grad_aggr; ldg = p.ldg_aggr; }
    const int nq = p.D >> 2;
    for (int e = tid; e < S * nq; e += 256) {
        const int i = e / nq, q = e - i * nq;
        const f32x4 fi = *reinterpret_cast<const f32x4*>(s_buf + i * LR_LD + 4 * q);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < S; ++j) {
            if (j == i) continue;
            const float c = s_tab[i * LR_TS + j] + s_tab[j * LR_TS + i];
            const f32x4 fj = *reinterpret_cast<const f32x4*>(s_buf + j * LR_LD + 4 * q);
            acc[0] = fmaf(fi[0] - fj[0], c, acc[0]); acc[1] = fmaf(fi[1] - fj[1], c, acc[1]);
            acc[2] = fmaf(fi[2] - fj[2], c, acc[2]); acc[3] = fmaf(fi[3] - fj[3], c, acc[3]);
        }
        float* o = g + (size_t)s_row[i] * ldg + 4 * q;
        o[0] = 2.f * acc[0] / meshes; o[1] = 2.f * acc[1] / meshes; o[2] = 2.f * acc[2] / meshes; o[3] = 2.f * acc[3] / meshes;
    }
}

// ===================================================================================================
// masked soft-label cross-entropy (training/train_skin.py:168-174), one thread per vertex
// ===================================================================================================
struct CeRow { float c[CE_MAX_K]; float v; float cnt; };

// g_k = label_k * mask_k; q_k = g_k / (sum |g| + 1e-8); v = |sum q - 1| < 1e-8. Both sums in index order, plain float32 adds, a correctly
// rounded division, nothing contracted or reassociated: the comparison is an equality test on a rounded sum and its outcome depends on
// the order. c_k = q_k * m_k * v, cnt = sum_k m_k * v.
__device__ __forceinline__ CeRow ce_row(const float* __restrict__ label, const float* __restrict__ mask, int K) {
#pragma clang fp contract(off)
    CeRow r;
    float g[CE_MAX_K], mk[CE_MAX_K];
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) {
        g[k] = 0.f; mk[k] = 0.f;
        if (k < K) { mk[k] = mask[k]; g[k] = label[k] * mk[k]; den = den + fabsf(g[k]); }
    }
    den = den + 1e-8f;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) {
        if (k < K) { g[k] = g[k] / den; sum = sum + g[k]; }
    }
    r.v = fabsf(sum - 1.0f) < 1e-8f ? 1.f : 0.f;
    r.cnt = 0.f;
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) {
        r.c[k] = g[k] * mk[k] * r.v;
        if (k < K) r.cnt = r.cnt + mk[k] * r.v;
    }
    return r;
}

__global__ __launch_bounds__(256) void skin_ce_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ label, int ldl,
                                                          const float* __restrict__ mask, int ldm, int n, int K, float* __restrict__ vert_mask,
                                                          double* __restrict__ part) {
    __shared__ double sh[256];
    const int v = blockIdx.x * 256 + threadIdx.x;
    double num = 0.0, den = 0.0;
    if (v < n) {
        const CeRow r = ce_row(label + (size_t)v * ldl, mask + (size_t)v * ldm, K);
        float xv[CE_MAX_K];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < CE_MAX_K; ++k) { xv[k] = k < K ? x[(size_t)v * ldx + k] : -INFINITY; mx = fmaxf(mx, xv[k]); }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < CE_MAX_K; ++k) if (k < K) se += expf(xv[k] - mx);
        const float lse = logf(se);
        float row = 0.f;
#pragma unroll
        for (int k = 0; k < CE_MAX_K; ++k) if (k < K) row += -r.c[k] * ((xv[k] - mx) - lse);
        vert_mask[v] = r.v;
        num = (double)row; den = (double)r.cnt;
    }
    num = block_sum256(num, sh);
    den = block_sum256(den, sh);
    if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = num; part[2 * (size_t)blockIdx.x + 1] = den; }
}

// sums[0 .. 1] = the partial pairs added in order; out = ratio ? sums[0] / sums[1] (0 / 0 = NaN: nothing survived the masks) : sums[0] * scale
__global__ __launch_bounds__(256) void pair_reduce_kernel(const double* __restrict__ part, int n_part, int ratio, double scale,
                                                          double* __restrict__ sums, float* __restrict__ out) {
    __shared__ double sh[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_part; i += 256) { a += part[2 * (size_t)i]; b += part[2 * (size_t)i + 1]; }
    a = block_sum256(a, sh);
    b = block_sum256(b, sh);
    if (threadIdx.x == 0) {
        sums[0] = a; sums[1] = b;
        out[0] = ratio ? (float)(a / b) : (float)(a * scale);
    }
}

// d x_j = (upstream / den) (softmax_j sum_k c_k - c_j)
__global__ __launch_bounds__(256) void skin_ce_bwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ label, int ldl,
                                                          const float* __restrict__ mask, int ldm, int n, int K, const double* __restrict__ sums,
                                                          const float* __restrict__ upstream, float* __restrict__ grad) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const CeRow r = ce_row(label + (size_t)v * ldl, mask + (size_t)v * ldm, K);
    const float coef = (float)((double)upstream[0] / sums[1]);
    float xv[CE_MAX_K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) { xv[k] = k < K ? x[(size_t)v * ldx + k] : -INFINITY; mx = fmaxf(mx, xv[k]); }
    float se = 0.f, sc = 0.f;
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) if (k < K) { se += expf(xv[k] - mx); sc += r.c[k]; }
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) if (k < K) grad[(size_t)v * K + k] = coef * (expf(xv[k] - mx) / se * sc - r.c[k]);
}

// ===================================================================================================
// cross_entropy_with_probs (models/customized_losses.py:216-228): cum[v][k] = -target * log_softmax(input) (* weight); one thread per row
// ===================================================================================================
__global__ __launch_bounds__(256) void ce_probs_fwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ w,
                                                           int n, int K, float* __restrict__ cum, double* __restrict__ part) {
    __shared__ double sh[256];
    const int v = blockIdx.x * 256 + threadIdx.x;
    double rowsum = 0.0;
    if (v < n) {
        const float* xr = x + (size_t)v * K;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, xr[k]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(xr[k] - mx);
        const float lse = logf(se);
        float row = 0.f;
        for (int k = 0; k < K; ++k) {
            float c = -t[(size_t)v * K + k] * ((xr[k] - mx) - lse);
            if (w) c *= w[(size_t)v * K + k];
            if (cum) cum[(size_t)v * K + k] = c;
            row += c;
        }
        rowsum = (double)row;
    }
    if (part) {
        rowsum = block_sum256(rowsum, sh);
        if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = rowsum; part[2 * (size_t)blockIdx.x + 1] = 0.0; }
    }
}

// u_k = upstream of cum[v][k] (per_elem: up[v][k], else up[0] * scale); d x_j = softmax_j sum_k u_k t_k w_k - u_j t_j w_j
__global__ __launch_bounds__(256) void ce_probs_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ w,
                                                           int n, int K, const float* __restrict__ up, int per_elem, float scale,
                                                           float* __restrict__ grad) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float* xr = x + (size_t)v * K;
    const float u0 = per_elem ? 0.f : up[0] * scale;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, xr[k]);
    float se = 0.f, sc = 0.f;
    for (int k = 0; k < K; ++k) {
        se += expf(xr[k] - mx);
        float c = (per_elem ? up[(size_t)v * K + k] : u0) * t[(size_t)v * K + k];
        if (w) c *= w[(size_t)v * K + k];
        sc += c;
    }
    for (int k = 0; k < K; ++k) {
        float c = (per_elem ? up[(size_t)v * K + k] : u0) * t[(size_t)v * K + k];
        if (w) c *= w[(size_t)v * K + k];
        grad[(size_t)v * K + k] = expf(xr[k] - mx) / se * sc - c;
    }
}

}  // namespace

}  // namespace morig

using namespace morig;

static_assert(sizeof(morig_logratio_args) == MORIG_LOGRATIO_STRUCT_BYTES, "include/morig_hip.h states the size");

static int logratio_params(const morig_logratio_args* args, bool backward, morig_logratio_args& a, LrParams& p) {
    if (!take_args(args, a, MORIG_LOGRATIO_STRUCT_BYTES)) return MORIG_E_INVALID;
    if (a.n_meshes <= 0 || a.n_rows <= 0 || a.n_sets <= 0 || a.n_all < 0 || (a.n_sets != a.n_all && a.n_sets != a.n_all + 1)) return MORIG_E_INVALID;
    if (a.n_sample < 3 || a.n_sample > LR_MAX_S || a.D < 4 || a.D > LR_MAX_W || (a.D & 3) || a.W < 4 || a.W > LR_MAX_W || (a.W & 3))
        return MORIG_E_UNSUPPORTED;
    if ((long)a.n_sets * a.n_meshes > 0x7fffffffL / (2 * a.n_sample * a.n_sample) || a.n_sets > 65535) return MORIG_E_UNSUPPORTED;
    const bool has_aggr = a.n_sets == a.n_all + 1;
    if (!a.gt || !a.ptr || !a.samples || !a.tab || !a.wg_loss || !a.status || (a.n_all > 0 && !a.feat_all) || (has_aggr && !a.feat_aggr))
        return MORIG_E_INVALID;
    if (a.ld_gt < a.W || (a.n_all > 0 && (a.ld_all < a.D || a.set_stride < 0)) || (has_aggr && a.ld_aggr < a.D)) return MORIG_E_INVALID;
    if (!backward && !a.loss) return MORIG_E_INVALID;
    if (backward) {
        if (!a.upstream || (a.n_all > 0 && (!a.grad_all || a.ldg_all < a.D || a.gset_stride < 0)) || (has_aggr && (!a.grad_aggr || a.ldg_aggr < a.D)))
            return MORIG_E_INVALID;
    }
    p.feat_all = a.feat_all; p.ld_all = a.ld_all; p.set_stride = a.set_stride; p.n_all = a.n_all;
    p.feat_aggr = a.feat_aggr; p.ld_aggr = a.ld_aggr; p.gt = a.gt; p.ld_gt = a.ld_gt;
    p.ptr = a.ptr; p.samples = a.samples;
    p.B = a.n_meshes; p.S = a.n_sample; p.D = a.D; p.W = a.W; p.n_sets = a.n_sets; p.n_rows = a.n_rows;
    p.vec_all = a.n_all > 0 && vec4_ptr(a.feat_all, a.ld_all) && (a.set_stride & 3) == 0;
    p.vec_aggr = has_aggr && vec4_ptr(a.feat_aggr, a.ld_aggr);
    p.vec_gt = vec4_ptr(a.gt, a.ld_gt);
    p.tab = a.tab; p.wg_loss = a.wg_loss; p.loss = a.loss; p.upstream = a.upstream;
    p.grad_all = a.grad_all; p.ldg_all = a.ldg_all; p.gset_stride = a.gset_stride; p.grad_aggr = a.grad_aggr; p.ldg_aggr = a.ldg_aggr;
    p.status = a.status;
    return MORIG_OK;
}

extern "C" int morig_logratio_forward(const morig_logratio_args* args, void* stream) {
    morig_logratio_args a; LrParams p;
    const int st = logratio_params(args, false, a, p);
    if (st != MORIG_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    {
        const double n = 0.5 * a.n_sample * (a.n_sample - 1);
        ProfScope ps(K_LOSS_LOGRATIO, s, 1.5 * n * (n - 1) * (double)a.n_meshes * a.n_sets, 0.0);
        hipLaunchKernelGGL(logratio_fwd_kernel, dim3(a.n_meshes, a.n_sets), dim3(256), 0, s, p);
        MORIG_LAUNCH_CHECK();
    }
    ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
    hipLaunchKernelGGL(logratio_reduce_kernel, dim3(1), dim3(256), 0, s, a.wg_loss, a.n_meshes, a.n_sets, a.loss, a.status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_logratio_backward(const morig_logratio_args* args, void* stream) {
    morig_logratio_args a; LrParams p;
    const int st = logratio_params(args, true, a, p);
    if (st != MORIG_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double n = 0.5 * a.n_sample * (a.n_sample - 1);
    ProfScope ps(K_LOSS_LOGRATIO, s, 1.0 * n * (n - 1) * (double)a.n_meshes * a.n_sets, 0.0);
    hipLaunchKernelGGL(logratio_bwd_kernel, dim3(a.n_meshes, a.n_sets), dim3(256), 0, s, p);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

static int skin_ce_check(const float* x, int ldx, const float* label, int ldl, const float* mask, int ldm, int n, int K) {
    if (!x || !label || !mask || n <= 0) return MORIG_E_INVALID;
    if (K < 1 || K > CE_MAX_K) return MORIG_E_UNSUPPORTED;
    if (ldx < K || ldl < K || ldm < K) return MORIG_E_INVALID;
    return MORIG_OK;
}

extern "C" int morig_skin_ce_forward(const float* x, int32_t ldx, const float* label, int32_t ld_label, const float* mask, int32_t ld_mask,
                                     int32_t n, int32_t K, float* vert_mask, double* part, double* sums, float* loss, void* stream) {
    const int st = skin_ce_check(x, ldx, label, ld_label, mask, ld_mask, n, K);
    if (st != MORIG_OK) return st;
    if (!vert_mask || !part || !sums || !loss) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nb = cdiv(n, 256);
    {
        ProfScope ps(K_LOSS_SKIN_CE, s, 0.0, 4.0 * 3 * K * (double)n);
        hipLaunchKernelGGL(skin_ce_fwd_kernel, dim3(nb), dim3(256), 0, s, x, ldx, label, ld_label, mask, ld_mask, n, K, vert_mask, part);
        MORIG_LAUNCH_CHECK();
    }
    ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
    hipLaunchKernelGGL(pair_reduce_kernel, dim3(1), dim3(256), 0, s, part, nb, 1, 1.0, sums, loss);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skin_ce_backward(const float* x, int32_t ldx, const float* label, int32_t ld_label, const float* mask, int32_t ld_mask,
                                      int32_t n, int32_t K, const double* sums, const float* upstream, float* grad, void* stream) {
    const int st = skin_ce_check(x, ldx, label, ld_label, mask, ld_mask, n, K);
    if (st != MORIG_OK) return st;
    if (!sums || !upstream || !grad) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_LOSS_SKIN_CE, s, 0.0, 4.0 * 4 * K * (double)n);
    hipLaunchKernelGGL(skin_ce_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, x, ldx, label, ld_label, mask, ld_mask, n, K, sums, upstream, grad);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_ce_probs_forward(const float* x, const float* target, const float* weight, int32_t n, int32_t K, int32_t reduction,
                                      float* cum, double* part, double* sums, float* loss, void* stream) {
    if (!x || !target || n <= 0 || reduction < 0 || reduction > 2) return MORIG_E_INVALID;
    if (K < 1 || K > CEP_MAX_K) return MORIG_E_UNSUPPORTED;
    if (reduction == 0 ? !cum : (!part || !sums || !loss)) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nb = cdiv(n, 256);
    {
        ProfScope ps(K_LOSS_SKIN_CE, s, 0.0, 4.0 * 3 * K * (double)n);
        hipLaunchKernelGGL(ce_probs_fwd_kernel, dim3(nb), dim3(256), 0, s, x, target, weight, n, K, reduction == 0 ? cum : nullptr,
                           reduction == 0 ? nullptr : part);
        MORIG_LAUNCH_CHECK();
    }
    if (reduction != 0) {
        ProfScope ps(K_LOSS_REDUCE, s, 0.0, 0.0);
        hipLaunchKernelGGL(pair_reduce_kernel, dim3(1), dim3(256), 0, s, part, nb, 0, reduction == 1 ? 1.0 / (double)n : 1.0, sums, loss);
        MORIG_LAUNCH_CHECK();
    }
    return MORIG_OK;
}

extern "C" int morig_ce_probs_backward(const float* x, const float* target, const float* weight, int32_t n, int32_t K, int32_t reduction,
                                       const float* upstream, float* grad, void* stream) {
    if (!x || !target || !upstream || !grad || n <= 0 || reduction < 0 || reduction > 2) return MORIG_E_INVALID;
    if (K < 1 || K > CEP_MAX_K) return MORIG_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_LOSS_SKIN_CE, s, 0.0, 4.0 * 4 * K * (double)n);
    hipLaunchKernelGGL(ce_probs_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, x, target, weight, n, K, upstream, reduction == 0 ? 1 : 0,
                       reduction == 1 ? 1.f / (float)n : 1.f, grad);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
