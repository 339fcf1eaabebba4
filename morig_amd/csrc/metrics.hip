// Rig evaluation metrics: what evaluate/eval_rigging.py:107-131 and utils/eval_utils.py:72-119 report, batched over the meshes of a batch.
// Everything is float64 (the reference computes these in numpy float64), ragged through ptr arrays, without floating-point atomics: two
// runs give the same bits.
//
// bone samples   one thread per bone for the counts, one per sample for the points; np.round is rint (half to even), the length is
//                sqrt((dx^2 + dy^2) + dz^2), a sample is p + (ray / (n + 1e-30)) * k: a multiply, then an add.
// nearest        one thread per source row; a workgroup takes 256 consecutive rows of a, walks the meshes they belong to and streams each
//                mesh's b through LDS in tiles of MORIG_NEAREST_TILE rows. Serves CD-J2J, CD-J2B and CD-B2B. A NaN squared distance among a
//                row's candidates (a NaN coordinate on either side) makes its result NaN, as np.min does.
// segment mean   one workgroup per mesh: strided partial sums, then a fixed tree.
// assignment     one wave per mesh runs csrc/assign_core.h; the cost matrix is written to the global workspace in the solver's orientation
//                and copied to LDS when it has at most AS_LDS_COST entries (the solver reads it through one flat pointer either way).
// joint scores   one wave per mesh; hits are counted in integers.
#include "common.h"
#include "assign_core.h"

// indices, counts and bit-for-bit comparisons depend on every value below: products and sums round separately, as numpy does
#pragma clang fp contract(off)

namespace morig {

namespace {

constexpr int NT = MORIG_NEAREST_TILE;
constexpr int AS_LDS_COST = 6144;                               // doubles: 48 KiB of the 64 KiB a workgroup may declare
constexpr int AS_SMALL = MORIG_ASSIGN_MAX_SMALL, AS_LARGE = MORIG_ASSIGN_MAX_LARGE;
static_assert(AS_SMALL == morig_assign::MAX_SMALL && AS_LARGE == morig_assign::MAX_LARGE, "include/morig_hip.h states assign_core.h's limits");
static_assert(AS_LARGE <= 0xffff, "morig_assign::Best keeps the column in 16 bits");

__device__ __forceinline__ double sqdist3d(const double* a, double bx, double by, double bz) {
    const double dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- bone samples ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bone_steps(const double* p, const double* c) {
    const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
    return rint(sqrt((dx * dx + dy * dy) + dz * dz) / 0.005);
}

__global__ __launch_bounds__(256) void bone_count_kernel(const double* __restrict__ joints, int n_joints, const int* __restrict__ bones,
                                                         int n_bones, long long* __restrict__ counts) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_bones) return;
    const int pi = bones[2 * b], ci = bones[2 * b + 1];
    long long n = 0;
    if (pi >= 0 && pi < n_joints && ci >= 0 && ci < n_joints) {
        const double steps = bone_steps(joints + 3 * (size_t)pi, joints + 3 * (size_t)ci);
        if (steps >= 0.0 && steps < (double)MORIG_BONE_MAX_SAMPLES) n = (long long)steps + 1;           // NaN fails both
    }
    counts[b] = n;
}

__global__ __launch_bounds__(256) void bone_sample_kernel(const double* __restrict__ joints, int n_joints, const int* __restrict__ bones,
                                                          const long long* __restrict__ off, int n_bones, long long n_samples,
                                                          double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_samples) return;
    const int lo = segment_of(off, n_bones, e);                // the last bone with off[bone] <= e
    const int pi = bones[2 * lo], ci = bones[2 * lo + 1];
    const double nan = __builtin_nan("");
    double x = nan, y = nan, z = nan;
    if (pi >= 0 && pi < n_joints && ci >= 0 && ci < n_joints && off[lo] <= e && e < off[lo + 1]) {
        const double* p = joints + 3 * (size_t)pi;
        const double* c = joints + 3 * (size_t)ci;
        const double n = bone_steps(p, c) + 1e-30, k = (double)(e - off[lo]);
        const double ux = (c[0] - p[0]) / n, uy = (c[1] - p[1]) / n, uz = (c[2] - p[2]) / n;
        x = p[0] + ux * k; y = p[1] + uy * k; z = p[2] + uz * k;
    }
    out[3 * e] = x; out[3 * e + 1] = y; out[3 * e + 2] = z;
}

// ---- nearest distance -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nearest_kernel(const double* __restrict__ a, const int* __restrict__ a_ptr, int n_a,
                                                      const double* __restrict__ b, const int* __restrict__ b_ptr, int n_b, int n_meshes,
                                                      int squared, double* __restrict__ out, int* __restrict__ flags) {
    __shared__ double s_b[NT * 3];
    const int tid = threadIdx.x, first = blockIdx.x * 256, i = first + tid;
    const int last = min(first + 255, n_a - 1);
    const int m_lo = segment_of(a_ptr, n_meshes, first), m_hi = segment_of(a_ptr, n_meshes, last);       // block-uniform
    int mine = -1;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (i < n_a) {
        const int m = segment_of(a_ptr, n_meshes, i);
        if (a_ptr[m] <= i && i < a_ptr[m + 1]) mine = m;
        ax = a[3 * (size_t)i]; ay = a[3 * (size_t)i + 1]; az = a[3 * (size_t)i + 2];
    }
    const double nan = __builtin_nan("");
    double result = nan;
    for (int m = m_lo; m <= m_hi; ++m) {                       // block-uniform bounds: the barriers below are met by every thread
        if (!__syncthreads_or(mine == m)) continue;              // (a ptr that starts past row 0 leaves blocks without a mesh)
        const int q0 = b_ptr[m], q1 = b_ptr[m + 1];
        if (q0 < 0 || q1 > n_b || q1 <= q0) {                   // no rows of b (or a ptr that leaves b): flag, no number
            if (mine == m) flags[m] = 1;
            continue;
        }
        double best = __builtin_huge_val();
        bool saw_nan = false;                                    // np.min's rule: one NaN among the candidates and the minimum is NaN
        for (int t0 = q0; t0 < q1; t0 += NT) {
            const int cnt = min(NT, q1 - t0);
            __syncthreads();
            for (int e = tid; e < cnt * 3; e += 256) s_b[e] = b[3 * (size_t)t0 + e];
            __syncthreads();
            if (mine == m)
                for (int k = 0; k < cnt; ++k) {
                    const double d = sqdist3d(s_b + 3 * k, ax, ay, az);
                    best = d < best ? d : best;
                    saw_nan = saw_nan || d != d;
                }
        }
        if (mine == m) result = saw_nan ? nan : (squared ? best : sqrt(best));
    }
    if (i < n_a) out[i] = result;
}

// ---- per-mesh mean ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segment_mean_kernel(const double* __restrict__ x, const int* __restrict__ ptr, int n,
                                                           double* __restrict__ out) {
    __shared__ double sh[256];
    const int m = blockIdx.x, tid = threadIdx.x;
    int s = ptr[m], e = ptr[m + 1];
    if (s < 0 || e > n || e < s) e = s = 0;
    double acc = 0.0;
    for (int i = s + tid; i < e; i += 256) acc += x[i];
    sh[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sh[tid] += sh[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[m] = sh[0] / (double)(e - s);             // no rows: 0 / 0 = NaN
}

// ---- assignment -------------------------------------------------------------------------------------------------------------------
struct WaveLanes {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int count() const { return 64; }
    __device__ void sync() const { __syncthreads(); }          // the workgroup IS the wave
    __device__ morig_assign::Best min(morig_assign::Best b) const {
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
            morig_assign::Best o;
            o.val = __shfl_xor(b.val, w, 64);
            o.key = __shfl_xor(b.key, w, 64);
            if (morig_assign::better(o, b)) b = o;
        }
        return b;
    }
};

struct AssignParams {
    const double* pred; const int* pred_ptr; int n_pred;
    const double* gt; const int* gt_ptr; int n_gt;
    const int* match_ptr; int n_match;
    double* cost; const long long* cost_off; long long n_cost;
    int* row_ind; int* col_ind; double* dist; int* status;
};

__global__ __launch_bounds__(64) void assign_kernel(const AssignParams p) {
    __shared__ double s_cost[AS_LDS_COST];
    __shared__ double s_u[AS_SMALL], s_v[AS_LARGE], s_short[AS_LARGE];
    __shared__ int s_path[AS_LARGE], s_c4r[AS_SMALL], s_r4c[AS_LARGE];
    __shared__ unsigned char s_sr[AS_SMALL], s_sc[AS_LARGE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int p0 = p.pred_ptr[b], np = p.pred_ptr[b + 1] - p0, g0 = p.gt_ptr[b], ng = p.gt_ptr[b + 1] - g0;
    const int m0 = p.match_ptr[b], nm = p.match_ptr[b + 1] - m0;
    // everything up to the solver is uniform over the wave
    if (p0 < 0 || np < 0 || p0 + np > p.n_pred || g0 < 0 || ng < 0 || g0 + ng > p.n_gt || m0 < 0 || nm < 0 || m0 + nm > p.n_match ||
        nm != (np < ng ? np : ng)) {
        if (lane == 0) p.status[b] = MORIG_ASSIGN_ST_PTR;       // nothing of this mesh can be addressed safely
        return;
    }
    const double nan = __builtin_nan("");
    const long long c0 = p.cost_off[b], c1 = p.cost_off[b + 1];
    const long long entries = (long long)ng * np;
    int refuse = 0;
    if (!morig_assign::supported(ng, np) || c0 < 0 || c1 > p.n_cost || c1 - c0 < entries) refuse = MORIG_ASSIGN_ST_SIZE;
    if (refuse || nm == 0) {
        for (int k = lane; k < nm; k += 64) { p.row_ind[m0 + k] = -1; p.col_ind[m0 + k] = -1; p.dist[m0 + k] = nan; }
        if (lane == 0) p.status[b] = refuse;
        return;
    }
    const bool tr = morig_assign::transposed(ng, np);          // rows = ground truth, columns = predictions
    const int nr = tr ? np : ng, nc = tr ? ng : np;
    const bool in_lds = nr * nc <= AS_LDS_COST;
    double* gcost = p.cost + c0;
    for (int e = lane; e < nr * nc; e += 64) {
        const int i = e / nc, j = e - i * nc;
        const int g = tr ? j : i, q = tr ? i : j;
        const double* pq = p.pred + 3 * (size_t)(p0 + q);
        const double* gg = p.gt + 3 * (size_t)(g0 + g);
        const double d = sqrt(sqdist3d(pq, gg[0], gg[1], gg[2]));
        gcost[e] = d;
        if (in_lds) s_cost[e] = d;
    }
    __syncthreads();
    morig_assign::State st = {s_u, s_v, s_short, s_path, s_c4r, s_r4c, s_sr, s_sc};
    WaveLanes L;
    const bool ok = morig_assign::solve(in_lds ? (const double*)s_cost : (const double*)gcost, nr, nc, st, L);
    if (!ok) {                                                 // a NaN or infinite joint position
        for (int k = lane; k < nm; k += 64) { p.row_ind[m0 + k] = -1; p.col_ind[m0 + k] = -1; p.dist[m0 + k] = nan; }
        if (lane == 0) p.status[b] = MORIG_ASSIGN_ST_INFEASIBLE;
        return;
    }
    morig_assign::emit(st, ng, np, p.row_ind + m0, p.col_ind + m0, L);
    __threadfence_block();
    __syncthreads();
    for (int k = lane; k < nm; k += 64) {
        const int r = p.row_ind[m0 + k], c = p.col_ind[m0 + k];
        p.dist[m0 + k] = (r >= 0 && r < ng && c >= 0 && c < np) ? gcost[morig_assign::solver_index(r, c, ng, np)] : nan;
    }
    if (lane == 0) p.status[b] = 0;
}

// ---- IoU, precision, recall -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void joint_scores_kernel(const int* __restrict__ row_ind, const double* __restrict__ dist,
                                                          const int* __restrict__ match_ptr, int n_match, const int* __restrict__ pred_ptr,
                                                          const int* __restrict__ gt_ptr, const double* __restrict__ fs,
                                                          const int* __restrict__ fs_ptr, int n_fs, int n_meshes, int* __restrict__ hits,
                                                          double* __restrict__ out) {
    __shared__ int s_hits;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) s_hits = 0;
    __syncthreads();
    int m0 = match_ptr[b], m1 = match_ptr[b + 1], f0 = fs_ptr[b], f1 = fs_ptr[b + 1];
    if (m0 < 0 || m1 > n_match || m1 < m0) m1 = m0 = 0;
    if (f0 < 0 || f1 > n_fs || f1 < f0) f1 = f0 = 0;
    int mine = 0;
    for (int k = m0 + lane; k < m1; k += 64) {
        const int r = row_ind[k];
        if (r >= 0 && r < f1 - f0 && dist[k] < fs[f0 + r]) ++mine;
    }
    if (mine) atomicAdd(&s_hits, mine);                         // integers: the order does not matter
    __syncthreads();
    if (lane == 0) {
        const int h = s_hits;
        const double np = (double)(pred_ptr[b + 1] - pred_ptr[b]), ng = (double)(gt_ptr[b + 1] - gt_ptr[b]);
        hits[b] = h;
        out[b] = (double)(2 * h) / (np + ng);
        out[n_meshes + b] = (double)h / np;
        out[2 * n_meshes + b] = (double)h / ng;
    }
}

__global__ __launch_bounds__(64) void valid_mean_kernel(const double* __restrict__ x, const int* __restrict__ valid, int n_rows, int n,
                                                        double* __restrict__ out) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    double s = 0.0;
    int cnt = 0;
    for (int i = 0; i < n; ++i)
        if (valid[i]) { s += x[(size_t)r * n + i]; ++cnt; }
    out[r] = s / (double)cnt;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_bone_sample_counts(const double* joints, int32_t n_joints, const int32_t* bones, int32_t n_bones, int64_t* counts, void* stream) {
    if (n_bones < 0 || n_joints < 0) return MORIG_E_INVALID;
    if (n_bones == 0) return MORIG_OK;
    if (!joints || !bones || !counts) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 0.0);
    bone_count_kernel<<<cdiv(n_bones, 256), 256, 0, s>>>(joints, n_joints, bones, n_bones, (long long*)counts);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_bone_samples(const double* joints, int32_t n_joints, const int32_t* bones, const int64_t* off, int32_t n_bones, int64_t n_samples,
                       double* out, void* stream) {
    if (n_bones < 0 || n_joints < 0 || n_samples < 0 || n_samples > ((int64_t)1 << 38)) return MORIG_E_INVALID;
    if (n_samples == 0) return MORIG_OK;
    if (!joints || !bones || !off || !out || n_bones == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 24.0 * (double)n_samples);
    bone_sample_kernel<<<(unsigned)((n_samples + 255) / 256), 256, 0, s>>>(joints, n_joints, bones, (const long long*)off, n_bones,
                                                                           (long long)n_samples, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_nearest_distance(const double* a, const int32_t* a_ptr, int32_t n_a, const double* b, const int32_t* b_ptr, int32_t n_b,
                           int32_t n_meshes, int32_t squared, double* out, int32_t* flags, void* stream) {
    if (n_a < 0 || n_b < 0 || n_meshes < 1 || n_a > (1 << 30) || n_b > (1 << 30)) return MORIG_E_INVALID;
    if (n_a == 0) return MORIG_OK;
    if (!a || !a_ptr || !b_ptr || !out || !flags || (n_b > 0 && !b)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 0.0);
    nearest_kernel<<<cdiv(n_a, 256), 256, 0, s>>>(a, a_ptr, n_a, b, b_ptr, n_b, n_meshes, squared, out, flags);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_segment_mean(const double* x, const int32_t* ptr, int32_t n, int32_t n_meshes, double* out, void* stream) {
    if (n < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!ptr || !out || (n > 0 && !x)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 8.0 * n);
    segment_mean_kernel<<<n_meshes, 256, 0, s>>>(x, ptr, n, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_assign_joints(const double* pred, const int32_t* pred_ptr, int32_t n_pred, const double* gt, const int32_t* gt_ptr, int32_t n_gt,
                        int32_t n_meshes, const int32_t* match_ptr, int32_t n_match, double* cost, const int64_t* cost_off, int64_t n_cost,
                        int32_t* row_ind, int32_t* col_ind, double* dist, int32_t* status, void* stream) {
    if (n_pred < 0 || n_gt < 0 || n_meshes < 0 || n_match < 0 || n_cost < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!pred_ptr || !gt_ptr || !match_ptr || !cost_off || !status) return MORIG_E_INVALID;
    if ((n_pred > 0 && !pred) || (n_gt > 0 && !gt) || (n_cost > 0 && !cost) || (n_match > 0 && (!row_ind || !col_ind || !dist)))
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 0.0);
    AssignParams p = {pred, pred_ptr, n_pred, gt, gt_ptr, n_gt, match_ptr, n_match, cost, (const long long*)cost_off, (long long)n_cost,
                      row_ind, col_ind, dist, status};
    assign_kernel<<<n_meshes, 64, 0, s>>>(p);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_joint_scores(const int32_t* row_ind, const double* dist, const int32_t* match_ptr, int32_t n_match, const int32_t* pred_ptr,
                       const int32_t* gt_ptr, const double* fs, const int32_t* fs_ptr, int32_t n_fs, int32_t n_meshes, int32_t* hits,
                       double* out, void* stream) {
    if (n_match < 0 || n_fs < 0 || n_meshes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!match_ptr || !pred_ptr || !gt_ptr || !fs_ptr || !hits || !out) return MORIG_E_INVALID;
    if ((n_match > 0 && (!row_ind || !dist)) || (n_fs > 0 && !fs)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 0.0);
    joint_scores_kernel<<<n_meshes, 64, 0, s>>>(row_ind, dist, match_ptr, n_match, pred_ptr, gt_ptr, fs, fs_ptr, n_fs, n_meshes, hits, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_valid_mean(const double* x, const int32_t* valid, int32_t n_rows, int32_t n, double* out, void* stream) {
    if (n_rows < 0 || n < 0) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!out || (n > 0 && (!x || !valid))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_METRICS, s, 0.0, 0.0);
    valid_mean_kernel<<<cdiv(n_rows, 64), 64, 0, s>>>(x, valid, n_rows, n, out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
