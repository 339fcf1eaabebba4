// Skeleton connection between the joint extraction and the skinning stage (evaluate/joint2rig.py:197-264): the per-pair geometry of
// create_one_data, the cost matrix of predict_skeleton with utils/mst_utils.py:269-291 (increase_cost_for_outside_bone) folded in, and
// utils/mst_utils.py:63-108 (minKey / primMST). Batched over meshes by prefix sums; pairs of a mesh are itertools.combinations order.
//
// Pair geometry: one wavefront per pair, one lane per bone sample, the counts from ballots. A pair is walked twice because the
// reference walks it twice with different number formats: create_one_data on the float64 joints, the cost loop
// on the float32 joints of the Data object (length, step count and unit step in float32, the samples themselves in float64).
// Prim: one workgroup per mesh, every joint owned by one thread (key / in-tree flag / parent in LDS), the J steps sequential, the
// arg-min a wave shuffle reduction plus one LDS exchange per step, the relaxation a coalesced read of the picked joint's cost row.
#include "common.h"

// voxel indices and step counts decide everything below: products and sums round separately, as numpy does
#pragma clang fp contract(off)

namespace morig {

constexpr int SK_VG = 88;                        // the reference's grids are 88^3 (inside_check hard-codes it)
constexpr long SK_VOXELS = (long)SK_VG * SK_VG * SK_VG;
constexpr int SK_PAIR_THREADS = 256;             // 4 pairs per workgroup
constexpr double SK_MAX_SAMPLES = 16777216.0;    // 2^24, as csrc/skin.hip
constexpr int SK_PRIM_THREADS = 256;
constexpr int SK_PRIM_SLOTS = MORIG_PRIM_MAX_JOINTS / SK_PRIM_THREADS;

// k-th pair of itertools.combinations(range(J), 2) -> (i, j), i < j; row i starts at i (2J - i - 1) / 2
__device__ __forceinline__ void pair_of(int k, int J, int& i, int& j) {
    const double t = 2.0 * J - 1.0;
    int r = (int)((t - sqrt(t * t - 8.0 * (double)k)) * 0.5);
    r = r < 0 ? 0 : (r > J - 2 ? J - 2 : r);
    while (r > 0 && (long)r * (2L * J - r - 1) / 2 > k) --r;
    while (r < J - 2 && (long)(r + 1) * (2L * J - r - 2) / 2 <= k) ++r;
    i = r;
    j = k - (int)((long)r * (2L * J - r - 1) / 2) + r + 1;
}

__device__ __forceinline__ int pair_index(int a, int b, int J) {           // a < b
    return (int)((long)a * (2L * J - a - 1) / 2) + (b - a - 1);
}

// inside_check / the cost loop on one sample: round(((s - t) / scale) * dims0) inside [0, 88) on every axis and occupied
__device__ __forceinline__ bool sample_inside(double sx, double sy, double sz, double tx, double ty, double tz, double scale, double dims0,
                                              const uint8_t* __restrict__ grid) {
    const double rx = rint(((sx - tx) / scale) * dims0), ry = rint(((sy - ty) / scale) * dims0), rz = rint(((sz - tz) / scale) * dims0);
    const bool in = rx >= 0.0 && rx < (double)SK_VG && ry >= 0.0 && ry < (double)SK_VG && rz >= 0.0 && rz < (double)SK_VG;   // NaN: outside
    if (!in) return false;
    return grid[((long)(int)rx * SK_VG + (int)ry) * SK_VG + (int)rz] != 0;
}

// samples p + u * i, i = 1 .. ns, of one bone, lanes over i: the number inside (the same on every lane)
__device__ __forceinline__ int count_inside(double px, double py, double pz, double ux, double uy, double uz, long ns, int lane,
                                            double tx, double ty, double tz, double scale, double dims0, const uint8_t* __restrict__ grid) {
    int n = 0;
    for (long base = 0; base < ns; base += 64) {                          // uniform trip count: the ballot sees the whole wave
        const long i = base + lane + 1;
        bool in = false;
        if (i <= ns) {
            const double fi = (double)i;
            in = sample_inside(px + ux * fi, py + uy * fi, pz + uz * fi, tx, ty, tz, scale, dims0, grid);
        }
        n += __popcll(__ballot(in));
    }
    return n;
}

// status[0]: 0, or 1 = a bone with more than 2^24 samples (its counts are then left 0)
__global__ __launch_bounds__(SK_PAIR_THREADS) void pair_attr_kernel(
    const double* __restrict__ joints64, const float* __restrict__ joints32, const int32_t* __restrict__ joint_ptr,
    const int32_t* __restrict__ pair_ptr, int n_meshes, int n_pairs, const uint8_t* __restrict__ vox, const double* __restrict__ vox_tf,
    int64_t* __restrict__ pairs, float* __restrict__ pair_attr, int32_t* __restrict__ outside_count, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (SK_PAIR_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= n_pairs) return;                                              // whole waves leave together
    const int b = segment_of(pair_ptr, n_meshes, g);
    const int j0 = joint_ptr[b], J = joint_ptr[b + 1] - j0;
    if (J < 2) return;                                                     // pair_ptr that disagrees with joint_ptr: nothing is read
    int i, j;
    pair_of(g - pair_ptr[b], J, i, j);
    j = j > J - 1 ? J - 1 : j;
    const double tx = vox_tf[b * 5 + 0], ty = vox_tf[b * 5 + 1], tz = vox_tf[b * 5 + 2], scale = vox_tf[b * 5 + 3], dims0 = vox_tf[b * 5 + 4];
    const uint8_t* grid = vox + (long)b * SK_VOXELS;
    bool too_long = false;

    // create_one_data (:237-241): float64 joints throughout
    const double* p = joints64 + (long)(j0 + i) * 3;
    const double* c = joints64 + (long)(j0 + j) * 3;
    const double ex = p[0] - c[0], ey = p[1] - c[1], ez = p[2] - c[2];
    const double len = sqrt((ex * ex + ey * ey) + ez * ez);
    const double ns = rint(len / 0.01);
    double proportion = 0.0;                                               // 0 samples: 0 / (0 + 1e-10)
    if (ns >= 1.0 && ns <= SK_MAX_SAMPLES) {
        const double den = ns + 1e-30;
        const int inside = count_inside(p[0], p[1], p[2], (c[0] - p[0]) / den, (c[1] - p[1]) / den, (c[2] - p[2]) / den, (long)ns, lane,
                                        tx, ty, tz, scale, dims0, grid);
        proportion = (double)inside / (ns + 1e-10);
    } else if (ns > SK_MAX_SAMPLES) too_long = true;

    // increase_cost_for_outside_bone (:275-283): float32 joints; ray, length, step count and unit step stay float32 (a float32 scalar
    // against a Python float stays float32 under NumPy 2), the sample positions are float64 because arange(1, n + 1) is
    const float* pf = joints32 + (long)(j0 + i) * 3;
    const float* cf = joints32 + (long)(j0 + j) * 3;
    const float fx = pf[0] - cf[0], fy = pf[1] - cf[1], fz = pf[2] - cf[2];
    const float lenf = sqrtf((fx * fx + fy * fy) + fz * fz);
    const float nsf = rintf(lenf / 0.01f);
    int outside = 0;
    if (nsf >= 1.0f && (double)nsf <= SK_MAX_SAMPLES) {
        const float denf = nsf + 1e-30f;
        const float ux = (cf[0] - pf[0]) / denf, uy = (cf[1] - pf[1]) / denf, uz = (cf[2] - pf[2]) / denf;
        const long n = (long)nsf;
        outside = (int)n - count_inside((double)pf[0], (double)pf[1], (double)pf[2], (double)ux, (double)uy, (double)uz, n, lane,
                                        tx, ty, tz, scale, dims0, grid);
    } else if ((double)nsf > SK_MAX_SAMPLES) too_long = true;

    if (lane == 0) {
        pairs[(long)g * 2 + 0] = j0 + i;
        pairs[(long)g * 2 + 1] = j0 + j;
        pair_attr[(long)g * 3 + 0] = (float)len;
        pair_attr[(long)g * 3 + 1] = (float)proportion;
        pair_attr[(long)g * 3 + 2] = 1.0f;
        outside_count[g] = outside;
        if (too_long) atomicMax(status, 1);
    }
}

// torch.sigmoid of a float32 logit, as the correctly rounded float32 of the float64 value
__device__ __forceinline__ float sigmoid_f32(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }

// grid (blocks over the J x J entries, mesh). predict_skeleton :212-218 + increase_cost_for_outside_bone :285-290
__global__ __launch_bounds__(256) void skeleton_cost_kernel(
    const float* __restrict__ pair_logits, int ld_pair, const float* __restrict__ root_logits, int ld_root, const float* __restrict__ joints32,
    const int32_t* __restrict__ outside_count, const int32_t* __restrict__ joint_ptr, const int32_t* __restrict__ pair_ptr,
    const int64_t* __restrict__ cost_off, double* __restrict__ cost, int32_t* __restrict__ root) {
    const int b = blockIdx.y;
    const int j0 = joint_ptr[b], J = joint_ptr[b + 1] - j0;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < (long)J * J) {
        const int r = (int)(e / J), c = (int)(e % J);
        double v;
        if (r == c) v = -log(1e-10);
        else {
            const int lo = r < c ? r : c, hi = r < c ? c : r;
            const long k = (long)pair_ptr[b] + pair_index(lo, hi, J);
            const double prob = (double)sigmoid_f32(pair_logits[k * ld_pair]);
            v = -log(prob + 1e-10);
            const int n_out = outside_count[k];
            if (n_out > 1) v = (double)(2 * (long)n_out);
            // np.abs(float32) < 2e-2: the Python float is compared as a float32
            if (fabsf(joints32[(long)(j0 + lo) * 3]) < 2e-2f && fabsf(joints32[(long)(j0 + hi) * 3]) < 2e-2f) v *= 0.5;
        }
        cost[cost_off[b] + e] = v;
    }
    // root id: np.argmax of the float32 sigmoid, first index on ties (one wave of the mesh's first workgroup)
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        float best = -1.0f;                                               // below every sigmoid; NaN never wins, as in np.argmax without NaN
        int arg = 0x7fffffff;
        for (int v = threadIdx.x; v < J; v += 64) {
            const float s = sigmoid_f32(root_logits[(long)(j0 + v) * ld_root]);
            if (s > best) { best = s; arg = v; }                          // ascending v per lane: the first of equal values stays
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (threadIdx.x == 0) root[b] = J > 0 ? (arg == 0x7fffffff ? 0 : arg) : -1;
    }
}

// status[b]: 0, 1 = the graph is disconnected (the reference's minKey raises), 2 = root outside [0, J), 3 = more joints than the limit
__global__ __launch_bounds__(SK_PRIM_THREADS) void prim_mst_kernel(
    const double* __restrict__ cost, const int64_t* __restrict__ cost_off, const int32_t* __restrict__ joint_ptr,
    const int32_t* __restrict__ root, int32_t* __restrict__ parent, double* __restrict__ key_out, int32_t* __restrict__ status) {
    __shared__ double s_key[MORIG_PRIM_MAX_JOINTS];
    __shared__ int s_parent[MORIG_PRIM_MAX_JOINTS];
    __shared__ unsigned char s_in[MORIG_PRIM_MAX_JOINTS];
    __shared__ double s_wkey[2][SK_PRIM_THREADS / 64];
    __shared__ int s_widx[2][SK_PRIM_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int j0 = joint_ptr[b], J = joint_ptr[b + 1] - j0;
    if (J <= 0) { if (tid == 0) status[b] = 0; return; }
    const int r = root[b];
    if (J > MORIG_PRIM_MAX_JOINTS || r < 0 || r >= J) {                    // uniform
        if (tid == 0) status[b] = J > MORIG_PRIM_MAX_JOINTS ? 3 : 2;
        return;
    }
    const double* C = cost + cost_off[b];
    const double inf = __longlong_as_double(0x7ff0000000000000LL);         // the reference's sys.maxsize: above every cost
    // joint v belongs to thread v % 256: key, flag and parent of v are touched by that thread alone
    for (int v = tid; v < J; v += SK_PRIM_THREADS) { s_key[v] = v == r ? 0.0 : inf; s_parent[v] = -1; s_in[v] = 0; }
    bool connected = true;
    for (int step = 0; step < J; ++step) {
        // minKey: the smallest key outside the tree, the first index among equal keys; a joint no edge has reached is no candidate
        double bk = inf;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < SK_PRIM_SLOTS; ++k) {
            const int v = tid + k * SK_PRIM_THREADS;
            if (v < J && !s_in[v] && s_key[v] < bk) { bk = s_key[v]; bi = v; }      // ascending v: strict < keeps the first
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(bk, off);
            const int oi = __shfl_xor(bi, off);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ok < bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
        }
        const int buf = step & 1;                                          // two buffers: the next step's writes need no second barrier
        if ((tid & 63) == 0) { s_wkey[buf][tid >> 6] = bk; s_widx[buf][tid >> 6] = bi; }
        __syncthreads();
        bk = s_wkey[buf][0]; bi = s_widx[buf][0];
#pragma unroll
        for (int w = 1; w < SK_PRIM_THREADS / 64; ++w) {
            const double ok = s_wkey[buf][w];
            const int oi = s_widx[buf][w];
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ok < bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
        }
        if (bi == 0x7fffffff) { connected = false; break; }                // uniform: every thread read the same four entries
        const int u = bi;
        if ((u % SK_PRIM_THREADS) == tid) s_in[u] = 1;
        const double* row = C + (long)u * J;
#pragma unroll
        for (int k = 0; k < SK_PRIM_SLOTS; ++k) {
            const int v = tid + k * SK_PRIM_THREADS;
            if (v < J && !s_in[v]) {
                const double c = row[v];
                if (c > 0.0 && s_key[v] > c) { s_key[v] = c; s_parent[v] = u; }     // cost > 0 is the reference's edge test
            }
        }
    }
    for (int v = tid; v < J; v += SK_PRIM_THREADS) {
        parent[j0 + v] = connected ? s_parent[v] : -1;
        key_out[j0 + v] = s_key[v];
    }
    if (tid == 0) status[b] = connected ? 0 : 1;
}

}  // namespace morig

using namespace morig;

extern "C" int morig_pair_attr(const double* joints64, const float* joints32, const int32_t* joint_ptr, const int32_t* pair_ptr,
                               int32_t n_meshes, int32_t n_pairs, const uint8_t* vox, const double* vox_tf, int64_t* pairs,
                               float* pair_attr, int32_t* outside_count, int32_t* status, void* stream) {
    if (!joint_ptr || !pair_ptr || !vox || !vox_tf || !status || n_meshes <= 0 || n_pairs < 0) return MORIG_E_INVALID;
    if (n_pairs > 0 && (!joints64 || !joints32 || !pairs || !pair_attr || !outside_count)) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_pairs == 0) return MORIG_OK;
    hipLaunchKernelGGL(pair_attr_kernel, dim3(cdiv(n_pairs, SK_PAIR_THREADS / 64)), dim3(SK_PAIR_THREADS), 0, s, joints64, joints32, joint_ptr,
                       pair_ptr, n_meshes, n_pairs, vox, vox_tf, pairs, pair_attr, outside_count, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skeleton_cost(const float* pair_logits, int32_t ld_pair, const float* root_logits, int32_t ld_root, const float* joints32,
                                   const int32_t* outside_count, const int32_t* joint_ptr, const int32_t* pair_ptr, const int64_t* cost_off,
                                   int32_t n_meshes, int32_t max_joints, double* cost, int32_t* root, void* stream) {
    if (!root_logits || !joints32 || !joint_ptr || !pair_ptr || !cost_off || !cost || !root || n_meshes <= 0 || max_joints < 1 ||
        ld_pair < 1 || ld_root < 1) return MORIG_E_INVALID;
    if (max_joints > 1 && (!pair_logits || !outside_count)) return MORIG_E_INVALID;
    if (max_joints > 46340 || n_meshes > 65535) return MORIG_E_UNSUPPORTED;          // J * J in an int; grid.y
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(skeleton_cost_kernel, dim3(cdiv((long)max_joints * max_joints, 256), n_meshes), dim3(256), 0, s, pair_logits, ld_pair,
                       root_logits, ld_root, joints32, outside_count, joint_ptr, pair_ptr, cost_off, cost, root);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_prim_mst(const double* cost, const int64_t* cost_off, const int32_t* joint_ptr, const int32_t* root, int32_t n_meshes,
                              int32_t max_joints, int32_t* parent, double* key, int32_t* status, void* stream) {
    if (!cost || !cost_off || !joint_ptr || !root || !parent || !key || !status || n_meshes <= 0 || max_joints < 1) return MORIG_E_INVALID;
    if (max_joints > MORIG_PRIM_MAX_JOINTS) return MORIG_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(prim_mst_kernel, dim3(n_meshes), dim3(SK_PRIM_THREADS), 0, s, cost, cost_off, joint_ptr, root, parent, key, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
