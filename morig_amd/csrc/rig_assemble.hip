// The last step of the rigging driver (evaluate/joint2rig.py:147-162 assemble_skel_skin, :363-394 remove_dup_joints): per-bone skin
// weights [V, n_bones] -> per-joint skins [V, J], for all meshes of a batch at once. The tree bookkeeping (which bone writes to which
// joint of the rig with duplicated joints, which of those joints are folded into which final joint) is host work on host objects
// (morig_amd/rigging.py) and arrives as two CSR tables; the kernels replay what the reference's per-vertex loops do with the numbers.
// Everything is float64 copies and fixed-order sums, without atomics: two runs give the same bits.
//
// assemble   one thread per (vertex, output joint). An output joint owns segments, a segment owns bones in ascending order. A segment's
//            value is w of its LAST bone with w > 1e-5 (the reference's `skw_new[idx] = w` overwrites; strict, NaN is false), else 0;
//            a joint's value is the left-to-right sum of its segments' values (`skins[:, p] += skins[:, dup]`). The tables are read
//            from global memory by every thread -- they are a few KiB per batch and stay in L2; nothing is staged, so no size has
//            its own path.
// entries    the dense result -> the sparse form tracking.skin_entries gives: one wave per vertex, the row in chunks of 64 columns;
//            the lanes' non-zero flags are balloted, so the count pass is a popcount and the fill pass writes entry k of a vertex at
//            (its offset + the number of flagged lanes below it): ascending joint, no atomics.
#include "common.h"

#pragma clang fp contract(off)

namespace morig {

namespace {

__global__ __launch_bounds__(256) void rig_assemble_kernel(const double* __restrict__ W, long long ldw, int n_cols, int n_rows,
                                                           const int* __restrict__ vtx_ptr, const int* __restrict__ joint_ptr, int n_meshes,
                                                           const int* __restrict__ seg_ptr, int n_joints, const int* __restrict__ bone_ptr,
                                                           int n_segs, const int* __restrict__ bones, int n_bones, int raw,
                                                           double* __restrict__ out, int ld_out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_rows * ld_out) return;
    const int v = (int)(e / ld_out), j = (int)(e - (long long)v * ld_out);
    const int m = segment_of(vtx_ptr, n_meshes, v);
    double sum = 0.0;
    if (vtx_ptr[m] <= v && v < vtx_ptr[m + 1]) {
        const int j0 = joint_ptr[m], j1 = joint_ptr[m + 1];
        if (j0 >= 0 && j1 <= n_joints && j < j1 - j0) {
            const double* __restrict__ row = W + (size_t)v * ldw;
            int s0 = seg_ptr[j0 + j], s1 = seg_ptr[j0 + j + 1];
            if (s0 < 0) s0 = 0;
            if (s1 > n_segs) s1 = n_segs;
            for (int s = s0; s < s1; ++s) {
                int b0 = bone_ptr[s], b1 = bone_ptr[s + 1];
                if (b0 < 0) b0 = 0;
                if (b1 > n_bones) b1 = n_bones;
                double val = 0.0;
                for (int k = b0; k < b1; ++k) {
                    const int c = bones[k];
                    if (c < 0 || c >= n_cols) continue;
                    const double w = row[c];
                    if (raw || w > 1e-5) val = w;
                }
                sum = (s == s0) ? val : sum + val;
            }
        }
    }
    out[e] = sum;
}

// COUNT: counts[v] = #(x[v][j] != 0); otherwise entry k of vertex v goes to ent_ptr[v] + k
template <bool COUNT>
__global__ __launch_bounds__(256) void rig_entries_kernel(const double* __restrict__ x, int ld, int n_rows, int n_cols,
                                                          const int* __restrict__ vtx_ptr, int n_meshes, int* __restrict__ counts,
                                                          const int* __restrict__ ent_ptr, int n_entries, int* __restrict__ vertex,
                                                          int* __restrict__ joint, double* __restrict__ weight) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);                     // wave-uniform
    if (v >= n_rows) return;
    int base = 0, local = v;
    if constexpr (!COUNT) {
        base = ent_ptr[v];
        const int m = segment_of(vtx_ptr, n_meshes, v);
        local = (vtx_ptr[m] <= v && v < vtx_ptr[m + 1]) ? v - vtx_ptr[m] : -1;
    }
    const double* __restrict__ row = x + (size_t)v * ld;
    int n = 0;
    for (int c0 = 0; c0 < n_cols; c0 += 64) {                              // wave-uniform trip count: every lane ballots
        const int c = c0 + lane;
        const double w = c < n_cols ? row[c] : 0.0;
        const bool nz = w != 0.0;                                          // NaN != 0: an entry, as np.nonzero has it
        const unsigned long long mask = __ballot(nz);
        if constexpr (!COUNT) {
            if (nz) {
                const int k = base + n + __popcll(mask & ((1ull << lane) - 1ull));
                if (k >= 0 && k < n_entries) { vertex[k] = local; joint[k] = c; weight[k] = w; }
            }
        }
        n += __popcll(mask);
    }
    if constexpr (COUNT) {
        if (lane == 0) counts[v] = n;
    }
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_rig_assemble(const double* W, int64_t ldw, int32_t n_cols, int32_t n_rows, const int32_t* vtx_ptr, const int32_t* joint_ptr,
                       int32_t n_meshes, const int32_t* seg_ptr, int32_t n_joints, const int32_t* bone_ptr, int32_t n_segs,
                       const int32_t* bones, int32_t n_bones, int32_t flags, double* out, int32_t ld_out, void* stream) {
    if (n_rows < 0 || n_cols < 0 || n_meshes < 1 || n_joints < 0 || n_segs < 0 || n_bones < 0 || ld_out < 0 || ldw < n_cols) return MORIG_E_INVALID;
    if ((flags & ~MORIG_RIG_RAW) != 0) return MORIG_E_INVALID;
    const long long total = (long long)n_rows * ld_out;
    if (total == 0) return MORIG_OK;
    if (total > ((long long)1 << 38)) return MORIG_E_INVALID;
    if (!vtx_ptr || !joint_ptr || !seg_ptr || !bone_ptr || !out || (n_bones > 0 && (!bones || !W))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RIG_ASSEMBLE, s, 0.0, 8.0 * (double)total + 8.0 * (double)n_rows * n_cols);
    rig_assemble_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(W, (long long)ldw, n_cols, n_rows, vtx_ptr, joint_ptr, n_meshes,
                                                                        seg_ptr, n_joints, bone_ptr, n_segs, bones, n_bones,
                                                                        (flags & MORIG_RIG_RAW) ? 1 : 0, out, ld_out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_rig_skin_entries(const double* x, int32_t ld, int32_t n_rows, int32_t n_cols, const int32_t* vtx_ptr, int32_t n_meshes,
                           int32_t* counts, const int32_t* ent_ptr, int32_t n_entries, int32_t* vertex, int32_t* joint, double* weight,
                           void* stream) {
    if (n_rows < 0 || n_cols < 0 || ld < n_cols || n_meshes < 1 || n_entries < 0) return MORIG_E_INVALID;
    if (n_rows == 0) return MORIG_OK;
    if (!vtx_ptr || (n_cols > 0 && !x)) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (!ent_ptr) {                                                        // the count pass
        if (!counts) return MORIG_E_INVALID;
        ProfScope ps(K_RIG_ENTRIES, s, 0.0, 8.0 * (double)n_rows * n_cols);
        rig_entries_kernel<true><<<cdiv(n_rows, 4), 256, 0, s>>>(x, ld, n_rows, n_cols, vtx_ptr, n_meshes, counts, nullptr, 0, nullptr,
                                                                 nullptr, nullptr);
        MORIG_LAUNCH_CHECK();
        return MORIG_OK;
    }
    if (n_entries == 0) return MORIG_OK;
    if (!vertex || !joint || !weight) return MORIG_E_INVALID;
    ProfScope ps(K_RIG_ENTRIES, s, 0.0, 8.0 * (double)n_rows * n_cols + 16.0 * (double)n_entries);
    rig_entries_kernel<false><<<cdiv(n_rows, 4), 256, 0, s>>>(x, ld, n_rows, n_cols, vtx_ptr, n_meshes, nullptr, ent_ptr, n_entries, vertex,
                                                              joint, weight);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
