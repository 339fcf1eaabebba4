// Motion playback (morig_amd/playback.py): the reference's smooth_quats (evaluate/visualize_tracking.py:43-61) for a
// ragged batch of rigs and one clip length T -- smoothed quaternions, Rig.FK for every frame at once, linear-blend skinning into a vertex
// trajectory -- and the per-frame trajectory errors. Everything is float64 in the written order of operations (contraction off; the
// per-joint arithmetic is csrc/pose_core.h, shared with tools/pose_host_check.cpp); the only atomics are integer ORs into the status words:
// two runs give the same bits, and a mesh alone gives the bits it gives inside a batch.
//
// validate   one thread per joint row and per vertex row: parent / order entries outside the rig, entry offsets that do not rise inside
//            [0, E], entry joints outside the rig set MORIG_POSE_BAD_INDEX for the mesh. Every later kernel skips such a mesh whole, so
//            no index is ever followed unchecked and nothing of the mesh is written.
// quats      one thread per joint row, sequential over t (the sign alignment is a scan, the data is sum(J) T 32 bytes): copy with the
//            optional sign alignment, `passes` Jacobi passes in place with the two old neighbours carried in registers, then the matrices
//            R [row][9][T]; a zero or non-finite norm sets MORIG_POSE_BAD_QUAT.
// fk         one thread per (mesh, frame), lanes along t: walks the rig's level order, reads the parent's transform it wrote itself and
//            writes xf [row][12][T] (matrix, then position) -- the layout the skinning kernel reads with lanes along t.
// local      one thread per vertex row, once per entry: inverse bind transform of the entry's joint times [v; 1].
// skin       THE hot kernel: one thread per (vertex row, frame) in flat order v T + t, so a wave covers MORIG_POSE_FRAME_TILE = 64
//            consecutive frames and its 192 results are one contiguous run of the output, written as three 512-byte rows through LDS. A
//            vertex's entries and local coordinates are one wave-wide load per entry for the 64 frames (all lanes of a vertex share the
//            address); the 12 transform components are 12 loads of 64 consecutive doubles. Offsets into the output are 64-bit.
//            Floor: 24 bytes written per (vertex, frame). Bound in this form by the transform reads, 96 bytes per entry and (vertex,
//            frame) through the vector L1 / L2 (a rig's table, J 12 T doubles, stays in L2); there is no LDS-resident table, so J is not
//            limited by LDS.
// errors     one workgroup of 16 x 64 threads per (mesh, 64 frames): vertex lane l sums the vertices l, l + 16, ... ascending, the 16
//            lane sums are added ascending.
#include "common.h"

#pragma clang fp contract(off)

#include "pose_core.h"

namespace morig {

namespace {

constexpr int TILE = MORIG_POSE_FRAME_TILE;

__global__ void __launch_bounds__(256) pose_validate_kernel(const int* __restrict__ jptr, const int* __restrict__ parent,
                                                            const int* __restrict__ order, const int* __restrict__ vptr,
                                                            const int* __restrict__ eptr, const int* __restrict__ ent_joint, int n_meshes,
                                                            int n_joints, int n_rows, int n_entries, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_joints) {
        const int b = segment_of(jptr, n_meshes, i), J = jptr[b + 1] - jptr[b];
        const int p = parent[i], o = order ? order[i] : 0;
        if (p < -1 || p >= J || o < 0 || o >= J) atomicOr(&status[b], MORIG_POSE_BAD_INDEX);
    } else if (i - n_joints < n_rows && eptr) {
        const long long v = i - n_joints;
        const int b = segment_of(vptr, n_meshes, v), J = jptr[b + 1] - jptr[b];
        const int e0 = eptr[v], e1 = eptr[v + 1];
        bool bad = e0 < 0 || e1 < e0 || e1 > n_entries;
        if (!bad)
            for (int e = e0; e < e1; ++e) {
                const int j = ent_joint[e];
                bad = bad || j < 0 || j >= J;
            }
        if (bad) atomicOr(&status[b], MORIG_POSE_BAD_INDEX);
    }
}

__global__ void __launch_bounds__(64) pose_quats_kernel(const double* __restrict__ q_in, const int* __restrict__ jptr, int n_meshes,
                                                        int n_joints, int T, int passes, int align, double* __restrict__ q_out,
                                                        double* __restrict__ R, int* __restrict__ status) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_joints) return;
    const int b = segment_of(jptr, n_meshes, r);
    if (status[b] & MORIG_POSE_BAD_INDEX) return;
    const double* src = q_in + (size_t)r * T * 4;
    double* dst = q_out + (size_t)r * T * 4;
    double prev[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < T; ++t) {
        double q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = src[(size_t)t * 4 + c];
        if (align && t > 0 && morig_pose::dot4(q, prev) < 0.0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = -q[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) { dst[(size_t)t * 4 + c] = q[c]; prev[c] = q[c]; }
    }
    if (T >= 3)
        for (int pass = 0; pass < passes; ++pass) {
            double pv[4], cur[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { pv[c] = dst[c]; cur[c] = dst[4 + c]; }
            for (int t = 1; t < T - 1; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double next = dst[(size_t)(t + 1) * 4 + c];
                    dst[(size_t)t * 4 + c] = morig_pose::smooth(cur[c], next, pv[c]);
                    pv[c] = cur[c];
                    cur[c] = next;
                }
        }
    if (!R) return;
    bool bad = false;
    for (int t = 0; t < T; ++t) {
        double q[4], m[9];
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = dst[(size_t)t * 4 + c];
        bad = !morig_pose::quat_to_matrix(q, m) || bad;
#pragma unroll
        for (int c = 0; c < 9; ++c) R[((size_t)r * 9 + c) * T + t] = m[c];
    }
    if (bad) atomicOr(&status[b], MORIG_POSE_BAD_QUAT);
}

__global__ void __launch_bounds__(64) pose_fk_kernel(const double* __restrict__ R, const int* __restrict__ jptr, const int* __restrict__ parent,
                                                     const int* __restrict__ order, const double* __restrict__ offsets,
                                                     const double* __restrict__ root_pos, const int* __restrict__ pos_f32, int n_meshes, int T,
                                                     const int* __restrict__ status, double* xf) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long long)n_meshes * T) return;
    const int b = (int)(i / T), t = (int)(i - (long long)b * T);
    if (status[b] & MORIG_POSE_BAD_INDEX) return;
    const int j0 = jptr[b], J = jptr[b + 1] - j0;
    const bool f32 = pos_f32[b] != 0;
    for (int k = 0; k < J; ++k) {
        const int j = order[j0 + k], p = parent[j0 + j];
        double m[9], out[12];
#pragma unroll
        for (int c = 0; c < 9; ++c) m[c] = R[((size_t)(j0 + j) * 9 + c) * T + t];
        if (p < 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) out[c] = m[c];
#pragma unroll
            for (int a = 0; a < 3; ++a) out[9 + a] = root_pos[((size_t)b * T + t) * 3 + a];
        } else {
            double par[12], off[3];
#pragma unroll
            for (int c = 0; c < 12; ++c) par[c] = xf[((size_t)(j0 + p) * 12 + c) * T + t];
#pragma unroll
            for (int a = 0; a < 3; ++a) off[a] = offsets[(size_t)(j0 + j) * 3 + a];
            morig_pose::fk_step(par, m, off, f32, out);
        }
#pragma unroll
        for (int c = 0; c < 12; ++c) xf[((size_t)(j0 + j) * 12 + c) * T + t] = out[c];
    }
}

__global__ void __launch_bounds__(256) pose_local_kernel(const double* __restrict__ bind, const double* __restrict__ vtx,
                                                         const int* __restrict__ vptr, const int* __restrict__ jptr, const int* __restrict__ eptr,
                                                         const int* __restrict__ ent_joint, int n_meshes, int n_rows,
                                                         const int* __restrict__ status, double* __restrict__ local) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_rows) return;
    const int b = segment_of(vptr, n_meshes, v);
    if (status[b] & MORIG_POSE_BAD_INDEX) return;
    const int j0 = jptr[b];
    const double x[3] = {vtx[(size_t)v * 3], vtx[(size_t)v * 3 + 1], vtx[(size_t)v * 3 + 2]};
    for (int e = eptr[v]; e < eptr[v + 1]; ++e) {
        double bt[12], inv[12], l[3];
#pragma unroll
        for (int c = 0; c < 12; ++c) bt[c] = bind[(size_t)(j0 + ent_joint[e]) * 12 + c];
        morig_pose::inverse_transform(bt, inv);
        morig_pose::apply(inv, x, l);
#pragma unroll
        for (int a = 0; a < 3; ++a) local[(size_t)e * 3 + a] = l[a];
    }
}

__global__ void __launch_bounds__(256) pose_skin_kernel(const double* __restrict__ xf, const int* __restrict__ jptr, const int* __restrict__ vptr,
                                                        const int* __restrict__ eptr, const int* __restrict__ ent_joint,
                                                        const double* __restrict__ ent_weight, const double* __restrict__ local, int n_meshes,
                                                        long long n_rows, int T, const int* __restrict__ status, double* __restrict__ out) {
    __shared__ double sm[256 * 3];
    __shared__ unsigned char live[256];
    __shared__ int ends[2];
    const long long total = n_rows * T, first = (long long)blockIdx.x * 256, i = first + threadIdx.x;
    // one 64-bit division per workgroup, a 32-bit one per thread; the mesh is searched per thread only where the workgroup spans two
    const long long v_first = first / T;
    const unsigned in_first = (unsigned)(first - v_first * T) + threadIdx.x;
    if (threadIdx.x < 2) {
        const long long last = first + 255 < total ? first + 255 : total - 1;
        ends[threadIdx.x] = segment_of(vptr, n_meshes, threadIdx.x == 0 ? v_first : last / T);
    }
    __syncthreads();
    double acc[3] = {0.0, 0.0, 0.0};
    bool mine = false;
    if (i < total) {
        const long long v = v_first + in_first / (unsigned)T;
        const int t = (int)(in_first % (unsigned)T), b = ends[0] == ends[1] ? ends[0] : segment_of(vptr, n_meshes, v);
        if (!(status[b] & MORIG_POSE_BAD_INDEX)) {
            mine = true;
            const int j0 = jptr[b];
            for (int e = eptr[v]; e < eptr[v + 1]; ++e) {
                const double w = ent_weight[e];
                if (w == 0.0) continue;
                const double* base = xf + (size_t)(j0 + ent_joint[e]) * 12 * T + t;
                double m[12], p[3];
#pragma unroll
                for (int c = 0; c < 12; ++c) m[c] = base[(size_t)c * T];
                const double l[3] = {local[(size_t)e * 3], local[(size_t)e * 3 + 1], local[(size_t)e * 3 + 2]};
                morig_pose::apply(m, l, p);
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] = acc[a] + w * p[a];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) sm[threadIdx.x * 3 + a] = acc[a];
    live[threadIdx.x] = mine ? 1 : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int slot = k * 256 + threadIdx.x;                 // element `slot` of the workgroup's contiguous run of 768 doubles
        if (live[slot / 3]) out[(size_t)first * 3 + slot] = sm[slot];
    }
}

__global__ void __launch_bounds__(1024) pose_errors_kernel(const double* __restrict__ pred, const double* __restrict__ gt,
                                                           const unsigned char* __restrict__ vis, const int* __restrict__ vptr, int T,
                                                           double* __restrict__ full, double* __restrict__ visible) {
    __shared__ double sh[2][16][TILE];
    __shared__ int shn[16][TILE];
    const int b = blockIdx.y, tl = threadIdx.x & (TILE - 1), vl = threadIdx.x >> 6, t = blockIdx.x * TILE + tl;
    const int v0 = vptr[b], v1 = vptr[b + 1];
    double s = 0.0, sv = 0.0;
    int n = 0;
    if (t < T)
        for (int v = v0 + vl; v < v1; v += 16) {
            const size_t at = (size_t)v * T + t;
            const double dx = pred[at * 3] - gt[at * 3], dy = pred[at * 3 + 1] - gt[at * 3 + 1], dz = pred[at * 3 + 2] - gt[at * 3 + 2];
            const double d = sqrt((dx * dx + dy * dy) + dz * dz);
            const int seen = vis[at] ? 1 : 0;
            s = s + d;
            sv = sv + d * (double)seen;                         // d * 0, as numpy's (d * vis).sum(): a NaN distance stays a NaN
            n += seen;
        }
    sh[0][vl][tl] = s; sh[1][vl][tl] = sv; shn[vl][tl] = n;
    __syncthreads();
    if (vl == 0 && t < T) {
        double S = 0.0, SV = 0.0;
        int N = 0;
        for (int l = 0; l < 16; ++l) { S = S + sh[0][l][tl]; SV = SV + sh[1][l][tl]; N += shn[l][tl]; }
        full[(size_t)b * T + t] = S / (double)(v1 - v0);
        visible[(size_t)b * T + t] = SV / (double)N;
    }
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_pose_validate(const int32_t* jptr, const int32_t* parent, const int32_t* order, const int32_t* vptr, const int32_t* eptr,
                        const int32_t* ent_joint, int32_t n_meshes, int32_t n_joints, int32_t n_rows, int32_t n_entries, int32_t* status,
                        void* stream) {
    if (n_meshes < 0 || n_joints < 0 || n_rows < 0 || n_entries < 0) return MORIG_E_INVALID;
    if (n_meshes == 0) return MORIG_OK;
    if (!jptr || !parent || !status || (eptr && (!vptr || (n_entries > 0 && !ent_joint)))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_PREP, s, 0.0, 0.0);
    const long n = (long)n_joints + (eptr ? (long)n_rows : 0);
    if (n == 0) return MORIG_OK;
    pose_validate_kernel<<<cdiv(n, 256), 256, 0, s>>>(jptr, parent, order, vptr, eptr, ent_joint, n_meshes, n_joints, eptr ? n_rows : 0, n_entries,
                                                      status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_pose_quats(const double* quats, const int32_t* jptr, int32_t n_meshes, int32_t n_joints, int32_t T, int32_t passes, int32_t align_signs,
                     double* quats_out, double* R, int32_t* status, void* stream) {
    if (n_meshes < 0 || n_joints < 0 || T < 0 || passes < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_joints == 0 || T == 0) return MORIG_OK;
    if (!quats || !jptr || !quats_out || !status || quats == quats_out) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_PREP, s, 0.0, 0.0);
    pose_quats_kernel<<<cdiv(n_joints, 64), 64, 0, s>>>(quats, jptr, n_meshes, n_joints, T, passes, align_signs, quats_out, R, status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_pose_fk(const double* R, const int32_t* jptr, const int32_t* parent, const int32_t* order, const double* offsets, const double* root_pos,
                  const int32_t* pos_f32, int32_t n_meshes, int32_t T, const int32_t* status, double* xf, void* stream) {
    if (n_meshes < 0 || T < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || T == 0) return MORIG_OK;
    if (!R || !jptr || !parent || !order || !offsets || !root_pos || !pos_f32 || !status || !xf) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_PREP, s, 0.0, 0.0);
    pose_fk_kernel<<<cdiv((long)n_meshes * T, 64), 64, 0, s>>>(R, jptr, parent, order, offsets, root_pos, pos_f32, n_meshes, T, status, xf);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_pose_local(const double* bind, const double* vtx, const int32_t* vptr, const int32_t* jptr, const int32_t* eptr, const int32_t* ent_joint,
                     int32_t n_meshes, int32_t n_rows, const int32_t* status, double* local, void* stream) {
    if (n_meshes < 0 || n_rows < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0) return MORIG_OK;
    if (!bind || !vtx || !vptr || !jptr || !eptr || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_PREP, s, 0.0, 0.0);
    pose_local_kernel<<<cdiv(n_rows, 256), 256, 0, s>>>(bind, vtx, vptr, jptr, eptr, ent_joint, n_meshes, n_rows, status, local);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_pose_skin(const double* xf, const int32_t* jptr, const int32_t* vptr, const int32_t* eptr, const int32_t* ent_joint,
                    const double* ent_weight, const double* local, int32_t n_meshes, int32_t n_rows, int32_t T, const int32_t* status, double* out,
                    void* stream) {
    if (n_meshes < 0 || n_rows < 0 || T < 0) return MORIG_E_INVALID;
    if (n_meshes == 0 || n_rows == 0 || T == 0) return MORIG_OK;
    if (!xf || !jptr || !vptr || !eptr || !status || !out) return MORIG_E_INVALID;
    const long long total = (long long)n_rows * T;
    if ((total + 255) / 256 > 0x7fffffffLL) return MORIG_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_SKIN, s, 0.0, 24.0 * (double)total);
    pose_skin_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(xf, jptr, vptr, eptr, ent_joint, ent_weight, local, n_meshes, n_rows, T, status,
                                                                     out);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_pose_traj_errors(const double* pred, const double* gt, const uint8_t* vis, const int32_t* vptr, int32_t n_meshes, int32_t T, double* full,
                           double* visible, void* stream) {
    if (n_meshes < 0 || T < 0 || n_meshes > 65535) return MORIG_E_INVALID;
    if (n_meshes == 0 || T == 0) return MORIG_OK;
    if (!vptr || !full || !visible) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_POSE_ERRORS, s, 0.0, 0.0);
    pose_errors_kernel<<<dim3(cdiv(T, TILE), n_meshes), 1024, 0, s>>>(pred, gt, vis, vptr, T, full, visible);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
