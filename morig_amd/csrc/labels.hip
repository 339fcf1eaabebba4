// Bone rays (morig_amd/labels.py): the nearest hit of arbitrary rays on the meshes of a ragged batch, the per-joint
// statistics of the hit distances and the per-vertex attention label. Everything is float64 in the written order of operations
// (contraction off) or integer; the only atomic is the integer OR into the status word: two runs give the same bits, and a mesh alone
// gives the bits it gives inside a batch.
//
// cast        one wave per ray; the lanes stride over the faces of the ray's mesh, every face through raytri_core.h with near = 0. A lane
//             keeps its best (t, face) under a strict `<` over ascending faces; the wave then takes the lexicographic minimum of (t, face)
//             through a butterfly of __shfl_xor, so ties on t go to the lowest face and every lane ends on the same pair. t = +inf never
//             wins, so an overflowing quotient is a miss. The winner's determinant is recomputed for the orientation filter: a nearest
//             hit of the wrong orientation makes the ray a miss. Face indices are clamped into the mesh's vertex block, so no read leaves
//             a buffer, and MORIG_RAY_BAD_FACE is ORed into the status word; a ray outside every segment of ray_ptr misses and raises
//             MORIG_RAY_BAD_TABLE.
// select      one wave per joint (boneray_core.h): the lanes stride over the joint's rays, rank every hit by counting, the two lanes that
//             own the percentile's neighbours hand them to the wave through a maximum (t > 0), every lane writes its kept flags, lane 0
//             adds the kept t in ascending ray order.
// attention   one thread per vertex; the rays of the vertex's mesh pass through LDS in tiles of 256 (hit point and kept flag); a thread
//             stops testing at the first kept hit within the radius, and a workgroup leaves the loop once all of its threads have.
#include "common.h"

#pragma clang fp contract(off)                 // in front of the rule headers: the pragma holds from here on

#include "boneray_core.h"
#include "raytri_core.h"

namespace morig {

namespace {

using morig_raytri::Num;
constexpr int TILE = 256;
constexpr int NO_FACE = 0x7fffffff;

// the corners of face f of a mesh with nv >= 1 vertices from row v0; true when an index had to be clamped
__device__ __forceinline__ bool load_face(const double* __restrict__ verts, const int* __restrict__ faces, int v0, int nv, size_t f, double (*P)[3]) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int raw = faces[f * 3 + k];
        const int id = min(max(raw, 0), nv - 1);
        bad = bad || id != raw;
#pragma unroll
        for (int c = 0; c < 3; ++c) P[k][c] = verts[((size_t)v0 + id) * 3 + c];
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------------------------------ cast
__global__ void __launch_bounds__(256) ray_cast_kernel(const double* __restrict__ origins, const double* __restrict__ dirs, const int* __restrict__ ray_ptr,
                                                       int n_rays, const double* __restrict__ verts, const int* __restrict__ vptr,
                                                       const int* __restrict__ faces, const int* __restrict__ fptr, int n_meshes, int orientation,
                                                       double* __restrict__ t_out, int* __restrict__ face_out, double* __restrict__ point,
                                                       int* __restrict__ status) {
    const int r = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rays) return;                                                            // uniform per wave
    const int b = segment_of(ray_ptr, n_meshes, r);
    const bool owned = ray_ptr[b] <= r && r < ray_ptr[b + 1];
    const int v0 = vptr[b], nv = vptr[b + 1] - v0, f0 = fptr[b], nf = fptr[b + 1] - f0;
    double o[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = origins[(size_t)r * 3 + c]; d[c] = dirs[(size_t)r * 3 + c]; }
    double best = INFINITY;
    int bf = NO_FACE;
    bool bad = !owned || (nf > 0 && nv < 1);
    if (owned && nv >= 1)
        for (int f = lane; f < nf; f += 64) {
            double P[3][3], t;
            bad = load_face(verts, faces, v0, nv, (size_t)f0 + f, P) || bad;
            const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
            if (morig_raytri::hit(n, 0.0, t) && t < best) { best = t; bf = f; }         // strict: the lowest face of the lane among equals
        }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double ot = __shfl_xor(best, m, 64);
        const int of = __shfl_xor(bf, m, 64);
        if (ot < best || (ot == best && of < bf)) { best = ot; bf = of; }
    }
    if (bad) atomicOr(status, !owned ? MORIG_RAY_BAD_TABLE : MORIG_RAY_BAD_FACE);
    if (lane != 0) return;
    double p[3] = {NAN, NAN, NAN};
    if (bf != NO_FACE) {
        double P[3][3];
        load_face(verts, faces, v0, nv, (size_t)f0 + bf, P);
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);                 // the bits the owning lane saw
        const bool wrong = (orientation > 0 && !(n.det < 0.0)) || (orientation < 0 && !(n.det > 0.0));
        if (wrong) { best = INFINITY; bf = NO_FACE; }
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = o[c] + best * d[c];
        }
    }
    t_out[r] = bf != NO_FACE ? best : INFINITY;
    face_out[r] = bf != NO_FACE ? bf : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) point[(size_t)r * 3 + c] = p[c];
}

// ------------------------------------------------------------------------------------------------------------------------ select
__global__ void __launch_bounds__(256) ray_select_kernel(const double* __restrict__ t, const int* __restrict__ joint_ptr, int n_joints, double keep_factor,
                                                         double fill, unsigned char* __restrict__ flags, double* __restrict__ stats) {
    const int j = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= n_joints) return;                                                          // uniform per wave
    const int r0 = joint_ptr[j];
    const int n = min(max(joint_ptr[j + 1] - r0, 0), morig_boneray::MAX_RAYS);          // the entry point refuses more before the launch
    const double* tj = t + r0;
    int n_hit = 0;
    for (int i = lane; i < n; i += 64) n_hit += morig_boneray::hit(tj[i]) ? 1 : 0;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) n_hit += __shfl_xor(n_hit, m, 64);
    double* out = stats + (size_t)j * MORIG_RAY_STATS;
    if (n_hit == 0) {
        for (int i = lane; i < n; i += 64) flags[(size_t)r0 + i] = 0;
        if (lane == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = NAN; out[3] = fill; }
        return;
    }
    int lo, hi;
    double frac, s_lo = -INFINITY, s_hi = -INFINITY;
    morig_boneray::position(n_hit, lo, hi, frac);
    for (int i = lane; i < n; i += 64) {
        if (!morig_boneray::hit(tj[i])) continue;
        const int rank = morig_boneray::rank_of(tj, n, i);
        if (rank == lo) s_lo = tj[i];
        if (rank == hi) s_hi = tj[i];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {                                                  // ranks are distinct: one lane holds each value
        s_lo = fmax(s_lo, __shfl_xor(s_lo, m, 64));
        s_hi = fmax(s_hi, __shfl_xor(s_hi, m, 64));
    }
    const double p20 = morig_boneray::value(s_lo, s_hi, frac);
    const double threshold = keep_factor * p20;
    for (int i = lane; i < n; i += 64) flags[(size_t)r0 + i] = morig_boneray::kept(tj[i], threshold) ? 1 : 0;
    if (lane == 0) {
        int count;
        const double fs = morig_boneray::mean_kept(tj, n, threshold, fill, count);
        out[0] = (double)n_hit; out[1] = (double)count; out[2] = p20; out[3] = fs;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ attention
__global__ void __launch_bounds__(TILE) ray_attention_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ blk_ptr,
                                                             int n_meshes, const double* __restrict__ point, const unsigned char* __restrict__ flags,
                                                             const int* __restrict__ ray_ptr, double r2, float* __restrict__ attn) {
    __shared__ double s_p[TILE][3];
    __shared__ unsigned char s_k[TILE];
    const BlockRow at = block_row(blk_ptr, n_meshes, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const int b = at.seg, v0 = vptr[b], nv = vptr[b + 1] - v0, r0 = ray_ptr[b], nr = ray_ptr[b + 1] - r0;
    const long long lv = at.row;
    const bool live = lv >= 0 && lv < nv;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) { x = verts[((size_t)v0 + lv) * 3]; y = verts[((size_t)v0 + lv) * 3 + 1]; z = verts[((size_t)v0 + lv) * 3 + 2]; }
    bool found = false;
    for (int base = 0; base < nr; base += TILE) {
        if (__syncthreads_and(found || !live)) break;                                   // uniform: also the barrier in front of the next tile
        const int i = base + (int)threadIdx.x;
        if (i < nr) {
            const unsigned char k = flags[(size_t)r0 + i];
            s_k[threadIdx.x] = k;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_p[threadIdx.x][c] = k ? point[((size_t)r0 + i) * 3 + c] : 0.0;
        }
        __syncthreads();
        const int m = min(TILE, nr - base);
        if (live && !found)
            for (int k = 0; k < m; ++k) {
                if (!s_k[k]) continue;
                const double dx = x - s_p[k][0], dy = y - s_p[k][1], dz = z - s_p[k][2];
                if ((dx * dx + dy * dy) + dz * dz <= r2) { found = true; break; }
            }
    }
    if (live) attn[(size_t)v0 + lv] = found ? 1.0f : 0.0f;
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_ray_cast(const double* origins, const double* dirs, const int32_t* ray_ptr, int32_t n_rays, const double* verts, const int32_t* vptr,
                   const int32_t* faces, const int32_t* fptr, int32_t n_meshes, int32_t orientation, double* t, int32_t* face, double* point,
                   int32_t* status, void* stream) {
    if (n_rays < 0 || n_meshes < 0 || orientation < -1 || orientation > 1 || !status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_rays == 0) return MORIG_OK;
    if (!origins || !dirs || !ray_ptr || !vptr || !fptr || !t || !face || !point || n_meshes == 0) return MORIG_E_INVALID;
    ProfScope ps(K_RAY_CAST, s, 0.0, 0.0);
    ray_cast_kernel<<<cdiv(n_rays, 4), 256, 0, s>>>(origins, dirs, ray_ptr, n_rays, verts, vptr, faces, fptr, n_meshes, orientation, t, face, point,
                                                    status);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_ray_select(const double* t, const int32_t* joint_ptr, int32_t n_joints, int32_t max_rays, double keep_factor, double fill, uint8_t* kept,
                     double* stats, void* stream) {
    if (n_joints < 0 || max_rays < 0) return MORIG_E_INVALID;
    if (max_rays > MORIG_RAY_MAX_PER_JOINT) return MORIG_E_UNSUPPORTED;
    if (n_joints == 0) return MORIG_OK;
    if (!joint_ptr || !stats || (max_rays > 0 && (!t || !kept))) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RAY_SELECT, s, 0.0, 0.0);
    ray_select_kernel<<<cdiv(n_joints, 4), 256, 0, s>>>(t, joint_ptr, n_joints, keep_factor, fill, kept, stats);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_ray_attention(const double* verts, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* point,
                        const uint8_t* kept, const int32_t* ray_ptr, double radius, float* attn, void* stream) {
    if (n_meshes < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!verts || !vptr || !blk_ptr || !ray_ptr || !attn || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_RAY_ATTENTION, s, 0.0, 0.0);
    ray_attention_kernel<<<n_blocks, TILE, 0, s>>>(verts, vptr, blk_ptr, n_meshes, point, kept, ray_ptr, radius * radius, attn);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
