// Skinning on either side of SkinNet: the volumetric geodesic distance of every vertex to every bone
// (data_proc/common_ops.py:275-328 calc_volumetric_geodesic / one_bone), the per-vertex "bind" rows and labels built from it
// (data_proc/gen_skin_data.py:86-118, the tensors datasets/dataset_rig.py:30-76,94-101 makes of them) and the post-processing of
// SkinNet's logits into final weights (training/train_skin.py:40-66,232-244; evaluate/joint2rig.py:447-462).
//
// Volumetric geodesic: one job = (mesh, bone), a persistent grid of one 1024-thread workgroup per CU pulls jobs from a counter.
// A job's reached set lives in LDS as a bitset, 88 x 88 rows along z of 4 words (88 bits + one zero pad word, so a row is one 16-byte
// read): 123 904 B. The mesh's occupancy grid is the same layout in global memory (packed once per mesh, L2-resident across its bones).
// One call of the reference's binary_dilation(reached, 3x3x3, mask=occupancy) is one synchronous step: every thread ORs the 9 (dx, dy)
// rows of its own rows, dilates along z with carries between the words and keeps `new = dilated & occupied & ~reached` in registers;
// a barrier; then each owner ORs its new bits into LDS, counts them and writes their layer. The step's result never needs a second
// LDS buffer. Layers (the reference's distmap) go to a per-slot uint16 map in global memory, written once when a voxel is reached and
// read only at reached voxels, so the map is never cleared.
#include "common.h"

// voxel indices decide everything below: products and sums round separately, as numpy does (see joints.hip for why a pragma)
#pragma clang fp contract(off)

namespace morig {

constexpr int VG = 88;                       // the reference hard-codes 88^3 (the clip to 87 in one_bone / calc_volumetric_geodesic)
constexpr int VG_ROWS = VG * VG;             // rows (x, y), z along the bits
constexpr int VG_WORDS = VG_ROWS * 4;        // 3 words of bits + 1 zero word per row
constexpr int VG_VOXELS = VG * VG * VG;
constexpr int GEO_THREADS = 1024;
constexpr int GEO_RPT = (VG_ROWS + GEO_THREADS - 1) / GEO_THREADS;   // rows owned per thread: 8
constexpr int GEO_MAX_LAYER = 65535;
constexpr long GEO_MAX_SAMPLES = 1L << 24;

// status[0]: 0, or 1 = a layer above 65535, 2 = a bone with more than 2^24 samples; status[1]: the job counter
enum { GEO_ERR_LAYER = 1, GEO_ERR_SAMPLES = 2 };

__device__ __forceinline__ int vox_coord(double p, double t, double scale, double dims0) {
    double r = rint(((p - t) / scale) * dims0);          // np.round: half to even
    r = fmin(fmax(r, 0.0), 87.0);                        // np.clip(.., 0, 87) (NaN -> 0, as the int cast then clip does)
    return (int)r;
}

__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint4 andnot4(uint4 a, uint4 b) { return make_uint4(a.x & ~b.x, a.y & ~b.y, a.z & ~b.z, a.w & ~b.w); }
__device__ __forceinline__ bool any4(uint4 a) { return (a.x | a.y | a.z) != 0u; }
__device__ __forceinline__ int popc4(uint4 a) { return __popc(a.x) + __popc(a.y) + __popc(a.z); }
// bit z of the result = bit z - 1 / z + 1 of a (88 bits in words x, y, z; w stays 0)
__device__ __forceinline__ uint4 zminus(uint4 a) { return make_uint4(a.x << 1, (a.y << 1) | (a.x >> 31), (a.z << 1) | (a.y >> 31), 0u); }
__device__ __forceinline__ uint4 zplus(uint4 a) { return make_uint4((a.x >> 1) | (a.y << 31), (a.y >> 1) | (a.z << 31), a.z >> 1, 0u); }
__device__ __forceinline__ uint4 zdilate(uint4 a) { return or4(or4(a, zminus(a)), zplus(a)); }
__device__ __forceinline__ uint4 zinterior(uint4 a) { return and4(zminus(a), zplus(a)); }
__device__ __forceinline__ uint32_t word_of(uint4 a, int w) { return w == 0 ? a.x : (w == 1 ? a.y : a.z); }

// occupancy grids, uint8 [n_meshes][88^3] -> bit rows [n_meshes][7744][4]
__global__ void vox_pack_kernel(const uint8_t* __restrict__ vox, int n_meshes, uint32_t* __restrict__ bits) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_meshes * VG_WORDS) return;
    const long b = i / VG_WORDS;
    const int rw = (int)(i % VG_WORDS), row = rw >> 2, w = rw & 3;
    uint32_t v = 0;
    if (w < 3) {
        const uint8_t* src = vox + b * VG_VOXELS + (long)row * VG;
        for (int j = 0; j < 32; ++j) {
            const int z = w * 32 + j;
            if (z < VG && src[z]) v |= 1u << j;
        }
    }
    bits[i] = v;
}

__device__ __forceinline__ uint4 lds_row(const uint4* s, int x, int y) {
    return (x < 0 || x >= VG || y < 0 || y >= VG) ? make_uint4(0u, 0u, 0u, 0u) : s[x * VG + y];
}
__device__ __forceinline__ uint4 mask_row(const uint4* m, int x, int y) {
    return (x < 0 || x >= VG || y < 0 || y >= VG) ? make_uint4(0u, 0u, 0u, 0u) : m[x * VG + y];
}

__device__ int block_sum(int v, int* s_tmp) {
    // wave sum, then one LDS add per wave; s_tmp zeroed by the caller before the preceding barrier
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(s_tmp, v);
    __syncthreads();
    return *s_tmp;
}

// The patch of one_bone (common_ops.py:297-312): A = occupied & unreached, R = reached. Every unreached voxel at the minimum distance
// to R is reached with layer (layer of its nearest reached voxel) + 1. A closest pair of A and R has both ends on the 6-boundaries of
// their sets (a step from an interior point towards the other end stays in the set and is strictly closer), so only boundary voxels
// are listed. Ties among equally near reached voxels: the smallest layer (the reference's KDTree picks one of them). Squared distances
// are integers and compare exactly. Returns the number of patched voxels.
__device__ __forceinline__ int geo_patch(uint4* s_reach, const uint4* maskb, uint16_t* __restrict__ layer, uint32_t* __restrict__ list,
                                         int* s_small) {
    const int tid = threadIdx.x;
    int* s_nA = s_small + 0;
    int* s_nR = s_small + 1;
    int* s_D = s_small + 2;
    int* s_P = s_small + 3;
    __syncthreads();
    if (tid == 0) { *s_nA = 0; *s_nR = 0; *s_D = 0x7fffffff; *s_P = 0; }
    __syncthreads();
    for (int row = tid; row < VG_ROWS; row += GEO_THREADS) {
        const int x = row / VG, y = row % VG;
        // R's boundary on this row
        const uint4 r = s_reach[row];
        if (any4(r)) {
            uint4 in = and4(and4(lds_row(s_reach, x - 1, y), lds_row(s_reach, x + 1, y)),
                            and4(lds_row(s_reach, x, y - 1), lds_row(s_reach, x, y + 1)));
            in = and4(in, zinterior(r));
            const uint4 bnd = andnot4(r, in);
            const int c = popc4(bnd);
            if (c) {
                int base = atomicAdd(s_nR, c);
                for (int w = 0; w < 3; ++w)
                    for (uint32_t m = word_of(bnd, w); m; m &= m - 1) {
                        const int z = w * 32 + __ffs(m) - 1;
                        list[VG_VOXELS - 1 - base] = ((uint32_t)x << 16) | ((uint32_t)y << 8) | (uint32_t)z;
                        ++base;
                    }
            }
        }
        // A's boundary on this row (the neighbour rows' A from the occupancy and LDS)
        auto arow = [&](int xx, int yy) { return andnot4(mask_row(maskb, xx, yy), lds_row(s_reach, xx, yy)); };
        const uint4 a = andnot4(maskb[row], r);
        if (any4(a)) {
            uint4 in = and4(and4(arow(x - 1, y), arow(x + 1, y)), and4(arow(x, y - 1), arow(x, y + 1)));
            in = and4(in, zinterior(a));
            const uint4 bnd = andnot4(a, in);
            const int c = popc4(bnd);
            if (c) {
                int base = atomicAdd(s_nA, c);
                for (int w = 0; w < 3; ++w)
                    for (uint32_t m = word_of(bnd, w); m; m &= m - 1) {
                        const int z = w * 32 + __ffs(m) - 1;
                        list[base] = ((uint32_t)x << 16) | ((uint32_t)y << 8) | (uint32_t)z;
                        ++base;
                    }
            }
        }
    }
    __syncthreads();
    const int nA = *s_nA, nR = *s_nR;
    const uint32_t* Rl = list + (VG_VOXELS - nR);
    // pass 1: the minimum squared distance D over all pairs
    int dmin = 0x7fffffff;
    for (int i = tid; i < nA; i += GEO_THREADS) {
        const uint32_t e = list[i];
        const int ax = (int)(e >> 16), ay = (int)((e >> 8) & 255u), az = (int)(e & 255u);
        for (int j = 0; j < nR; ++j) {
            const uint32_t f = Rl[j];
            const int dx = ax - (int)(f >> 16), dy = ay - (int)((f >> 8) & 255u), dz = az - (int)(f & 255u);
            const int d2 = dx * dx + dy * dy + dz * dz;
            dmin = d2 < dmin ? d2 : dmin;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(dmin, o); dmin = t < dmin ? t : dmin; }
    if ((tid & 63) == 0) atomicMin(s_D, dmin);
    __syncthreads();
    const int D = *s_D;
    // pass 2: every A voxel at distance D from R takes the smallest layer among its reached voxels at D, + 1
    int np = 0;
    for (int i = tid; i < nA; i += GEO_THREADS) {
        const uint32_t e = list[i];
        const int ax = (int)(e >> 16), ay = (int)((e >> 8) & 255u), az = (int)(e & 255u);
        int best = 0x7fffffff;
        for (int j = 0; j < nR; ++j) {
            const uint32_t f = Rl[j];
            const int rx = (int)(f >> 16), ry = (int)((f >> 8) & 255u), rz = (int)(f & 255u);
            const int dx = ax - rx, dy = ay - ry, dz = az - rz;
            if (dx * dx + dy * dy + dz * dz == D) {
                const int l = (int)layer[(rx * VG + ry) * VG + rz];
                best = l < best ? l : best;
            }
        }
        if (best != 0x7fffffff) {
            layer[(ax * VG + ay) * VG + az] = (uint16_t)(best + 1);
            atomicOr(reinterpret_cast<uint32_t*>(s_reach) + (ax * VG + ay) * 4 + (az >> 5), 1u << (az & 31));
            ++np;
        }
    }
    for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o);
    if ((tid & 63) == 0 && np) atomicAdd(s_P, np);
    __syncthreads();
    return *s_P;
}

__global__ __launch_bounds__(GEO_THREADS) void vol_geodesic_kernel(
        const uint32_t* __restrict__ mask_bits, const double* __restrict__ vox_tf, const double* __restrict__ pos,
        const int32_t* __restrict__ vtx_ptr, const double* __restrict__ bones, const int32_t* __restrict__ bone_ptr, int n_meshes,
        const int64_t* __restrict__ dist_off, int n_jobs, uint16_t* __restrict__ layer_ws, uint32_t* __restrict__ list_ws,
        int32_t* __restrict__ status, int32_t* __restrict__ dist) {
    __shared__ uint4 s_reach[VG_ROWS];
    __shared__ int s_cnt[2];
    __shared__ int s_small[4];
    __shared__ int s_job, s_tmp;
    const int tid = threadIdx.x;
    uint16_t* layer = layer_ws + (size_t)blockIdx.x * VG_VOXELS;
    uint32_t* list = list_ws + (size_t)blockIdx.x * VG_VOXELS;
    for (;;) {
        __syncthreads();
        if (tid == 0) s_job = atomicAdd(status + 1, 1);
        __syncthreads();
        const int g = s_job;
        if (g >= n_jobs) return;
        const int b = segment_of(bone_ptr, n_meshes, g);  // mesh b with bone_ptr[b] <= g < bone_ptr[b + 1]
        const int nb = bone_ptr[b + 1] - bone_ptr[b], bi = g - bone_ptr[b];
        const double tx = vox_tf[b * 5 + 0], ty = vox_tf[b * 5 + 1], tz = vox_tf[b * 5 + 2];
        const double scale = vox_tf[b * 5 + 3], dims0 = vox_tf[b * 5 + 4];
        const uint4* maskb = reinterpret_cast<const uint4*>(mask_bits) + (size_t)b * VG_ROWS;

        for (int r = tid; r < VG_ROWS; r += GEO_THREADS) s_reach[r] = make_uint4(0u, 0u, 0u, 0u);
        if (tid < 2) s_cnt[tid] = 0;
        if (tid == 0) s_tmp = 0;
        // seeds (one_bone :279-285 with mst_utils.sample_on_bone, step 0.01): p + (c - p) / (n + 1e-30) * i for i = 1 .. n - 1, and p
        const double* bn = bones + (size_t)g * 6;
        const double px = bn[0], py = bn[1], pz = bn[2], cx = bn[3], cy = bn[4], cz = bn[5];
        const double ex = px - cx, ey = py - cy, ez = pz - cz;
        const double ns = rint(sqrt((ex * ex + ey * ey) + ez * ez) / 0.01);
        if (!(ns <= (double)GEO_MAX_SAMPLES)) {
            if (tid == 0) atomicMax(status, GEO_ERR_SAMPLES);
            continue;                                    // uniform: every thread takes the branch
        }
        const long n_seed = ns >= 1.0 ? (long)ns : 1;    // samples 1 .. ns - 1 plus p itself
        const double den = ns + 1e-30;
        const double ux = (cx - px) / den, uy = (cy - py) / den, uz = (cz - pz) / den;
        __syncthreads();
        for (long i = tid; i < n_seed; i += GEO_THREADS) {
            double sx = px, sy = py, sz = pz;
            if (i > 0) { const double fi = (double)i; sx = px + ux * fi; sy = py + uy * fi; sz = pz + uz * fi; }
            const int vx = vox_coord(sx, tx, scale, dims0), vy = vox_coord(sy, ty, scale, dims0), vz = vox_coord(sz, tz, scale, dims0);
            atomicOr(reinterpret_cast<uint32_t*>(s_reach) + (vx * VG + vy) * 4 + (vz >> 5), 1u << (vz & 31));
            layer[(vx * VG + vy) * VG + vz] = 0;
        }
        __syncthreads();
        uint4 unf[GEO_RPT];                             // occupied & unreached, own rows
        int c = 0;
#pragma unroll
        for (int k = 0; k < GEO_RPT; ++k) {
            const int row = tid + k * GEO_THREADS;
            unf[k] = row < VG_ROWS ? andnot4(maskb[row], s_reach[row]) : make_uint4(0u, 0u, 0u, 0u);
            c += popc4(unf[k]);
        }
        int unfilled = block_sum(c, &s_tmp);            // exact count of occupied & unreached
        int last = unfilled;                            // the reference's num_unfilled_last
        int dist_bone = 1;
        int step = 0;
        bool failed = false;
        while (last > 0) {
            if (dist_bone > GEO_MAX_LAYER) { failed = true; break; }
            // phase A: this step's new voxels per own row, from the LDS image of the previous step; their layers are written and
            // `unf` updated at once (nobody reads either before the next barrier), the count goes to this step's counter
            const int par = step & 1;
            int cn = 0;
            unsigned changed = 0;
#pragma unroll
            for (int k = 0; k < GEO_RPT; ++k) {
                const int row = tid + k * GEO_THREADS;
                if (row < VG_ROWS && any4(unf[k])) {
                    const int x = row / VG, y = row % VG;
                    uint4 acc = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
                    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll 1
                        for (int dy = -1; dy <= 1; ++dy) acc = or4(acc, lds_row(s_reach, x + dx, y + dy));
                    const uint4 nw = and4(zdilate(acc), unf[k]);
                    if (any4(nw)) {
                        unf[k] = andnot4(unf[k], nw);
                        cn += popc4(nw);
                        changed |= 1u << k;
                        for (int w = 0; w < 3; ++w)
                            for (uint32_t m = word_of(nw, w); m; m &= m - 1)
                                layer[(size_t)row * VG + w * 32 + __ffs(m) - 1] = (uint16_t)dist_bone;
                    }
                }
            }
            for (int o = 32; o > 0; o >>= 1) cn += __shfl_xor(cn, o);
            if ((tid & 63) == 0 && cn) atomicAdd(&s_cnt[par], cn);
            __syncthreads();
            // phase B: reached = previous reached | (occupied & ~unf) on the changed own rows
            if (tid == 0) s_cnt[par ^ 1] = 0;           // read by everyone in the previous step, before this step's first barrier
#pragma unroll
            for (int k = 0; k < GEO_RPT; ++k) {
                if ((changed >> k) & 1u) {
                    const int row = tid + k * GEO_THREADS;
                    s_reach[row] = or4(s_reach[row], andnot4(maskb[row], unf[k]));
                }
            }
            __syncthreads();
            const int added = s_cnt[par];
            ++step;
            ++dist_bone;                                 // every dilation call counts, also one that reaches nothing
            unfilled -= added;
            const int this_count = unfilled;
            if (this_count == last) {
                const int np = geo_patch(s_reach, maskb, layer, list, s_small);
                unfilled -= np;
#pragma unroll
                for (int k = 0; k < GEO_RPT; ++k) {
                    const int row = tid + k * GEO_THREADS;
                    if (row < VG_ROWS) unf[k] = andnot4(maskb[row], s_reach[row]);
                }
            }
            last = this_count;                           // the count BEFORE the patch, as the reference sets it
        }
        if (failed) {
            if (tid == 0) atomicMax(status, GEO_ERR_LAYER);
            continue;
        }
        // distmap at the vertices' voxels; a voxel never reached reads 0 (calc_volumetric_geodesic :318-321, one_bone :314)
        const int vs = vtx_ptr[b], ve = vtx_ptr[b + 1];
        int32_t* out = dist + dist_off[b];
        for (int v = vs + tid; v < ve; v += GEO_THREADS) {
            const double* p = pos + (size_t)v * 3;
            const int vx = vox_coord(p[0], tx, scale, dims0), vy = vox_coord(p[1], ty, scale, dims0), vz = vox_coord(p[2], tz, scale, dims0);
            const uint32_t word = reinterpret_cast<const uint32_t*>(s_reach)[(vx * VG + vy) * 4 + (vz >> 5)];
            const int d = ((word >> (vz & 31)) & 1u) ? (int)layer[(vx * VG + vy) * VG + vz] : 0;
            out[(size_t)(v - vs) * nb + bi] = d;
        }
    }
}

// ---- bind rows (gen_skin_data.py:86-118) and what load_skin / the dataset make of them (dataset_rig.py:30-76, 94-101) ----
// One thread per vertex. Slot order: ascending D, ties by ascending bone id (a stable argsort). Labels: the weight of the bone's
// start joint when > 0 and not taken by an earlier slot.
__global__ void skin_bind_kernel(const int32_t* __restrict__ dist, const int64_t* __restrict__ dist_off, const int32_t* __restrict__ vtx_ptr,
                                 const int32_t* __restrict__ bone_ptr, int n_meshes, int n, const double* __restrict__ bones,
                                 const uint8_t* __restrict__ is_leaf, const int32_t* __restrict__ start_jid, const double* __restrict__ skins,
                                 int ld_skins, int k, int32_t* __restrict__ bind_ids, double* __restrict__ bind_invd,
                                 double* __restrict__ labels, float* __restrict__ skin_input, int64_t* __restrict__ skin_nn,
                                 int64_t* __restrict__ loss_mask, int64_t* __restrict__ skin_nnjids) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int b = segment_of(vtx_ptr, n_meshes, v), b0 = bone_ptr[b], nb = bone_ptr[b + 1] - b0;
    if (nb <= 0) return;                                 // refused by the host layer
    const int32_t* row = dist + dist_off[b] + (size_t)(v - vtx_ptr[b]) * nb;
    unsigned long long prev = 0, used = 0;
    int first = 0;
    for (int s = 0; s < k; ++s) {
        const size_t o = (size_t)v * k + s;
        int id = -1;
        double invd = 0.0, lab = 0.0;
        if (s < nb) {
            unsigned long long best = ~0ull;
            for (int j = 0; j < nb; ++j) {
                const unsigned long long key = ((unsigned long long)(uint32_t)row[j] << 32) | (uint32_t)j;
                if ((s == 0 || key > prev) && key < best) best = key;
            }
            prev = best;
            id = (int)(best & 0xffffffffu);
            invd = 1.0 / ((double)(int)(best >> 32) + 1e-10);
            if (skins) {
                const int jt = start_jid[b0 + id];
                const double w = skins[(size_t)v * ld_skins + jt];
                if (w > 0.0 && !((used >> jt) & 1ull)) { lab = w; used |= 1ull << jt; }
            }
        }
        if (s == 0) first = id;
        bind_ids[o] = id;
        bind_invd[o] = invd;
        if (labels) labels[o] = lab;
        // load_skin: an invalid slot repeats slot 0, masked out
        const bool valid = id != -1;
        const int t = valid ? id : first;
        const double tinv = valid ? invd : bind_invd[(size_t)v * k];
        const double* bo = bones + (size_t)(b0 + t) * 6;
        float* si = skin_input + o * 8;
        for (int c = 0; c < 6; ++c) si[c] = (float)bo[c];
        si[6] = (float)tinv;
        si[7] = is_leaf[b0 + t] ? 1.0f : 0.0f;
        skin_nn[o] = t;
        loss_mask[o] = valid ? 1 : 0;
        skin_nnjids[o] = start_jid[b0 + t];
    }
}

// ---- post-processing of SkinNet's logits (train_skin.py:232-244, joint2rig.py:447-462) ----
// mode 0 (train_skin): softmax over the k logits, then x loss_mask; mode 1 (joint2rig): logits x loss_mask, then softmax. float32, as
// torch computes it there. The slots with mask 1 are scattered into row v of P [n][ldp] (fp64, zeroed here) at skin_nn.
__global__ void skin_scatter_kernel(const float* __restrict__ logits, int ldl, const int64_t* __restrict__ skin_nn,
                                    const int64_t* __restrict__ loss_mask, const int64_t* __restrict__ batch, const int32_t* __restrict__ n_bones,
                                    int n, int k, int mode, double* __restrict__ P, int ldp) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const float* x = logits + (size_t)v * ldl;
    const int64_t* msk = loss_mask + (size_t)v * k;
    const int64_t* nn = skin_nn + (size_t)v * k;
    double* out = P + (size_t)v * ldp;
    const int nb = n_bones[batch[v]];
    for (int c = 0; c < ldp; ++c) out[c] = 0.0;
    float m = -INFINITY;
    for (int s = 0; s < k; ++s) { const float a = mode == 1 ? x[s] * (float)msk[s] : x[s]; m = fmaxf(m, a); }
    float sum = 0.0f;
    for (int s = 0; s < k; ++s) { const float a = mode == 1 ? x[s] * (float)msk[s] : x[s]; sum += expf(a - m); }
    for (int s = 0; s < k; ++s) {
        if (msk[s] != 1) continue;
        const float a = mode == 1 ? x[s] * (float)msk[s] : x[s];
        float p = expf(a - m) / sum;
        if (mode == 0) p = p * (float)msk[s];
        const int64_t t = nn[s];
        if (t >= 0 && t < nb && t < ldp) out[t] = (double)p;
    }
}

// post_filter (train_skin.py:40-66, num_ring = 1): row v = mean of the rows of its unique 1-ring neighbours (CSR, self excluded, summed
// in CSR order); a vertex without neighbours keeps its own row (the reference raises there). Then entries < ratio * row max -> 0 and
// division by row sum + 1e-10. fp64; columns at and past the mesh's bone count are 0.
__global__ void skin_filter_kernel(const double* __restrict__ P, int ldp, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                   const int64_t* __restrict__ batch, const int32_t* __restrict__ n_bones, int n, double ratio,
                                   double* __restrict__ W, int ldw) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int nb = min(n_bones[batch[v]], ldw);
    const int s0 = rowptr[v], s1 = rowptr[v + 1];
    double* out = W + (size_t)v * ldw;
    double mx = -INFINITY;
    for (int c = 0; c < nb; ++c) {
        double a;
        if (s1 > s0) {
            double acc = 0.0;
            for (int e = s0; e < s1; ++e) acc += P[(size_t)cols[e] * ldp + c];
            a = acc / (double)(s1 - s0);
        } else {
            a = P[(size_t)v * ldp + c];
        }
        out[c] = a;
        mx = fmax(mx, a);
    }
    const double thr = mx * ratio;
    double sum = 0.0;
    for (int c = 0; c < nb; ++c) {
        double a = out[c];
        if (a < thr) a = 0.0;
        out[c] = a;
        sum += a;
    }
    const double den = sum + 1e-10;
    for (int c = 0; c < nb; ++c) out[c] = out[c] / den;
    for (int c = nb; c < ldw; ++c) out[c] = 0.0;
}

}  // namespace morig

using namespace morig;

extern "C" int64_t morig_vol_geodesic_workspace(int32_t n_meshes, int32_t n_slots) {
    if (n_meshes < 0 || n_slots < 0) return MORIG_E_INVALID;
    // packed grids (uint32) + per slot a layer map (uint16) and a boundary list (uint32), in bytes
    return (int64_t)n_meshes * VG_WORDS * 4 + (int64_t)n_slots * VG_VOXELS * (2 + 4);
}

extern "C" int morig_vol_geodesic(const uint8_t* vox, int32_t n_meshes, const double* vox_tf, const double* pos, const int32_t* vtx_ptr,
                                  const double* bones, const int32_t* bone_ptr, int32_t n_jobs, const int64_t* dist_off, int32_t n_slots,
                                  void* workspace, int64_t workspace_bytes, int32_t* status, int32_t* dist, void* stream) {
    if (!vox || !vox_tf || !vtx_ptr || !bone_ptr || !dist_off || !status || n_meshes <= 0 || n_jobs < 0 || n_slots <= 0) return MORIG_E_INVALID;
    if (workspace_bytes < morig_vol_geodesic_workspace(n_meshes, n_slots) || !workspace) return MORIG_E_INVALID;
    if (n_jobs > 0 && (!bones || !dist || !pos)) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), s));
    if (n_jobs == 0) return MORIG_OK;
    uint32_t* bits = reinterpret_cast<uint32_t*>(workspace);
    uint16_t* layer = reinterpret_cast<uint16_t*>(bits + (size_t)n_meshes * VG_WORDS);
    uint32_t* list = reinterpret_cast<uint32_t*>(layer + (size_t)n_slots * VG_VOXELS);
    hipLaunchKernelGGL(vox_pack_kernel, dim3(cdiv((long)n_meshes * VG_WORDS, 256)), dim3(256), 0, s, vox, n_meshes, bits);
    MORIG_LAUNCH_CHECK();
    const int grid = n_slots < n_jobs ? n_slots : n_jobs;
    hipLaunchKernelGGL(vol_geodesic_kernel, dim3(grid), dim3(GEO_THREADS), 0, s, bits, vox_tf, pos, vtx_ptr, bones, bone_ptr, n_meshes,
                       dist_off, n_jobs, layer, list, status, dist);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skin_bind(const int32_t* dist, const int64_t* dist_off, const int32_t* vtx_ptr, const int32_t* bone_ptr, int32_t n_meshes,
                               int32_t n_vertices, const double* bones, const uint8_t* is_leaf, const int32_t* start_jid, const double* skins,
                               int32_t ld_skins, int32_t k, int32_t* bind_ids, double* bind_invd, double* labels, float* skin_input,
                               int64_t* skin_nn, int64_t* loss_mask, int64_t* skin_nnjids, void* stream) {
    if (!dist || !dist_off || !vtx_ptr || !bone_ptr || !bones || !is_leaf || !start_jid || !bind_ids || !bind_invd || !skin_input ||
        !skin_nn || !loss_mask || !skin_nnjids || n_meshes <= 0 || n_vertices < 0 || k < 1) return MORIG_E_INVALID;
    if ((skins != nullptr) != (labels != nullptr) || (skins && ld_skins < 1)) return MORIG_E_INVALID;
    if (n_vertices == 0) return MORIG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(skin_bind_kernel, dim3(cdiv(n_vertices, 128)), dim3(128), 0, s, dist, dist_off, vtx_ptr, bone_ptr, n_meshes, n_vertices,
                       bones, is_leaf, start_jid, skins, ld_skins, k, bind_ids, bind_invd, labels, skin_input, skin_nn, loss_mask, skin_nnjids);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skin_scatter(const float* logits, int32_t ldl, const int64_t* skin_nn, const int64_t* loss_mask, const int64_t* batch,
                                  const int32_t* n_bones, int32_t n, int32_t k, int32_t mode, double* P, int32_t ldp, void* stream) {
    if (!logits || !skin_nn || !loss_mask || !batch || !n_bones || !P || n < 0 || k < 1 || ldl < k || ldp < 1 || (mode != 0 && mode != 1))
        return MORIG_E_INVALID;
    if (n == 0) return MORIG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(skin_scatter_kernel, dim3(cdiv(n, 128)), dim3(128), 0, s, logits, ldl, skin_nn, loss_mask, batch, n_bones, n, k, mode, P, ldp);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_skin_filter(const double* P, int32_t ldp, const int32_t* rowptr, const int32_t* cols, const int64_t* batch,
                                 const int32_t* n_bones, int32_t n, double ratio, double* W, int32_t ldw, void* stream) {
    if (!P || !rowptr || !batch || !n_bones || !W || n < 0 || ldp < 1 || ldw < 1) return MORIG_E_INVALID;
    if (n == 0) return MORIG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    hipLaunchKernelGGL(skin_filter_kernel, dim3(cdiv(n, 128)), dim3(128), 0, s, P, ldp, rowptr, cols, batch, n_bones, n, ratio, W, ldw);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
