// Depth scans (morig_amd/scan.py): from posed vertices, faces and cameras to depth images, partial point clouds,
// the visibility mask of the vertices and the nearest-neighbour correspondences between the two. A VIEW is one (mesh, frame, camera): it
// owns a block of vertex rows (vptr), names the mesh whose faces it draws (views[v][0], fptr) and a camera (cams[v], csrc/raytri_core.h).
// Everything is float64 in the written order of operations (contraction off) or integer. The only atomic is the 64-bit integer atomicMin
// of the rasteriser, whose result does not depend on order: two runs give the same bits, and a view alone gives the bits it gives inside
// a batch.
//
// raster      one wave per (view, triangle): the pixel box of the projected corners, padded by one pixel and clamped (the whole image when
//             a pinhole corner has depth <= near or a projection is no finite number), lanes striding over its pixels, every pixel through
//             raytri_core.h; a hit takes the minimum of (bits of float32(t) << 32 | face) into the view's key image (all ones = no hit).
//             A wave per triangle keeps the 64 lanes on one triangle's box: the boxes of a scan differ by orders of magnitude (a far
//             limb against a torso facing the camera), which a thread per triangle would turn into divergence; one triangle covering a
//             256 x 256 image is 1024 steps of one wave. A triangle with a coordinate that is no finite number sets nothing.
// resolve     one thread per pixel: key -> face, then t, and the point o + t d recomputed in float64 from the winning face; a hit flag.
// compact     one thread per pixel: the flagged pixels to their rank (the caller's inclusive prefix sum), in row-major pixel order.
// visibility  one thread per (view, vertex); the view's triangles pass through LDS in tiles of 256 (the idiom of bone_visibility_kernel in
//             geodesic.hip). Visible: inside the image rectangle, depth > near, and no face that does not name the vertex meets the segment
//             from the camera point c to the vertex at 0 < t < 1 with t |d| < |d| - vis_eps.
// nearest     one thread per query row of a ragged batch, the segment's target rows (optionally masked) through LDS in tiles of 256:
//             the lowest index among the nearest by (dx^2 + dy^2) + dz^2, or -1.
// Face indices are clamped into the view's vertex block, so no read leaves a buffer; check_faces raises the status word for the host.
#include "common.h"

#pragma clang fp contract(off)                 // in front of raytri_core.h: the pragma holds from here on, and the rules live in that header

#include "raytri_core.h"

namespace morig {

namespace {

using morig_raytri::Num;
constexpr int CAM = MORIG_SCAN_CAM_DOUBLES;
constexpr int VIEW = MORIG_SCAN_VIEW_INTS;
constexpr int TILE = 256;
constexpr unsigned long long NO_HIT = ~0ull;

struct ViewInfo { int mesh, W, H, kind, v0, nv, f0, nf; long long k0; bool ok; };

__device__ __forceinline__ ViewInfo view_info(const int* __restrict__ views, const int* __restrict__ vptr, const int* __restrict__ fptr,
                                              const long long* __restrict__ kptr, int n_meshes, int v) {
    ViewInfo i;
    i.mesh = views[(size_t)v * VIEW]; i.W = views[(size_t)v * VIEW + 1]; i.H = views[(size_t)v * VIEW + 2]; i.kind = views[(size_t)v * VIEW + 3];
    i.v0 = vptr[v]; i.nv = vptr[v + 1] - i.v0;
    i.ok = i.mesh >= 0 && i.mesh < n_meshes && i.W >= 1 && i.W <= MORIG_SCAN_MAX_SIDE && i.H >= 1 && i.H <= MORIG_SCAN_MAX_SIDE &&
           (i.kind == MORIG_SCAN_ORTHOGRAPHIC || i.kind == MORIG_SCAN_PINHOLE) && i.nv >= 0;
    i.f0 = i.nf = 0; i.k0 = 0;
    if (i.ok) {
        i.f0 = fptr[i.mesh]; i.nf = fptr[i.mesh + 1] - i.f0;
        if (kptr) { i.k0 = kptr[v]; i.ok = kptr[v + 1] - i.k0 == (long long)i.W * i.H; }
    }
    return i;
}

// the corners of face `tri` of the view, indices clamped into its vertex block (nv >= 1)
__device__ __forceinline__ void load_tri(const double* __restrict__ verts, const int* __restrict__ faces, const ViewInfo& vi, int tri, double (*P)[3],
                                         int* id) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        id[k] = min(max(faces[(size_t)(vi.f0 + tri) * 3 + k], 0), vi.nv - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) P[k][c] = verts[(size_t)(vi.v0 + id[k]) * 3 + c];
    }
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ------------------------------------------------------------------------------------------------------------------------ face check
__global__ void __launch_bounds__(256) check_faces_kernel(const int* __restrict__ faces, int n_faces, const int* __restrict__ fptr,
                                                          const int* __restrict__ mesh_nv, int n_meshes, int* __restrict__ status) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int nv = mesh_nv[segment_of(fptr, n_meshes, f)];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int id = faces[(size_t)f * 3 + k];
        if (id < 0 || id >= nv) *status = MORIG_SCAN_BAD_FACE;                          // every writer stores the same word
    }
}

// ------------------------------------------------------------------------------------------------------------------------ raster
__global__ void __launch_bounds__(256) scan_raster_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                          const int* __restrict__ fptr, const double* __restrict__ cams, const int* __restrict__ views,
                                                          const long long* __restrict__ kptr, const long long* __restrict__ wptr, int n_views,
                                                          int n_meshes, long long n_work, unsigned long long* __restrict__ keys) {
    const long long w = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_work) return;
    const int v = segment_of(wptr, n_views, w);
    const ViewInfo vi = view_info(views, vptr, fptr, kptr, n_meshes, v);
    const long long tri = w - wptr[v];
    if (!vi.ok || vi.nv < 1 || tri < 0 || tri >= vi.nf) return;
    double P[3][3];
    int id[3];
    load_tri(verts, faces, vi, (int)tri, P, id);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (!morig_raytri::is_finite(P[k][c])) return;
    const double* cam = cams + (size_t)v * CAM;
    const double near = cam[14];
    bool whole = false;
    double jl = INFINITY, jh = -INFINITY, il = INFINITY, ih = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double de[3] = {P[k][0] - cam[0], P[k][1] - cam[1], P[k][2] - cam[2]};
        double a = dot3(de, cam + 6), b = dot3(de, cam + 9);
        if (vi.kind == MORIG_SCAN_PINHOLE) {
            const double z = dot3(de, cam + 3);
            if (!(z > near)) whole = true;
            a = a / z; b = b / z;
        }
        const double jf = (a / cam[12] + (double)(vi.W - 1)) * 0.5, rf = ((double)(vi.H - 1) - b / cam[13]) * 0.5;
        if (!morig_raytri::is_finite(jf) || !morig_raytri::is_finite(rf)) whole = true;
        jl = fmin(jl, jf); jh = fmax(jh, jf); il = fmin(il, rf); ih = fmax(ih, rf);
    }
    int j0 = 0, j1 = vi.W - 1, i0 = 0, i1 = vi.H - 1;
    if (!whole) {
        const double ja = floor(jl) - 1.0, jz = ceil(jh) + 1.0, ia = floor(il) - 1.0, iz = ceil(ih) + 1.0;
        if (jz < 0.0 || ja > (double)(vi.W - 1) || iz < 0.0 || ia > (double)(vi.H - 1)) return;
        j0 = (int)fmax(ja, 0.0); j1 = (int)fmin(jz, (double)(vi.W - 1));
        i0 = (int)fmax(ia, 0.0); i1 = (int)fmin(iz, (double)(vi.H - 1));
    }
    const int ew = j1 - j0 + 1, eh = i1 - i0 + 1;
    const int count = ew * eh;                                                          // at most 1024^2
    unsigned long long* image = keys + vi.k0;
    for (int q = lane; q < count; q += 64) {
        const int i = i0 + q / ew, j = j0 + q % ew;
        double o[3], d[3], t;
        morig_raytri::pixel_ray(cam, vi.kind, vi.W, vi.H, i, j, o, d);
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
        if (morig_raytri::hit(n, near, t)) {
            const unsigned long long key = ((unsigned long long)__float_as_uint((float)t) << 32) | (unsigned long long)(unsigned)tri;
            atomicMin(image + (size_t)i * vi.W + j, key);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ resolve, compact
__global__ void __launch_bounds__(256) scan_resolve_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                           const int* __restrict__ fptr, const double* __restrict__ cams, const int* __restrict__ views,
                                                           const long long* __restrict__ kptr, int n_views, int n_meshes, long long n_pixels,
                                                           const unsigned long long* __restrict__ keys, double* __restrict__ depth,
                                                           int* __restrict__ face, double* __restrict__ point, int* __restrict__ flags) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_pixels) return;
    const int v = segment_of(kptr, n_views, q);
    const ViewInfo vi = view_info(views, vptr, fptr, kptr, n_meshes, v);
    double t = INFINITY, p[3] = {INFINITY, INFINITY, INFINITY};
    int tri = -1;
    const unsigned long long key = keys[q];
    const long long local = q - vi.k0;
    if (vi.ok && vi.nv >= 1 && key != NO_HIT && local >= 0 && local < (long long)vi.W * vi.H && (long long)(key & 0xffffffffull) < vi.nf) {
        tri = (int)(key & 0xffffffffull);
        double P[3][3], o[3], d[3];
        int id[3];
        load_tri(verts, faces, vi, tri, P, id);
        morig_raytri::pixel_ray(cams + (size_t)v * CAM, vi.kind, vi.W, vi.H, (int)(local / vi.W), (int)(local % vi.W), o, d);
        const Num n = morig_raytri::numerators(o, d, P[0], P[1], P[2]);
        t = n.tn / n.det;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = o[c] + t * d[c];
    }
    depth[q] = t;
    face[q] = tri;
    flags[q] = tri >= 0 ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) point[(size_t)q * 3 + c] = p[c];
}

// rank: the inclusive prefix sum of flags
__global__ void __launch_bounds__(256) scan_compact_kernel(const double* __restrict__ point, const int* __restrict__ face, const int* __restrict__ flags,
                                                           const long long* __restrict__ rank, const long long* __restrict__ kptr, int n_views,
                                                           long long n_pixels, long long n_hits, double* __restrict__ pts, int* __restrict__ pixel,
                                                           int* __restrict__ hit_face) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_pixels || !flags[q]) return;
    const long long at = rank[q] - 1;
    if (at < 0 || at >= n_hits) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[(size_t)at * 3 + c] = point[(size_t)q * 3 + c];
    pixel[at] = (int)(q - kptr[segment_of(kptr, n_views, q)]);
    hit_face[at] = face[q];
}

// ------------------------------------------------------------------------------------------------------------------------ visibility
__global__ void __launch_bounds__(TILE) scan_visibility_kernel(const double* __restrict__ verts, const int* __restrict__ vptr, const int* __restrict__ faces,
                                                               const int* __restrict__ fptr, const double* __restrict__ cams, const int* __restrict__ views,
                                                               const int* __restrict__ blk_ptr, int n_views, int n_meshes, double vis_eps,
                                                               unsigned char* __restrict__ vis) {
    __shared__ double s_tri[TILE][9];
    __shared__ int s_id[TILE][3];
    const BlockRow at = block_row(blk_ptr, n_views, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const ViewInfo vi = view_info(views, vptr, fptr, nullptr, n_meshes, at.seg);
    const long long lv = at.row;
    const bool live = lv >= 0 && lv < vi.nv;                                            // uniform per block: vi.ok, vi.nf
    if (!vi.ok) { if (live) vis[(size_t)vi.v0 + lv] = 0; return; }
    const double* cam = cams + (size_t)at.seg * CAM;
    double c[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, len = 0.0;
    bool seen = false;
    if (live) {
        const double* p = verts + ((size_t)vi.v0 + lv) * 3;
        const double de[3] = {p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]};
        const double z = dot3(de, cam + 3);
        double a = dot3(de, cam + 6), b = dot3(de, cam + 9);
        if (vi.kind == MORIG_SCAN_PINHOLE) { a = a / z; b = b / z; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = vi.kind == MORIG_SCAN_PINHOLE ? cam[k] : p[k] - z * cam[3 + k];
            d[k] = p[k] - c[k];
        }
        len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        seen = z > cam[14] && fabs(a) <= (double)vi.W * cam[12] && fabs(b) <= (double)vi.H * cam[13];
    }
    for (int base = 0; base < vi.nf; base += TILE) {
        __syncthreads();
        if (base + (int)threadIdx.x < vi.nf && vi.nv >= 1) {
            double P[3][3];
            load_tri(verts, faces, vi, base + (int)threadIdx.x, P, s_id[threadIdx.x]);
#pragma unroll
            for (int k = 0; k < 9; ++k) s_tri[threadIdx.x][k] = P[k / 3][k % 3];
        }
        __syncthreads();
        const int m = min(TILE, vi.nf - base);
        if (seen)
            for (int j = 0; j < m; ++j) {
                if (s_id[j][0] == lv || s_id[j][1] == lv || s_id[j][2] == lv) continue;
                const double* T = s_tri[j];
                const Num n = morig_raytri::numerators(c, d, T, T + 3, T + 6);
                if (!morig_raytri::inside(n)) continue;
                const double t = n.tn / n.det;
                if (t > 0.0 && t < 1.0 && t * len < len - vis_eps) { seen = false; break; }
            }
    }
    if (live) vis[(size_t)vi.v0 + lv] = seen ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------------ nearest
__global__ void __launch_bounds__(TILE) scan_nearest_kernel(const double* __restrict__ q, const int* __restrict__ qptr, const double* __restrict__ t,
                                                            const int* __restrict__ tptr, const unsigned char* __restrict__ mask,
                                                            const int* __restrict__ blk_ptr, int n_segs, int* __restrict__ idx, double* __restrict__ d2) {
    __shared__ double s_t[TILE][3];
    __shared__ unsigned char s_m[TILE];
    const BlockRow at = block_row(blk_ptr, n_segs, (int)blockIdx.x, (int)threadIdx.x, TILE);
    const int b = at.seg, q0 = qptr[b], nq = qptr[b + 1] - q0, t0 = tptr[b], nt = tptr[b + 1] - t0;
    const long long lq = at.row;
    const bool live = lq >= 0 && lq < nq;
    double x = 0.0, y = 0.0, z = 0.0, best = INFINITY;
    int bi = -1;
    if (live) { x = q[((size_t)q0 + lq) * 3]; y = q[((size_t)q0 + lq) * 3 + 1]; z = q[((size_t)q0 + lq) * 3 + 2]; }
    for (int base = 0; base < nt; base += TILE) {
        __syncthreads();
        const int j = base + (int)threadIdx.x;
        if (j < nt) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s_t[threadIdx.x][c] = t[((size_t)t0 + j) * 3 + c];
            s_m[threadIdx.x] = mask ? mask[(size_t)t0 + j] : 1;
        }
        __syncthreads();
        const int m = min(TILE, nt - base);
        if (live)
            for (int k = 0; k < m; ++k) {
                if (!s_m[k]) continue;
                const double dx = x - s_t[k][0], dy = y - s_t[k][1], dz = z - s_t[k][2];
                const double dd = (dx * dx + dy * dy) + dz * dz;
                if (dd < best) { best = dd; bi = base + k; }                            // strict: the lowest index among equals
            }
    }
    if (live) { idx[(size_t)q0 + lq] = bi; d2[(size_t)q0 + lq] = best; }
}

}  // namespace

}  // namespace morig

using namespace morig;

extern "C" {

int morig_scan_raster(const double* verts, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* mesh_nv,
                      const double* cams, const int32_t* views, const int64_t* kptr, const int64_t* wptr, int32_t n_views, int32_t n_meshes,
                      int32_t min_side, int32_t max_side, int64_t n_pixels, int64_t n_work, uint64_t* keys, int32_t* status, void* stream) {
    if (n_views < 0 || n_meshes < 0 || n_faces < 0 || n_pixels < 0 || n_work < 0) return MORIG_E_INVALID;
    if (n_views > 0 && (min_side < 1 || max_side > MORIG_SCAN_MAX_SIDE)) return MORIG_E_UNSUPPORTED;
    if (n_work > (((int64_t)1 << 31) - 1) * 4) return MORIG_E_UNSUPPORTED;
    if (!status) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MORIG_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (n_views == 0 || n_pixels == 0) return MORIG_OK;
    if (!vptr || !fptr || !cams || !views || !kptr || !wptr || !keys || n_meshes == 0) return MORIG_E_INVALID;
    MORIG_HIP_TRY(hipMemsetAsync(keys, 0xff, (size_t)n_pixels * sizeof(uint64_t), s));
    if (n_faces == 0) return MORIG_OK;
    if (!faces || !mesh_nv) return MORIG_E_INVALID;
    ProfScope ps(K_SCAN_RASTER, s, 0.0, 0.0);
    check_faces_kernel<<<cdiv(n_faces, 256), 256, 0, s>>>(faces, n_faces, fptr, mesh_nv, n_meshes, status);
    MORIG_LAUNCH_CHECK();
    if (!verts || n_work == 0) return MORIG_OK;                                          // no view has a vertex: nothing to draw
    scan_raster_kernel<<<cdiv(n_work, 4), 256, 0, s>>>(verts, vptr, faces, fptr, cams, views, (const long long*)kptr, (const long long*)wptr, n_views,
                                                       n_meshes, n_work, (unsigned long long*)keys);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_scan_resolve(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams, const int32_t* views,
                       const int64_t* kptr, int32_t n_views, int32_t n_meshes, int64_t n_pixels, const uint64_t* keys, double* depth, int32_t* face,
                       double* point, int32_t* flags, void* stream) {
    if (n_views < 0 || n_meshes < 0 || n_pixels < 0 || n_pixels > ((int64_t)1 << 31) * 128) return MORIG_E_INVALID;
    if (n_pixels == 0) return MORIG_OK;
    if (!vptr || !fptr || !cams || !views || !kptr || !keys || !depth || !face || !point || !flags || n_views == 0 || n_meshes == 0)
        return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SCAN, s, 0.0, 52.0 * (double)n_pixels);
    scan_resolve_kernel<<<cdiv(n_pixels, 256), 256, 0, s>>>(verts, vptr, faces, fptr, cams, views, (const long long*)kptr, n_views, n_meshes, n_pixels,
                                                            (const unsigned long long*)keys, depth, face, point, flags);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_scan_compact(const double* point, const int32_t* face, const int32_t* flags, const int64_t* rank, const int64_t* kptr, int32_t n_views,
                       int64_t n_pixels, int64_t n_hits, double* pts, int32_t* pixel, int32_t* hit_face, void* stream) {
    if (n_views < 0 || n_pixels < 0 || n_hits < 0 || n_hits > n_pixels || n_pixels > ((int64_t)1 << 31) * 128) return MORIG_E_INVALID;
    if (n_pixels == 0 || n_hits == 0) return MORIG_OK;
    if (!point || !face || !flags || !rank || !kptr || !pts || !pixel || !hit_face || n_views == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SCAN, s, 0.0, 12.0 * (double)n_pixels + 64.0 * (double)n_hits);
    scan_compact_kernel<<<cdiv(n_pixels, 256), 256, 0, s>>>(point, face, flags, (const long long*)rank, (const long long*)kptr, n_views, n_pixels, n_hits,
                                                            pts, pixel, hit_face);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_scan_visibility(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams, const int32_t* views,
                          const int32_t* blk_ptr, int32_t n_views, int32_t n_meshes, int32_t n_blocks, double vis_eps, uint8_t* vis, void* stream) {
    if (n_views < 0 || n_meshes < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!verts || !vptr || !fptr || !cams || !views || !blk_ptr || !vis || n_views == 0 || n_meshes == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SCAN, s, 0.0, 0.0);
    scan_visibility_kernel<<<n_blocks, TILE, 0, s>>>(verts, vptr, faces, fptr, cams, views, blk_ptr, n_views, n_meshes, vis_eps, vis);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

int morig_scan_nearest(const double* q, const int32_t* qptr, const double* t, const int32_t* tptr, const uint8_t* mask, const int32_t* blk_ptr,
                       int32_t n_segs, int32_t n_blocks, int32_t* idx, double* d2, void* stream) {
    if (n_segs < 0 || n_blocks < 0) return MORIG_E_INVALID;
    if (n_blocks == 0) return MORIG_OK;
    if (!q || !qptr || !tptr || !blk_ptr || !idx || !d2 || n_segs == 0) return MORIG_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(K_SCAN, s, 0.0, 0.0);
    scan_nearest_kernel<<<n_blocks, TILE, 0, s>>>(q, qptr, t, tptr, mask, blk_ptr, n_segs, idx, d2);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // extern "C"
