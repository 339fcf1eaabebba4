// Rig tracking (evaluate/eval_tracking.py:56-154 on utils/deform_ik.py): the batched inverse-kinematics solver and the per-point
// winner of the correspondence selection.
//
// ik_solve_kernel: ONE workgroup per problem, all iter_time Adam iterations inside the launch, workgroup barriers only. Per iteration
//   A  per joint: sin / cos of the three angles, R = Rx (Ry Rz), locals = R locals_in                                   1 barrier
//   B  forward kinematics, one tree level per step, parent first (level 0 = the root)                                   1 barrier / level
//   C  per vertex: out = sum_e w_e (G_j x_e + jpos_j) over its skin entries (streamed from L2), residual
//      r = 2 mask (out - c) / (3 V) into LDS                                                                            1 barrier
//   D  per joint (one wave each, round robin): the 12 sums  sum_e w_e r_v [x_e^T | 1]  over the joint-sorted copy of the
//      entries, float64, lanes in a fixed order, shuffle tree                                                           1 barrier
//   E  the tree child first: a parent adds its children's  gG_c L_c^T + gp_c offset_c^T  and  gp_c                      1 barrier / level - 1
//   F  per joint: gL = G_parent^T gG, gR = gL locals_in^T, the three angle derivatives, then torch's Adam step in float32
// = 2 levels + 2 barriers per iteration. The forward is float32 as the reference's; every sum over vertices and the backward through
// the tree are float64. No floating-point atomics: two runs are bit-identical. Everything per joint, the residuals and the Adam state
// live in LDS, sized from the largest problem of the launch; a launch that does not fit is refused (MORIG_E_UNSUPPORTED).
#include "common.h"

namespace morig {

struct IkParams {
    const int* joint_ptr; const int* vert_ptr; const int* level_off;
    const float* locals_in; const float* offsets; const int* parent; const int* order; const int* level_ptr; const int* child_lo;
    const int* child_hi;
    const int* vptr; const int* vent_j; const float4* vent_xw;
    const int* jptr; const int* jent_v; const float4* jent_xw;
    long n_entries;
    const float* constraints; const float* vismask;
    const int* root; const int* iter_time; const double* lr; const float* w_invis; const float* thrd;
    const double* bias1; const double* bias2_sqrt;
    int max_joints, max_vertices, max_iter;
    float* angles; float* trans; float* locals; float* globals; float* jpos; float* loss; float* grad_angles; float* grad_trans;
    int* status;
};

// floats per joint in LDS: locals_in 9, offset 3, locals 9, globals 9, jpos 3, sin/cos 6; per parameter slot (joints + translation): value,
// first and second moment, gradient
constexpr int IK_JOINT_FLOATS = 39, IK_SLOT_FLOATS = 12;
constexpr size_t IK_STATIC_LDS = 512;                       // what the kernel declares besides (the barrier-with-vote scratch)
__host__ __device__ inline size_t ik_lds_bytes(int max_joints, int max_vertices, int threads) {
    const size_t J = (size_t)max_joints, V = (size_t)max_vertices;
    return sizeof(double) * (J * 12 + threads / 64) + sizeof(float) * (J * IK_JOINT_FLOATS + (J + 1) * IK_SLOT_FLOATS + V * 3) +
           sizeof(int) * (J * 4 + (J + 1));
}

template <class A, class B, class C>
__device__ __forceinline__ void mul33(const A* a, const B* b, C* c) {             // c = a b
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i * 3 + k] = (C)a[i * 3] * (C)b[k] + (C)a[i * 3 + 1] * (C)b[3 + k] + (C)a[i * 3 + 2] * (C)b[6 + k];
}
template <class A, class B, class C>
__device__ __forceinline__ void mul33_bt(const A* a, const B* b, C* c) {          // c = a b^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i * 3 + k] = (C)a[i * 3] * (C)b[k * 3] + (C)a[i * 3 + 1] * (C)b[k * 3 + 1] + (C)a[i * 3 + 2] * (C)b[k * 3 + 2];
}
template <class A, class B, class C>
__device__ __forceinline__ void mul33_at(const A* a, const B* b, C* c) {          // c = a^T b
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i * 3 + k] = (C)a[i] * (C)b[k] + (C)a[3 + i] * (C)b[3 + k] + (C)a[6 + i] * (C)b[6 + k];
}
template <class T> __device__ __forceinline__ void axis_x(T c, T s, bool deriv, T* m) {
    const T a = deriv ? -s : c, b = deriv ? c : s;                                 // d/dt (cos, sin) = (-sin, cos)
    m[0] = deriv ? (T)0 : (T)1; m[1] = 0; m[2] = 0; m[3] = 0; m[4] = a; m[5] = -b; m[6] = 0; m[7] = b; m[8] = a;
}
template <class T> __device__ __forceinline__ void axis_y(T c, T s, bool deriv, T* m) {
    const T a = deriv ? -s : c, b = deriv ? c : s;
    m[0] = a; m[1] = 0; m[2] = b; m[3] = 0; m[4] = deriv ? (T)0 : (T)1; m[5] = 0; m[6] = -b; m[7] = 0; m[8] = a;
}
template <class T> __device__ __forceinline__ void axis_z(T c, T s, bool deriv, T* m) {
    const T a = deriv ? -s : c, b = deriv ? c : s;
    m[0] = a; m[1] = -b; m[2] = 0; m[3] = b; m[4] = a; m[5] = 0; m[6] = 0; m[7] = 0; m[8] = deriv ? (T)0 : (T)1;
}
__device__ __forceinline__ double dot9(const double* a, const double* b) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) s += a[i] * b[i];
    return s;
}

// torch.optim.Adam's single-tensor step in its float32 operation order (betas 0.9 / 0.999, eps 1e-8, L2 weight decay 1e-4 added to the
// gradient): g' = fma(wd, p, g); m = fma(1 - b1, g' - m, m); v = fma((1 - b2) g', g', b2 v); p += (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps).
// bc1 and sqrt(bc2) arrive as float64 tables, lr / bc1 is a float64 quotient rounded once, as the Python scalars of the reference are.
__device__ __forceinline__ void adam_step(float g, float& p, float& m, float& v, double lr, double bc1, double bc2_sqrt) {
    const float gd = fmaf(1e-4f, p, g);
    m = fmaf((float)(1.0 - 0.9), gd - m, m);
    v = fmaf((float)(1.0 - 0.999) * gd, gd, v * 0.999f);
    const float denom = sqrtf(v) / (float)bc2_sqrt + 1e-8f;
    p = p + ((float)(-(lr / bc1)) * m) / denom;
}

template <int NT>
__global__ __launch_bounds__(NT) void ik_solve_kernel(const IkParams p) {
    extern __shared__ double ik_smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = NT / 64;
    const int j0 = p.joint_ptr[b], J = p.joint_ptr[b + 1] - j0;
    const int v0 = p.vert_ptr[b], V = p.vert_ptr[b + 1] - v0;
    const int lv0 = p.level_off[b], nlev = p.level_off[b + 1] - lv0 - 1;
    const int root = p.root[b], T = p.iter_time[b];
    // sizes first (uniform per workgroup): nothing below indexes LDS or global memory past what they promise
    if (J < 1 || J > p.max_joints || V < 1 || V > p.max_vertices || nlev < 1 || nlev > J || root < 0 || root >= J || T < 1 || T > p.max_iter) {
        if (tid == 0) p.status[b] = 1;
        return;
    }
    const int Jm = p.max_joints;
    double* gacc = ik_smem;                                   // [J][12]: dL/dG (9), dL/djpos (3)
    double* red = gacc + (size_t)Jm * 12;                     // [NW]
    float* sL0 = reinterpret_cast<float*>(red + NW);          // [J][9]
    float* sOff = sL0 + Jm * 9;                               // [J][3]
    float* sL = sOff + Jm * 3;                                // [J][9]
    float* sG = sL + Jm * 9;                                  // [J][9]
    float* sP = sG + Jm * 9;                                  // [J][3]
    float* sSC = sP + Jm * 3;                                 // [J][6]: sin x y z, cos x y z
    float* sPar = sSC + Jm * 6;                               // [J + 1][3]: angles, then the translation
    float* sM = sPar + (Jm + 1) * 3;
    float* sV = sM + (Jm + 1) * 3;
    float* sGrad = sV + (Jm + 1) * 3;
    int* sParent = reinterpret_cast<int*>(sGrad + (Jm + 1) * 3);
    int* sOrder = sParent + Jm;
    int* sLo = sOrder + Jm;
    int* sHi = sLo + Jm;
    int* sLev = sHi + Jm;                                     // [nlev + 1] <= [J + 1]
    float* sRes = reinterpret_cast<float*>(sLev + Jm + 1);    // [V][3]

    // ---- load and check the problem: every index that is used as an address below is proven in range here
    int bad = 0;
    for (int i = tid; i < J * 9; i += NT) sL0[i] = p.locals_in[(size_t)j0 * 9 + i];
    for (int i = tid; i < J * 3; i += NT) sOff[i] = p.offsets[(size_t)j0 * 3 + i];
    for (int j = tid; j < J; j += NT) {
        const int pa = p.parent[j0 + j], o = p.order[j0 + j], lo = p.child_lo[j0 + j], hi = p.child_hi[j0 + j];
        bad |= (pa < -1 || pa >= J || pa == j || (pa < 0) != (j == root) || o < 0 || o >= J || lo < 0 || hi < lo || hi > J);
        sParent[j] = pa; sOrder[j] = o; sLo[j] = lo; sHi[j] = hi;
        const long e0 = p.jptr[j0 + j], e1 = p.jptr[j0 + j + 1];
        bad |= (e0 < 0 || e1 < e0 || e1 > p.n_entries);
    }
    for (int l = tid; l <= nlev; l += NT) {
        const int a = p.level_ptr[lv0 + l];
        bad |= (a < 0 || a > J || (l == 0 && a != 0) || (l == nlev && a != J) || (l > 0 && a < p.level_ptr[lv0 + l - 1]));
        sLev[l] = a;
    }
    for (int v = tid; v < V; v += NT) {
        const long e0 = p.vptr[v0 + v], e1 = p.vptr[v0 + v + 1];
        const bool okr = !(e0 < 0 || e1 < e0 || e1 > p.n_entries);
        bad |= !okr;
        if (okr) for (long e = e0; e < e1; ++e) { const int j = p.vent_j[e]; bad |= (j < 0 || j >= J); }
    }
    for (int i = tid; i < (J + 1) * 3; i += NT) { sPar[i] = 0.01f; sM[i] = 0.f; sV[i] = 0.f; sGrad[i] = 0.f; }
    bad = __syncthreads_or(bad);
    if (!bad) {
        for (int j = wave; j < J; j += NW)
            for (long e = p.jptr[j0 + j] + lane; e < p.jptr[j0 + j + 1]; e += 64) { const int v = p.jent_v[e]; bad |= (v < 0 || v >= V); }
        for (int k = tid; k < J; k += NT) bad |= (sOrder[k] == root) != (k == 0);
        bad = __syncthreads_or(bad);
    }
    if (bad) {
        if (tid == 0) p.status[b] = 2;
        return;
    }
    if (tid == 0) p.status[b] = 0;

    const float invN = 1.0f / (3.0f * (float)V), thrd = p.thrd[b], w_invis = p.w_invis[b];
    const double lr = p.lr[b], lr_angle = lr * 3.141592653589793;
    const float* cons = p.constraints + (size_t)v0 * 3;
    const float* vis = p.vismask + v0;

    for (int it = 0; it < T; ++it) {
        const bool last = it == T - 1;
        // ---- A: local frames
        for (int j = tid; j < J; j += NT) {
            float s[3], c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { s[k] = sinf(sPar[j * 3 + k]); c[k] = cosf(sPar[j * 3 + k]); sSC[j * 6 + k] = s[k]; sSC[j * 6 + 3 + k] = c[k]; }
            float rx[9], ry[9], rz[9], yz[9], r[9], l[9];
            axis_x(c[0], s[0], false, rx); axis_y(c[1], s[1], false, ry); axis_z(c[2], s[2], false, rz);
            mul33(ry, rz, yz); mul33(rx, yz, r); mul33(r, sL0 + j * 9, l);
#pragma unroll
            for (int i = 0; i < 9; ++i) sL[j * 9 + i] = l[i];
        }
        __syncthreads();
        // ---- B: forward kinematics, level by level
        for (int lev = 0; lev < nlev; ++lev) {
            for (int k = sLev[lev] + tid; k < sLev[lev + 1]; k += NT) {
                const int c = sOrder[k], pa = sParent[c];
                if (pa < 0) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) sG[c * 9 + i] = sL[c * 9 + i];
#pragma unroll
                    for (int i = 0; i < 3; ++i) sP[c * 3 + i] = sOff[c * 3 + i] + sPar[J * 3 + i];
                } else {
                    float g[9];
                    mul33(sG + pa * 9, sL + c * 9, g);
#pragma unroll
                    for (int i = 0; i < 9; ++i) sG[c * 9 + i] = g[i];
                    const float* gp = sG + pa * 9; const float* o = sOff + c * 3;
#pragma unroll
                    for (int i = 0; i < 3; ++i) sP[c * 3 + i] = (gp[i * 3] * o[0] + gp[i * 3 + 1] * o[1] + gp[i * 3 + 2] * o[2]) + sP[pa * 3 + i];
                }
            }
            __syncthreads();
        }
        // ---- C: skinning and residuals
        double lossacc = 0.0;
        for (int v = tid; v < V; v += NT) {
            const int e0 = p.vptr[v0 + v], e1 = p.vptr[v0 + v + 1];
            float ox = 0.f, oy = 0.f, oz = 0.f;
            for (int e = e0; e < e1; ++e) {
                const int j = p.vent_j[e];
                const float4 xw = p.vent_xw[e];
                const float* g = sG + j * 9; const float* q = sP + j * 3;
                ox += xw.w * ((g[0] * xw.x + g[1] * xw.y + g[2] * xw.z) + q[0]);
                oy += xw.w * ((g[3] * xw.x + g[4] * xw.y + g[5] * xw.z) + q[1]);
                oz += xw.w * ((g[6] * xw.x + g[7] * xw.y + g[8] * xw.z) + q[2]);
            }
            const float mk = vis[v] > thrd ? 1.0f : w_invis;
            const float dx = ox - cons[v * 3], dy = oy - cons[v * 3 + 1], dz = oz - cons[v * 3 + 2];
            const float sc = mk * invN;
            sRes[v * 3] = (2.0f * dx) * sc; sRes[v * 3 + 1] = (2.0f * dy) * sc; sRes[v * 3 + 2] = (2.0f * dz) * sc;
            if (last) lossacc += (double)mk * ((double)dx * dx + (double)dy * dy + (double)dz * dz);
        }
        if (last) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) lossacc += __shfl_xor(lossacc, o);
            if (lane == 0) red[wave] = lossacc;
        }
        __syncthreads();
        // ---- D: per-joint sums over the joint-sorted entries
        for (int j = wave; j < J; j += NW) {
            double a[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) a[k] = 0.0;
            const int e1 = p.jptr[j0 + j + 1];
            for (int e = p.jptr[j0 + j] + lane; e < e1; e += 64) {
                const int v = p.jent_v[e];
                const float4 xw = p.jent_xw[e];
                const double w = xw.w;
                const double rx = w * (double)sRes[v * 3], ry = w * (double)sRes[v * 3 + 1], rz = w * (double)sRes[v * 3 + 2];
                a[0] += rx * xw.x; a[1] += rx * xw.y; a[2] += rx * xw.z;
                a[3] += ry * xw.x; a[4] += ry * xw.y; a[5] += ry * xw.z;
                a[6] += rz * xw.x; a[7] += rz * xw.y; a[8] += rz * xw.z;
                a[9] += rx; a[10] += ry; a[11] += rz;
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o);
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 12; ++k) gacc[j * 12 + k] = a[k];
            }
        }
        __syncthreads();
        // ---- E: back through the tree, child first
        for (int lev = nlev - 2; lev >= 0; --lev) {
            for (int k = sLev[lev] + tid; k < sLev[lev + 1]; k += NT) {
                const int pa = sOrder[k];
                double g[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) g[i] = gacc[pa * 12 + i];
                for (int q = sLo[pa]; q < sHi[pa]; ++q) {
                    const int c = sOrder[q];
                    const double* gc = gacc + c * 12;
                    double t[9];
                    mul33_bt(gc, sL + c * 9, t);                                  // gG_c L_c^T
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int m = 0; m < 3; ++m) g[i * 3 + m] += t[i * 3 + m] + gc[9 + i] * (double)sOff[c * 3 + m];
                        g[9 + i] += gc[9 + i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 12; ++i) gacc[pa * 12 + i] = g[i];
            }
            __syncthreads();
        }
        // ---- F: angle derivatives and the Adam step
        const double bc1 = p.bias1[it], bc2s = p.bias2_sqrt[it];
        for (int j = tid; j <= J; j += NT) {
            float g3[3];
            if (j < J) {
                const int pa = sParent[j];
                double gl[9], gr[9];
                if (pa < 0) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) gl[i] = gacc[j * 12 + i];
                } else {
                    mul33_at(sG + pa * 9, gacc + j * 12, gl);                     // G_parent^T gG
                }
                mul33_bt(gl, sL0 + j * 9, gr);                                    // gR = gL locals_in^T
                const double sx = sSC[j * 6], sy = sSC[j * 6 + 1], sz = sSC[j * 6 + 2], cx = sSC[j * 6 + 3], cy = sSC[j * 6 + 4], cz = sSC[j * 6 + 5];
                double rx[9], ry[9], rz[9], dx[9], dy[9], dz[9], t1[9], t2[9];
                axis_x(cx, sx, false, rx); axis_y(cy, sy, false, ry); axis_z(cz, sz, false, rz);
                axis_x(cx, sx, true, dx); axis_y(cy, sy, true, dy); axis_z(cz, sz, true, dz);
                mul33(ry, rz, t1); mul33(dx, t1, t2); g3[0] = (float)dot9(gr, t2);
                mul33(dy, rz, t1); mul33(rx, t1, t2); g3[1] = (float)dot9(gr, t2);
                mul33(ry, dz, t1); mul33(rx, t1, t2); g3[2] = (float)dot9(gr, t2);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) g3[k] = (float)gacc[root * 12 + 9 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int s = j * 3 + k;
                float pv = sPar[s], m = sM[s], v = sV[s];
                adam_step(g3[k], pv, m, v, j < J ? lr_angle : lr, bc1, bc2s);
                sPar[s] = pv; sM[s] = m; sV[s] = v; sGrad[s] = g3[k];
            }
        }
        // no barrier here: A of the next iteration touches only this thread's own joints; the translation is read after A's barrier
    }
    __syncthreads();
    // quirk (i): locals, globals and jpos of the LAST forward (the parameters before the last step); angles and translation after it
    for (int i = tid; i < J * 9; i += NT) { p.locals[(size_t)j0 * 9 + i] = sL[i]; p.globals[(size_t)j0 * 9 + i] = sG[i]; }
    for (int i = tid; i < J * 3; i += NT) {
        p.jpos[(size_t)j0 * 3 + i] = sP[i];
        p.angles[(size_t)j0 * 3 + i] = sPar[i];
        if (p.grad_angles) p.grad_angles[(size_t)j0 * 3 + i] = sGrad[i];
    }
    if (tid < 3) {
        p.trans[(size_t)b * 3 + tid] = sPar[J * 3 + tid];
        if (p.grad_trans) p.grad_trans[(size_t)b * 3 + tid] = sGrad[J * 3 + tid];
    }
    if (tid == 0 && p.loss) {
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += red[w];
        p.loss[b] = (float)(s / (3.0 * (double)V));
    }
}

// ---- correspondence selection (eval_tracking.py:84-91): per point the vertex with the largest similarity among those whose nearest point
// it is; the first vertex on ties; similarity > 0. key = (similarity bits << 32) | (0xffffffff - vertex): positive floats order as their
// bit patterns, so ONE 64-bit integer max decides both, in any arrival order.
__global__ __launch_bounds__(256) void corr_winner_kernel(const int* __restrict__ nn, const float* __restrict__ sim, int n_vtx, int n_pts,
                                                          unsigned long long* __restrict__ keys) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vtx) return;
    const int q = nn[v];
    const float s = sim[v];
    if (q < 0 || q >= n_pts || !(s > 0.f)) return;
    atomicMax(keys + q, ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)v));
}
__global__ __launch_bounds__(256) void corr_decode_kernel(const unsigned long long* __restrict__ keys, int n_pts, int* __restrict__ winner,
                                                          float* __restrict__ winner_sim) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_pts) return;
    const unsigned long long k = keys[q];
    winner[q] = k ? (int)(0xffffffffu - (unsigned)(k & 0xffffffffull)) : -1;
    winner_sim[q] = k ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
}

}  // namespace morig

using namespace morig;

static_assert(sizeof(morig_ik_args) == MORIG_IK_SOLVE_STRUCT_BYTES, "include/morig_hip.h states the size");
static int ik_threads(int max_vertices) { return max_vertices > 512 ? 1024 : 256; }

extern "C" int64_t morig_ik_solve_lds_bytes(int32_t max_joints, int32_t max_vertices) {
    if (max_joints < 1 || max_vertices < 1) return MORIG_E_INVALID;
    return (int64_t)ik_lds_bytes(max_joints, max_vertices, ik_threads(max_vertices));
}

extern "C" int morig_ik_solve(const morig_ik_args* args, void* stream) {
    morig_ik_args a;
    if (!take_args(args, a, MORIG_IK_SOLVE_STRUCT_BYTES)) return MORIG_E_INVALID;
    if (a.n_problems <= 0 || a.max_joints < 1 || a.max_vertices < 1 || a.max_iter < 1 || a.n_entries < 0) return MORIG_E_INVALID;
    if (!a.joint_ptr || !a.vert_ptr || !a.level_off || !a.locals_in || !a.offsets || !a.parent || !a.order || !a.level_ptr || !a.child_lo ||
        !a.child_hi || !a.vptr || !a.jptr || !a.constraints || !a.vismask || !a.root || !a.iter_time || !a.lr || !a.w_invis || !a.thrd ||
        !a.bias1 || !a.bias2_sqrt || !a.angles || !a.trans || !a.locals || !a.globals || !a.jpos || !a.status) return MORIG_E_INVALID;
    if (a.n_entries > 0 && (!a.vent_j || !a.vent_xw || !a.jent_v || !a.jent_xw)) return MORIG_E_INVALID;
    if (a.n_entries > 0x7fffffffL) return MORIG_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(a.vent_xw) | reinterpret_cast<uintptr_t>(a.jent_xw)) & 15) return MORIG_E_INVALID;
    const int nt = ik_threads(a.max_vertices);
    const size_t lds = ik_lds_bytes(a.max_joints, a.max_vertices, nt);
    int dev = 0, lds_max = 0;
    MORIG_HIP_TRY(hipGetDevice(&dev));
    MORIG_HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (lds + IK_STATIC_LDS > (size_t)lds_max) return MORIG_E_UNSUPPORTED;                       // the problem does not fit in LDS: refused, never spilled
    IkParams p;
    p.joint_ptr = a.joint_ptr; p.vert_ptr = a.vert_ptr; p.level_off = a.level_off; p.locals_in = a.locals_in; p.offsets = a.offsets;
    p.parent = a.parent; p.order = a.order; p.level_ptr = a.level_ptr; p.child_lo = a.child_lo; p.child_hi = a.child_hi;
    p.vptr = a.vptr; p.vent_j = a.vent_j; p.vent_xw = reinterpret_cast<const float4*>(a.vent_xw);
    p.jptr = a.jptr; p.jent_v = a.jent_v; p.jent_xw = reinterpret_cast<const float4*>(a.jent_xw); p.n_entries = a.n_entries;
    p.constraints = a.constraints; p.vismask = a.vismask; p.root = a.root; p.iter_time = a.iter_time; p.lr = a.lr; p.w_invis = a.w_invis;
    p.thrd = a.thrd; p.bias1 = a.bias1; p.bias2_sqrt = a.bias2_sqrt; p.max_joints = a.max_joints; p.max_vertices = a.max_vertices;
    p.max_iter = a.max_iter; p.angles = a.angles; p.trans = a.trans; p.locals = a.locals; p.globals = a.globals; p.jpos = a.jpos;
    p.loss = a.loss; p.grad_angles = a.grad_angles; p.grad_trans = a.grad_trans; p.status = a.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_JOINTS, s, 0.0, 0.0);
    if (nt == 1024) {
        if (lds > 64 * 1024) MORIG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ik_solve_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(ik_solve_kernel<1024>, dim3(a.n_problems), dim3(1024), lds, s, p);
    } else {
        if (lds > 64 * 1024) MORIG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ik_solve_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(ik_solve_kernel<256>, dim3(a.n_problems), dim3(256), lds, s, p);
    }
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

extern "C" int morig_corr_select(const int32_t* nn, const float* sim, int32_t n_vtx, int32_t n_pts, uint64_t* keys, int32_t* winner,
                                 float* winner_sim, void* stream) {
    if (!nn || !sim || !keys || !winner || !winner_sim || n_vtx <= 0 || n_pts <= 0) return MORIG_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ProfScope ps(K_COSINE_NN, s, 0.0, 0.0);
    MORIG_HIP_TRY(hipMemsetAsync(keys, 0, sizeof(uint64_t) * (size_t)n_pts, s));
    hipLaunchKernelGGL(corr_winner_kernel, dim3(cdiv(n_vtx, 256)), dim3(256), 0, s, nn, sim, n_vtx, n_pts,
                       reinterpret_cast<unsigned long long*>(keys));
    MORIG_LAUNCH_CHECK();
    hipLaunchKernelGGL(corr_decode_kernel, dim3(cdiv(n_pts, 256)), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(keys), n_pts,
                       winner, winner_sim);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}
