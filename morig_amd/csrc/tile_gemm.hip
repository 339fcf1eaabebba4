// The one MFMA tile engine behind both hot operators of the MoRig forward path:
//
//   morig_gemm      dense vertex layer   Y = s*act(X W^T + b + rowbias[seg]) + t   [+ per-mesh column max]
//   morig_edgeconv  fused EdgeConv       out[i] = max_{j->i} s2*relu(W2 (s1*relu(A_i + B_j) + t1) + b2) + t2
//
// Both are a [rows x K] x [K x N] contraction on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma
// chain) with a 128-row workgroup tile; they differ only in how the A operand tile is PRODUCED
// (dense rows vs gather-add-ReLU-affine of two per-vertex rows named by the CSR) and how the
// accumulator tile is CONSUMED (store vs segmented max over rows).
//
// Layout facts used below (cdna_hip_programming.md section 3, MI355X_MICROARCH.md LDS table):
//   * 32x32x2 f32 MFMA: A operand lane l -> A[i = l&31][k = l>>5]; B operand lane l -> B[k = l>>5][j = l&31];
//     D register r of lane l -> D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31].
//   * K order inside a group of 8 is permuted so that ONE ds_read_b128 feeds 4 consecutive MFMAs:
//     MFMA m of group q multiplies k = 8q+m (lanes 0-31) and k = 8q+4+m (lanes 32-63). Both operands
//     use the same permutation, so the sum is the same set of products.
//   * LDS rows are padded to KC+4 floats: for ds_read_b128 the 16-lane service groups then touch
//     16 distinct 16-byte slots (36*r mod 64 and 20*r mod 64 are 4*(odd*r mod 16)) -> conflict-free.
#include "common.h"
#include "epilogue_store.h"
#include <stdint.h>
#include <type_traits>

namespace morig {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 f16x2 __attribute__((ext_vector_type(2)));        // what __builtin_amdgcn_cvt_pkrtz returns

// Arithmetic modes of the contraction:
//   PREC_F32   : v_mfma_f32_32x32x2_f32, exact fp32 products (157 TFLOP/s peak).
//   PREC_F16X3 : every fp32 operand is split x = hi + lo with hi = fp16(x), lo = fp16(x - hi); the product
//                is  hi*hi + hi*lo + lo*hi  on v_mfma_f32_32x32x16_f16 with fp32 accumulation (3 MFMAs per
//                16 k = 5.3x the fp32-MFMA rate). fp16 products are exact in fp32, the dropped lo*lo term
//                and the rounding of lo are both ~2^-22 relative: fp32-class accuracy. |x| must stay below
//                the fp16 range; the loader raises `ovf` otherwise and the host re-runs in PREC_F32.
//   PREC_BF16X6 [r06]: both fp32 operands are split IN THE KERNEL into three bf16 limbs x = b1 + b2 + b3 (8 + 8 + 8 mantissa bits, float32's
//                exponent range: no range condition) and the product is the six terms down to 2^-16 of the leading one --
//                b1 b1 + b1 b2 + b2 b1 + b2 b2 + b1 b3 + b3 b1 -- on v_mfma_f32_32x32x16_bf16: float32-class products (the dropped terms are
//                <= 2^-24 relative) at 16/6 = 2.7x the fp32-MFMA rate. Takes plain fp32 X and W (weights that change every step need no
//                host-side image): the train-mode forward contractions and the exact path behind the range guard.
//   PREC_BF16X3 [r04]: the same 3-MFMA split as PREC_F16X3 on bf16 halves (float32 exponent range: the backward contractions, whose
//                operands are gradients); dense fp32-X stores only.
// (the PREC_* / LOAD_* / MODE_* constants and the list of instantiations that exist: dispatch_core.h)

// LOAD_EDGE3: an EdgeConv whose vertex input has 3 channels (positions; the keyframe flow of motionNet's first unit): instead of
//             gathering the per-vertex first-layer terms A[dst], B[src] (2 x 4 H bytes per edge row) the loader gathers the two
//             endpoints' 3 inputs (2 x 16 bytes) and evaluates the first Linear for its 4 hidden channels in registers
//             (relu((Wa - Wb) x_i + Wb x_j + b): 28 fused multiply-adds per thread and row).

struct TileParams {
    int M, N, K;                 // rows (edge: capacity), logical out width, contraction length
    const float* W; int ldw;
    const float* bias; const float* scale; const float* shift; int relu;
    // dense loader
    const float* X; int ldx;
    // edge loader
    const float* A; int lda; const float* B; int ldb;
    const float* X3; int ldx3; const float* W1a; const float* W1b; const float* b1;     // LOAD_EDGE3: inputs [rows][ldx3 >= 4], [Hpad][4] weights
    const int* rowptr; const int* srcS; const int* dstS; int n_nodes; int rep_in; int rep_out; int tiles_per_rep;
    const float* s1; const float* t1;
    // epilogue
    const float* rowbias; int ld_rowbias; const int* seg;
    float* Y; int ldy;           // store target / edge-max target / pool target
    int tiles_n;
    int* ovf;                    // PREC_F16X3: set to 1 when an operand leaves the fp16 range
    int x16, y16;                // PREC_F16X3 dense: X already in split-fp16 layout / store Y in split-fp16 layout
    int dbg;                     // ablation switches for tools/microbench.py (MORIG_DEBUG_FLAGS; 0 in production)
};
enum { DBG_NO_EPILOGUE = 1, DBG_NO_MFMA = 2, DBG_NO_GATHER = 4, DBG_NO_WLOAD = 8, DBG_NO_STAGE = 16 };

// The narrow EdgeConv tiles are latency chains (ids -> gathers -> one or two K-chunks -> scan): occupancy is what hides
// them, so their register budget is capped for 4 (fp32, KC = 16: 6) waves per SIMD (measured -17..21 % at H = 32).
// The dense fp32-X GEMM tile (BN = 128, KC = 32) likewise runs better at 3 waves per SIMD than at 2.
// FAST [r04]: every row of every tile exists (M a multiple of 128), K is a multiple of KC and no debug switch is set -- decided by the
// launcher; the row / column tests, zero fills and switch tests compile out (dense store GEMMs with fp32 X: the GCU units' MLPs of the
// forward, dX of the training step; the counters of the general form: 7.0 VALU + 3.6 SALU instructions per MFMA, matrix pipe 39 % busy).
template <int BN, int KC, int LOAD, int MODE, int PREC, bool FAST = false>
__global__ __launch_bounds__(256, ((BN == 256 && PREC == PREC_F32) ? 2 : (BN == 32 && LOAD != LOAD_DENSE) ? ((PREC == PREC_F32 && KC == 16) ? 6 : 4) : (BN == 64 && LOAD == LOAD_EDGE && PREC == PREC_F16X3) ? 4 : (PREC == PREC_BF16X6) ? (BN >= 256 ? 1 : 2) : (BN == 128 && KC == 32 && LOAD == LOAD_DENSE && MODE != MODE_EDGEMAX && PREC != PREC_F32) ? 3 :
                               (BN == 64 && LOAD == LOAD_DENSE && MODE == MODE_STORE && PREC != PREC_F32) ? 4 : 1)) void tile_kernel(const TileParams p) {
    constexpr int BM = 128;
    constexpr int WN = (BN >= 128) ? 2 : 1;
    constexpr int WM = 4 / WN;
    constexpr int MT = BM / WM / 32;
    constexpr int NT = BN / WN / 32;
    constexpr int LDK = (PREC == PREC_BF16X6 ? (KC / 32) * 48 : KC) + 4;      // floats per LDS row (BF16X6: three limbs = 192 B per 32-column chunk)
    constexpr int TPR = KC / 4;                 // loader threads per tile row
    constexpr int RPP = 256 / TPR;              // tile rows per loader pass
    constexpr int PA = BM / RPP;
    constexpr int PB = (BN + RPP - 1) / RPP;
    constexpr int ZC = BN < 64 ? BN : 64;       // epilogue column block
    constexpr int ZLD = ZC + 1;
    constexpr int SM_MAIN = (BM + BN) * LDK;
    constexpr int SM_Z = (MODE == MODE_STORE) ? 4 * EpilogueTile<NT>::FLOATS      // store: per-wave transposition tiles
                       : (MODE == MODE_EDGEMAX && BN == 32) ? BM * 36 : BM * ZLD;      // narrow EdgeConv: 16-byte Z rows
    constexpr int SM = SM_MAIN > SM_Z ? SM_MAIN : SM_Z;
    static_assert(BN % 32 == 0 && KC % 8 == 0, "tile shape");
    static_assert(PREC == PREC_F32 || KC % 32 == 0, "the split-fp16 LDS image is [hi 32 halves | lo 32 halves] per 32-column chunk");

    __shared__ __attribute__((aligned(16))) float smem[SM + BM];
    float* sA = smem;
    float* sB = smem + BM * LDK;
    int* sseg = reinterpret_cast<int*>(smem + SM);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;

    const int lin = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn, rep;
    if (LOAD == LOAD_DENSE) { tn = lin % p.tiles_n; tm = lin / p.tiles_n; rep = 0; }
    else { rep = lin / p.tiles_per_rep; tm = lin - rep * p.tiles_per_rep; tn = 0; }
    const int row0 = tm * BM;

    constexpr bool IS_EDGE = LOAD != LOAD_DENSE;                               // gathered edge rows (LOAD_EDGE, LOAD_EDGE3)
    constexpr bool EDGE_ROWS = IS_EDGE || (MODE == MODE_EDGEMAX);               // tile rows = sorted edges
    // Edge tiles: the edge count, this thread's edge ids and the ids just outside the tile are all fetched before anything
    // waits (rows are clamped to the arrays' capacity p.M, validity is applied afterwards): ONE memory latency at tile
    // start instead of a chain of two or three. The neighbour ids decide in the epilogue whether the first / last
    // segment is shared with another tile (rowptr look-ups there were two dependent global loads on its critical path).
    int Etot = 0;
    int dprev = -2, dafter = -3;
    int ld_d[BM / (256 / (KC / 4))], ld_s[BM / (256 / (KC / 4))];
    if (EDGE_ROWS) {
        Etot = p.rowptr[p.n_nodes];
        const int lr = tid / (KC / 4);
#pragma unroll
        for (int i = 0; i < BM / (256 / (KC / 4)); ++i) {
            const int rc = min(row0 + lr + i * (256 / (KC / 4)), p.M - 1);
            ld_d[i] = p.dstS[rc];
            ld_s[i] = IS_EDGE ? p.srcS[rc] : 0;
        }
        if (MODE == MODE_EDGEMAX) {
            const int dp = p.dstS[max(row0 - 1, 0)], da = p.dstS[min(row0 + BM, p.M - 1)];
            if (row0 > 0) dprev = dp;
            if (row0 + BM < Etot) dafter = da;
        }
        if (row0 >= Etot) return;               // block-uniform
    }
    const int Mlim = EDGE_ROWS ? Etot : p.M;

    // ---- loader set-up -------------------------------------------------------------------
    const int lrow = tid / TPR, lkq = tid % TPR;
    const float* pa[PA];
    const float* pb[PA];                        // edge only
    bool va[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int r = lrow + i * RPP;
        const int row = row0 + r;
        if (LOAD == LOAD_DENSE) {
            va[i] = FAST || row < Mlim;
            pa[i] = p.X + (size_t)(va[i] ? row : 0) * p.ldx + 4 * lkq;
            pb[i] = nullptr;
            if (MODE == MODE_EDGEMAX) {
                if (lkq == 0) sseg[r] = va[i] ? ld_d[i] : -1;
            } else if (MODE != MODE_STORE || p.seg != nullptr) {
                if (lkq == 0) sseg[r] = (va[i] && p.seg) ? p.seg[row] : -1;
            }
        } else {
            va[i] = row < Etot;
            const int d = va[i] ? ld_d[i] : -1;
            const int s = va[i] ? ld_s[i] : 0;
            const size_t base = (size_t)rep * p.rep_in;
            if (LOAD == LOAD_EDGE3) {
                pa[i] = p.X3 + (base + (va[i] ? d : 0)) * p.ldx3;
                pb[i] = p.X3 + (base + s) * p.ldx3;
            } else {
                pa[i] = p.A + (base + (va[i] ? d : 0)) * p.lda + 4 * lkq;
                pb[i] = p.B + (base + s) * p.ldb + 4 * lkq;
            }
            if (lkq == 0) sseg[r] = d;
        }
    }
    const float* pw = p.W + (size_t)(tn * BN + lrow) * p.ldw + 4 * lkq;

    // LOAD_EDGE3: first-layer rows [channel][8] = {W1a row (3), b1, W1b row (3), 0} in LDS (28 per-thread registers would spill the
    // 128-VGPR budget that keeps 4 waves per SIMD); read channel by channel while staging, reused over the thread's PA rows
    __shared__ __attribute__((aligned(16))) float w3[LOAD == LOAD_EDGE3 ? 32 * 8 : 4];
    if (LOAD == LOAD_EDGE3) {
        if (tid < 32) {
            w3[tid * 8 + 0] = p.W1a[tid * 4 + 0]; w3[tid * 8 + 1] = p.W1a[tid * 4 + 1]; w3[tid * 8 + 2] = p.W1a[tid * 4 + 2]; w3[tid * 8 + 3] = p.b1[tid];
            w3[tid * 8 + 4] = p.W1b[tid * 4 + 0]; w3[tid * 8 + 5] = p.W1b[tid * 4 + 1]; w3[tid * 8 + 6] = p.W1b[tid * 4 + 2]; w3[tid * 8 + 7] = 0.f;
        }
    }
    f32x4 ra[PA], rb[PA], rw[PB];
    f32x4 rs1 = {1.f, 1.f, 1.f, 1.f}, rt1 = {0.f, 0.f, 0.f, 0.f};      // hidden-layer affine of this thread's 4 k's
    auto fetch = [&](int k0) {
        if (LOAD == LOAD_EDGE3) {                           // one chunk (K = H = 32): both endpoints' inputs, 16 bytes each
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
                ra[i] = z; rb[i] = z;
                if (va[i] && !(p.dbg & DBG_NO_GATHER)) {
                    ra[i] = *reinterpret_cast<const f32x4*>(pa[i]);
                    rb[i] = *reinterpret_cast<const f32x4*>(pb[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                if ((BN % RPP == 0 || lrow + i * RPP < BN) && !(p.dbg & DBG_NO_WLOAD))
                    rw[i] = *reinterpret_cast<const f32x4*>(pw + (size_t)i * RPP * p.ldw + k0);
            }
            return;
        }
        if (LOAD == LOAD_EDGE && p.s1 != nullptr && k0 + 4 * lkq < p.K) {   // NULL: affine already folded into W2/b2
            rs1 = *reinterpret_cast<const f32x4*>(p.s1 + k0 + 4 * lkq);
            rt1 = *reinterpret_cast<const f32x4*>(p.t1 + k0 + 4 * lkq);
        }
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if (!FAST) { ra[i] = z; rb[i] = z; }
            // split-fp16 X: a 16-byte piece holds halves of its whole 32-column chunk -> guard per chunk
            const int k = (PREC == PREC_F16X3 && LOAD == LOAD_DENSE && p.x16) ? ((k0 + 4 * lkq) & ~31) : (k0 + 4 * lkq);
            if (FAST || (va[i] && k < p.K && !(p.dbg & DBG_NO_GATHER))) {
                ra[i] = *reinterpret_cast<const f32x4*>(pa[i] + k0);
                if (IS_EDGE) rb[i] = *reinterpret_cast<const f32x4*>(pb[i] + k0);
            }
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if ((BN % RPP == 0 || lrow + i * RPP < BN) && (FAST || !(p.dbg & DBG_NO_WLOAD)))
                rw[i] = *reinterpret_cast<const f32x4*>(pw + (size_t)i * RPP * p.ldw + k0);
        }
    };
    // BF16X6: four fp32 values -> their three bf16 limbs, 4 halves (8 bytes) each into the [b1 | b2 | b3] thirds of the row's 192-byte chunk
    auto split3_store = [&](char* rowp, const f32x4& v) __attribute__((always_inline)) {
        typedef float b32x2 __attribute__((ext_vector_type(2)));
        b32x2 l1, l2, l3;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float h, r0, r1, m, t;
            split_pair_bf16_rem(v[2 * q], v[2 * q + 1], h, r0, r1);       // h = bf16 pair, r = the exact remainders
            l1[q] = h;
            float s0, s1;
            split_pair_bf16_rem(r0, r1, m, s0, s1);
            l2[q] = m;
            split_pair_bf16(s0, s1, t, h);                                // third limb (h: the fourth, dropped)
            l3[q] = t;
        }
        *reinterpret_cast<b32x2*>(rowp) = l1;
        *reinterpret_cast<b32x2*>(rowp + 64) = l2;
        *reinterpret_cast<b32x2*>(rowp + 128) = l3;
    };
    auto stage = [&](int k0) {
        const int k = k0 + 4 * lkq;
        f32x4 v3[PA];
        if (LOAD == LOAD_EDGE3) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 wa = *reinterpret_cast<const f32x4*>(&w3[(4 * lkq + c) * 8]);        // W1a row, b1
                const f32x4 ws = *reinterpret_cast<const f32x4*>(&w3[(4 * lkq + c) * 8 + 4]);    // W1b row
#pragma unroll
                for (int i = 0; i < PA; ++i) {
                    float h = wa[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) h = fmaf(wa[j], ra[i][j], fmaf(ws[j], rb[i][j], h));
                    v3[i][c] = va[i] ? fmaxf(h, 0.f) : 0.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            f32x4 v = ra[i];
            if (LOAD == LOAD_EDGE3) {
                v = v3[i];
            } else if (LOAD == LOAD_EDGE) {
                if (p.s1 != nullptr) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float h = v[c] + rb[i][c];
                        h = h > 0.f ? h : 0.f;
                        v[c] = va[i] ? (h * rs1[c] + rt1[c]) : 0.f;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c] + rb[i][c], 0.f);      // invalid rows were fetched as 0
                }
            } else if (!FAST && k0 + KC > p.K && !(PREC == PREC_F16X3 && p.x16)) {   // only the last chunk can cross K
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = (k + c < p.K) ? v[c] : 0.f;
            }
            if (PREC == PREC_F32) {
                *reinterpret_cast<f32x4*>(&sA[(lrow + i * RPP) * LDK + 4 * lkq]) = v;
            } else if (PREC == PREC_BF16X6) {
                split3_store(reinterpret_cast<char*>(sA) + (lrow + i * RPP) * (LDK * 4) + 192 * (lkq >> 3) + 8 * (lkq & 7), v);
            } else if (PREC == PREC_F16X3 && LOAD == LOAD_DENSE && p.x16) {
                // the producer already wrote [32 halves hi | 32 halves lo] per 32-column chunk: plain copy
                *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(sA) + (lrow + i * RPP) * (LDK * 4) + 16 * lkq) = ra[i];
            } else {
                // hi = fp16(x) (round-toward-zero, 2 per instruction), lo = fp16(x - hi): x - hi is exact in fp32
                // (hi may truncate: lo absorbs it exactly; lo itself is rounded to nearest-even so the split is unbiased; common.h)
                typedef float b32x2 __attribute__((ext_vector_type(2)));
                b32x2 h, l;
                float h0, h1, l0, l1;
                if (PREC == PREC_BF16X3) {
                    split_pair_bf16(v[0], v[1], h0, l0);
                    split_pair_bf16(v[2], v[3], h1, l1);
                } else {
                    split_pair_f16(v[0], v[1], h0, l0);
                    split_pair_f16(v[2], v[3], h1, l1);
                    const float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
                    if (!(amax < FP16_RANGE_GUARD)) *p.ovf = 1;                 // also catches NaN
                }
                h[0] = h0; h[1] = h1; l[0] = l0; l[1] = l1;
                char* rowp = reinterpret_cast<char*>(sA) + (lrow + i * RPP) * (LDK * 4) + 128 * (lkq >> 3) + 8 * (lkq & 7);
                *reinterpret_cast<b32x2*>(rowp) = h;
                *reinterpret_cast<b32x2*>(rowp + 64) = l;
            }
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            if (BN % RPP == 0 || lrow + i * RPP < BN) {
                if (PREC == PREC_BF16X6) {                  // plain fp32 weights in, three limbs out (columns past K are zero in the packed rows)
                    f32x4 w = rw[i];
                    if (!FAST && (p.dbg & DBG_NO_WLOAD)) w = f32x4{0.f, 0.f, 0.f, 0.f};
                    split3_store(reinterpret_cast<char*>(sB) + (lrow + i * RPP) * (LDK * 4) + 192 * (lkq >> 3) + 8 * (lkq & 7), w);
                } else {
                    *reinterpret_cast<f32x4*>(&sB[(lrow + i * RPP) * LDK + 4 * lkq]) = rw[i];
                }
            }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // ---- main loop: register prefetch of chunk c+1 under the MFMAs of chunk c ---------------
    const int nchunk = (p.K + KC - 1) / KC;
    fetch(0);
    for (int c = 0; c < nchunk; ++c) {
        __syncthreads();                        // previous chunk's fragment reads are done
        if (FAST || !(p.dbg & DBG_NO_STAGE) || c == 0) stage(c * KC);
        __syncthreads();
        if (c + 1 < nchunk) fetch((c + 1) * KC);
        if (!FAST && (p.dbg & DBG_NO_MFMA)) continue;
        if (PREC == PREC_BF16X6) {
            const char* a0 = reinterpret_cast<const char*>(sA) + (wm * MT * 32 + l31) * (LDK * 4) + 16 * hi;
            const char* b0 = reinterpret_cast<const char*>(sB) + (wn * NT * 32 + l31) * (LDK * 4) + 16 * hi;
#pragma unroll
            for (int st2 = 0; st2 < KC / 16; ++st2) {
                const int off = 192 * (st2 >> 1) + 32 * (st2 & 1);     // 32-column chunk, 16-k step inside each 64-byte limb block
                bf16x8 x1[MT], x2[MT], x3[MT], w1[NT], w2[NT], w3[NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    x1[mt] = *reinterpret_cast<const bf16x8*>(a0 + mt * 32 * LDK * 4 + off);
                    x2[mt] = *reinterpret_cast<const bf16x8*>(a0 + mt * 32 * LDK * 4 + off + 64);
                    x3[mt] = *reinterpret_cast<const bf16x8*>(a0 + mt * 32 * LDK * 4 + off + 128);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    w1[nt] = *reinterpret_cast<const bf16x8*>(b0 + nt * 32 * LDK * 4 + off);
                    w2[nt] = *reinterpret_cast<const bf16x8*>(b0 + nt * 32 * LDK * 4 + off + 64);
                    w3[nt] = *reinterpret_cast<const bf16x8*>(b0 + nt * 32 * LDK * 4 + off + 128);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {           // smallest terms first
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3[mt], w1[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1[mt], w3[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2[mt], w2[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x2[mt], w1[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1[mt], w2[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x1[mt], w1[nt], acc[mt][nt], 0, 0, 0);
                    }
            }
            continue;
        }
        if (PREC != PREC_F32) {
            const char* a0 = reinterpret_cast<const char*>(sA) + (wm * MT * 32 + l31) * (LDK * 4) + 16 * hi;
            const char* b0 = reinterpret_cast<const char*>(sB) + (wn * NT * 32 + l31) * (LDK * 4) + 16 * hi;
#pragma unroll
            for (int st2 = 0; st2 < KC / 16; ++st2) {
                const int off = 128 * (st2 >> 1) + 32 * (st2 & 1);     // 32-column chunk, 16-k step inside it
                f16x8 ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    ah[mt] = *reinterpret_cast<const f16x8*>(a0 + mt * 32 * LDK * 4 + off);
                    al[mt] = *reinterpret_cast<const f16x8*>(a0 + mt * 32 * LDK * 4 + off + 64);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    bh[nt] = *reinterpret_cast<const f16x8*>(b0 + nt * 32 * LDK * 4 + off);
                    bl[nt] = *reinterpret_cast<const f16x8*>(b0 + nt * 32 * LDK * 4 + off + 64);
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if (PREC == PREC_BF16X3) {
                            const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[mt]), xl = __builtin_bit_cast(bf16x8, al[mt]);
                            const bf16x8 wh = __builtin_bit_cast(bf16x8, bh[nt]), wl = __builtin_bit_cast(bf16x8, bl[nt]);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, wh, acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, wl, acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, wh, acc[mt][nt], 0, 0, 0);
                        } else {
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                        }
                    }
            }
            continue;
        }
        const float* a0 = sA + (wm * MT * 32 + l31) * LDK + 4 * hi;
        const float* b0 = sB + (wn * NT * 32 + l31) * LDK + 4 * hi;
#pragma unroll
        for (int kk = 0; kk < KC / 8; ++kk) {
            f32x4 af[MT], bf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const f32x4*>(a0 + mt * 32 * LDK + kk * 8);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bf[nt] = *reinterpret_cast<const f32x4*>(b0 + nt * 32 * LDK + kk * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][j], bf[nt][j], acc[mt][nt], 0, 0, 0);
        }
    }

    // ---- epilogue ----------------------------------------------------------------------------
    if (!FAST && (p.dbg & DBG_NO_EPILOGUE)) { if (acc[0][0][0] == 12345.678f) p.Y[0] = 1.f; return; }
    const int colw0 = tn * BN + wn * NT * 32;   // first global column of this wave
    if (MODE == MODE_STORE) {
        __syncthreads();                        // all waves are done with the operand tiles; sseg visible
        store_tile_transposed<MT, NT, PREC == PREC_F16X3>(p, acc, smem + wave * EpilogueTile<NT>::FLOATS, sseg,
                                                          wm * MT * 32, row0, Mlim, colw0, lane);
        return;
    }

    // Segmented max over tile rows. The accumulator tile goes through LDS in column blocks of ZC (all four
    // waves write one or two fragments per pass); thread (column, row group) then preloads 16 rows at a time
    // (independent LDS reads, no dependent chain) and runs the segmented scan in registers.
    float* Z = smem;
    bool first_cont = false, last_cont = false;
    if (MODE == MODE_EDGEMAX) {
        // sseg was written before the main loop; every thread passed >= 1 barrier since
        first_cont = sseg[0] == dprev;
        last_cont = sseg[BM - 1] == dafter;
    }
    if constexpr (MODE == MODE_EDGEMAX && BN == 32) {
        // ---- narrow layers (H = 16, 32): the scan is half of the kernel if every thread walks a row group plus the tail
        // of its last segment (17-row segments over 16-row groups: ~3x redundant reads). Here wave 0 lists the segment
        // starts of the tile (two ballots over the 128 destination ids), and a slot of 8 threads -- 4 adjacent columns
        // each, 16-byte LDS reads -- reduces exactly the rows of one segment, slots taking segments round-robin.
        constexpr int ZL = 36;                      // floats per Z row (16-byte rows)
        __shared__ int sstart[BM + 2];              // start row of segment k; [nseg] = BM
        __shared__ int snseg;
        __syncthreads();                            // main-loop reads done
        {
            const int col = tn * BN + l31;
            const float b = (p.bias && col < p.N) ? p.bias[col] : 0.f;
            const float sc = (p.scale && col < p.N) ? p.scale[col] : 1.f;
            const float sh = (p.shift && col < p.N) ? p.shift[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;     // MT = NT = 1 for BN = 32
                float v = acc[0][0][r] + b;
                if (p.relu) v = v > 0.f ? v : 0.f;
                Z[rl * ZL + l31] = v * sc + sh;
            }
        }
        if (wave == 0) {
            const int r0 = lane, r1 = lane + 64;
            const bool f0 = r0 == 0 || sseg[r0] != sseg[r0 - 1];
            const bool f1 = sseg[r1] != sseg[r1 - 1];
            const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (f0) sstart[__popcll(m0 & below)] = r0;
            if (f1) sstart[__popcll(m0) + __popcll(m1 & below)] = r1;
            if (lane == 0) { const int ns = __popcll(m0) + __popcll(m1); snseg = ns; sstart[ns] = BM; }
        }
        __syncthreads();
        const int c4 = (tid & 7) * 4, slot = tid >> 3;                          // 8 threads x 4 columns per segment, 32 slots
        const int col0 = tn * BN + c4;
        if (col0 >= p.N) return;
        const int nseg = snseg;
        float* obase = p.Y + (size_t)rep * p.rep_out * p.ldy + col0;
        const bool vec_ok = (reinterpret_cast<uintptr_t>(p.Y) & 15) == 0 && (p.ldy & 3) == 0 && col0 + 4 <= p.N;
        for (int k = slot; k < nseg; k += 32) {
            const int rs = sstart[k], re = sstart[k + 1];
            const int sg = sseg[rs];
            if (sg < 0) continue;                                               // rows past the last edge
            f32x4 m = *reinterpret_cast<const f32x4*>(Z + rs * ZL + c4);
            for (int r = rs + 1; r < re; r += 4) {          // four independent reads in flight (rows past the end repeat the last)
                f32x4 z[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) z[u] = *reinterpret_cast<const f32x4*>(Z + min(r + u, re - 1) * ZL + c4);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) m[q] = fmaxf(m[q], z[u][q]);
            }
            float* o = obase + (size_t)sg * p.ldy;
            const bool partial = (rs == 0 && first_cont) || (re == BM && last_cont);
            if (partial) {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (col0 + q < p.N) atomic_max_f32(o + q, m[q]);
            } else if (vec_ok) {
                *reinterpret_cast<f32x4*>(o) = m;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (col0 + q < p.N) o[q] = m[q];
            }
        }
        return;
    }
    constexpr int NTP = ((ZC / 32) / WN) >= 1 ? ((ZC / 32) / WN) : 1;    // fragments per wave per pass
    constexpr int NPASS = NT / NTP;
    static_assert(NTP * WN * 32 == ZC && NPASS * NTP == NT, "epilogue column blocking");
    constexpr int G = 256 / ZC;                 // row groups in the reduce phase
    constexpr int RG = BM / G;                  // 32 (ZC = 64) or 16 (ZC = 32)
    const int zc = tid % ZC, zg = tid / ZC;
    const int r0 = (ZC == 64) ? __builtin_amdgcn_readfirstlane(zg * RG) : zg * RG;
    // MODE_EDGEMAX: segment starts of the tile's 128 rows as two ballots, once for all column passes
    unsigned long long seg_start_lo = 0, seg_start_hi = 0, seg_own = 0; int seg_id_own = 0;
    if constexpr (MODE == MODE_EDGEMAX && ZC == 64) {
        const int s_lo = sseg[lane], s_hi = sseg[lane + 64];
        const int p_lo = sseg[lane > 0 ? lane - 1 : 0], p_hi = sseg[lane + 63];
        seg_start_lo = __ballot(lane == 0 || s_lo != p_lo); seg_start_hi = __ballot(s_hi != p_hi);
        const bool up = r0 >= 64;
        const unsigned long long valid = up ? __ballot(s_hi >= 0) : __ballot(s_lo >= 0);
        seg_own = (up ? seg_start_hi : seg_start_lo) & valid & (((1ull << RG) - 1ull) << (r0 & 63));
        seg_id_own = up ? s_hi : s_lo;
    }
    // one instantiation per column pass: `cb` must be a compile-time constant so that acc[][] keeps
    // static register indices (a runtime-indexed accumulator array would live in scratch memory)
    auto run_pass = [&](auto cb_const) {
        constexpr int cb = decltype(cb_const)::value;
        __syncthreads();                        // main-loop reads / previous pass's scan done
#pragma unroll
        for (int j = 0; j < NTP; ++j) {
            constexpr int dummy = 0; (void)dummy;
            const int nt = cb * NTP + j;
            const int col = tn * BN + wn * NT * 32 + nt * 32 + l31;
            const float b = (p.bias && col < p.N) ? p.bias[col] : 0.f;
            const float sc = (p.scale && col < p.N) ? p.scale[col] : 1.f;
            const float sh = (p.shift && col < p.N) ? p.shift[col] : 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wm * MT * 32 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    float v = acc[mt][nt][r] + b;
                    if (p.relu) v = v > 0.f ? v : 0.f;
                    Z[rl * ZLD + (wn * NTP + j) * 32 + l31] = v * sc + sh;
                }
        }
        __syncthreads();
        const int wz = zc / (NTP * 32), jz = (zc >> 5) % NTP;
        const int col = tn * BN + wz * NT * 32 + (cb * NTP + jz) * 32 + (zc & 31);
        if (col >= p.N) return;
        const float* zcolp = Z + zc;
        if (MODE == MODE_POOL) {
            // every output is shared with other tiles -> all atomic; each group reduces its own rows
            int cur = -2; bool open = false; float m = 0.f;
#pragma unroll
            for (int bt = 0; bt < RG / 16; ++bt) {
                const int rb0 = r0 + bt * 16;
                float zv[16]; int sv[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sv[i] = (ZC == 64) ? __builtin_amdgcn_readfirstlane(sseg[rb0 + i]) : sseg[rb0 + i];
                    zv[i] = zcolp[(rb0 + i) * ZLD];
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (sv[i] != cur) {
                        if (open) atomic_max_f32(p.Y + (size_t)cur * p.ldy + col, m);
                        cur = sv[i]; open = cur >= 0; m = zv[i];
                    } else if (open) m = fmaxf(m, zv[i]);
                }
            }
            if (open) atomic_max_f32(p.Y + (size_t)cur * p.ldy + col, m);
        } else {
            // a wave (zg = wave id: ZC == 64 here) owns the segments that START in its row group and follows them to their
            // end. Segment bookkeeping by ballots (lane l looks at rows l and l + 64), then a walk over the set bits with four
            // LDS reads in flight per step -- not a per-row state machine (edge_pp.hip, same scheme).
            if constexpr (ZC == 64) {                          // (BN = 32 takes the narrow path above; its pooled variant the branch above)
            float* obase = p.Y + (size_t)rep * p.rep_out * p.ldy + col;
            const bool upper = r0 >= 64;
            unsigned long long mine = seg_own;
            while (mine) {                                                   // wave-uniform
                const int bl = __builtin_ctzll(mine);
                mine &= mine - 1ull;
                const unsigned long long above = bl < 63 ? ~((2ull << bl) - 1ull) : 0ull;
                int rs, re;
                if (upper) {
                    const unsigned long long later = seg_start_hi & above;
                    rs = 64 + bl; re = later ? 64 + __builtin_ctzll(later) : BM;
                } else {
                    const unsigned long long later = seg_start_lo & above;
                    rs = bl; re = later ? __builtin_ctzll(later) : (seg_start_hi ? 64 + __builtin_ctzll(seg_start_hi) : BM);
                }
                const int sg = __builtin_amdgcn_readlane(seg_id_own, bl);
                float m = zcolp[rs * ZLD];
                for (int r = rs + 1; r < re; r += 4) {
                    const int l = re - 1;
                    const float z0 = zcolp[r * ZLD], z1 = zcolp[min(r + 1, l) * ZLD], z2 = zcolp[min(r + 2, l) * ZLD], z3 = zcolp[min(r + 3, l) * ZLD];
                    m = fmaxf(fmaxf(m, z0), fmaxf(fmaxf(z1, z2), z3));
                }
                float* o = obase + (size_t)sg * p.ldy;
                if ((rs == 0 && first_cont) || (re == BM && last_cont)) atomic_max_f32(o, m); else *o = m;
            }
            }
        }
    };
    run_pass(std::integral_constant<int, 0>{});
    if constexpr (NPASS > 1) run_pass(std::integral_constant<int, 1>{});
    if constexpr (NPASS > 2) run_pass(std::integral_constant<int, 2>{});
    if constexpr (NPASS > 3) run_pass(std::integral_constant<int, 3>{});
    static_assert(NPASS <= 4, "column passes");
}

// Rows of `out` whose segment straddles a tile boundary are combined with integer-atomic float max
// by the two (or more) tiles involved: only THOSE rows need the identity pattern 0xFFFFFFFF beforehand.
// [r05] a LANE per boundary for the index chain (rowptr[n] -> dstS[e] -> rowptr[d]: three dependent loads, which one wave per
// boundary paid 330 k times per launch on the geo graph), then the wave walks the rows its lanes found and stores them 16 bytes per
// lane ([r04] had one wave per boundary: 17 us per launch on average, 0.3 ms per step).
// Tiles are numbered over the replicas, t = replica * tpr + tile (tpr = ceil(E' / tile_rows), E' read on the device); a persistent
// kernel that carries an open segment from tile to tile inside RUNS of `run` consecutive tiles (edge_rl.hip / edge_ws.hip) shares rows
// only where a run ends: candidate g = 1, 2, ... is the boundary in front of tile t = g * run (run = 1: every tile boundary).
// -> the output row (replica * rep_out + destination) whose segment straddles that boundary, or -1.
__device__ __forceinline__ int straddled_row(const int* __restrict__ rowptr, const int* __restrict__ dstS, int n_nodes, int tile_rows,
                                             int run, int replicas, int rep_out, int g, int n_cand, bool last_only) {
    if (g > n_cand) return -1;
    const int Etot = rowptr[n_nodes];
    const int tpr = (Etot + tile_rows - 1) / tile_rows;
    if (tpr <= 0) return -1;
    const long long t = (long long)g * run;
    const int rep = (int)(t / tpr), tile = (int)(t - (long long)rep * tpr);
    if (rep >= replicas || tile == 0) return -1;                      // a replica starts here: nothing above it
    const int e = tile * tile_rows;                                   // < Etot
    const int d = dstS[e];
    if (rowptr[d] >= e) return -1;                                    // a segment starts exactly on the boundary: no sharing
    // several shared boundaries inside one long segment: the LAST one stands for the row (the next one of this replica is run tiles on)
    if (last_only && (long long)e + (long long)run * tile_rows < rowptr[d + 1]) return -1;
    return rep * rep_out + d;
}

// One boundary pass may serve TWO launches [r06]: the template-graph and the geodesic-graph EdgeConv of a unit write disjoint column
// blocks of the same rows, their passes are independent of each other's kernels, and at one mesh per forward a pass is a launch plus one
// dependent index chain (7-9 us, 26 of them = 12 % of the forward): blockIdx.y selects the job.
struct BoundaryJob { const int* rowptr; const int* dstS; int n_nodes, H; float* out; int ldo, rep_out, tile_rows, run, replicas, n_cand; int* ovf; };
struct BoundaryJobs { BoundaryJob j[2]; };

__global__ __launch_bounds__(256) void init_boundary_rows_kernel(const BoundaryJobs js) {
    const BoundaryJob& b = js.j[blockIdx.y];
    if ((int)blockIdx.x * 256 >= b.n_cand) return;
    const int* __restrict__ rowptr = b.rowptr; const int* __restrict__ dstS = b.dstS;
    float* __restrict__ out = b.out;
    const int H = b.H, ldo = b.ldo;
    const int lane = threadIdx.x & 63;
    const int d = straddled_row(rowptr, dstS, b.n_nodes, b.tile_rows, b.run, b.replicas, b.rep_out, blockIdx.x * 256 + threadIdx.x + 1, b.n_cand, false);
    const bool vec = ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)(ldo * 4) | (uintptr_t)(H * 4)) & 15) == 0;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    unsigned long long todo = __ballot(d >= 0);
    while (todo) {                                                    // wave-uniform
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        float* orow = out + (size_t)__builtin_amdgcn_readlane(d, l) * ldo;
        if (vec) {
            u32x4* o4 = reinterpret_cast<u32x4*>(orow);
            for (int c = lane; c < H / 4; c += 64) o4[c] = u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        } else {
            unsigned* o = reinterpret_cast<unsigned*>(orow);
            for (int c = lane; c < H; c += 64) o[c] = 0xFFFFFFFFu;
        }
    }
}

static BoundaryJob boundary_job(const int* rowptr, const int* dstS, int n_nodes, int edge_capacity, int H, float* out, int ldo, int rep_out,
                                int slots, int tile_rows, int run, int* ovf) {
    BoundaryJob b = {};
    b.rowptr = rowptr; b.dstS = dstS; b.n_nodes = n_nodes; b.H = H; b.out = out; b.ldo = ldo; b.rep_out = rep_out;
    b.tile_rows = tile_rows; b.run = run; b.replicas = slots; b.ovf = ovf;
    const int n_cand = cdiv((long)cdiv(edge_capacity, tile_rows) * slots, run) - 1;      // upper bound (capacity >= E')
    b.n_cand = n_cand > 0 ? n_cand : 0;
    return b;
}

static int init_boundary_rows(const BoundaryJob* jobs, int n, hipStream_t s) {
    BoundaryJobs js = {};
    int m = 0, most = 0;
    for (int i = 0; i < n; ++i) if (jobs[i].n_cand > 0) { js.j[m++] = jobs[i]; most = jobs[i].n_cand > most ? jobs[i].n_cand : most; }
    if (m == 0) return MORIG_OK;
    hipLaunchKernelGGL(init_boundary_rows_kernel, dim3(cdiv(most, 256), m), dim3(256), 0, s, js);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

static int init_boundary_rows(const int* rowptr, const int* dstS, int n_nodes, int edge_capacity, int H, float* out, int ldo,
                              int rep_out, int slots, hipStream_t s, int tile_rows = 128, int run = 1) {
    const BoundaryJob b = boundary_job(rowptr, dstS, n_nodes, edge_capacity, H, out, ldo, rep_out, slots, tile_rows, run, nullptr);
    return init_boundary_rows(&b, 1, s);
}

// out_split launches (edge_rl.hip / edge_ws.hip): whole segments leave the kernel as split-fp16 halves, the shared rows above as fp32
// atomics -- the only rows still in fp32 afterwards. This pass rewrites exactly those rows in place (a 32-column chunk occupies the
// same 128 bytes in both layouts: a lane reads 4 adjacent columns, then stores their 4 hi and 4 lo halves over the chunk; a wave
// instruction covers whole chunks, so every read of a chunk precedes every write to it). A segment that straddles several shared
// boundaries is converted at the LAST one (once). Same lane-per-candidate index phase as the pass above; the rows are taken four at a
// time so that four loads are in flight.
__global__ __launch_bounds__(256) void split_boundary_rows_kernel(const BoundaryJobs js) {
    const BoundaryJob& b = js.j[blockIdx.y];
    if ((int)blockIdx.x * 64 >= b.n_cand) return;
    const int* __restrict__ rowptr = b.rowptr; const int* __restrict__ dstS = b.dstS;
    float* __restrict__ out = b.out;
    int* __restrict__ ovf = b.ovf;
    const int H = b.H, ldo = b.ldo;
    // 16 candidates per wave (lanes 0..15 run the index chain): a wave converts its rows one group of four after the other, a load
    // round trip each -- with 64 candidates per wave the launch was one long latency chain (24 us on average for 5 k rows)
    const int lane = threadIdx.x & 63;
    const int g = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + lane + 1;
    const int d = lane < 16 ? straddled_row(rowptr, dstS, b.n_nodes, b.tile_rows, b.run, b.replicas, b.rep_out, g, b.n_cand, true) : -1;
    unsigned long long todo = __ballot(d >= 0);
    float am = 0.f;
    bool bad = false;                                                 // a NaN: fmaxf drops NaN operands, so the amax below never sees one
    while (todo) {                                                    // wave-uniform
        int dr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = todo ? __builtin_ctzll(todo) : -1;
            todo &= todo - 1;                                         // (0 stays 0)
            dr[i] = l >= 0 ? __builtin_amdgcn_readlane(d, l) : -1;
        }
        for (int c0 = 0; c0 < H; c0 += 256) {
            const int c = c0 + 4 * lane;
            float4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (dr[i] >= 0 && c < H) v[i] = *reinterpret_cast<const float4*>(out + (size_t)dr[i] * ldo + c);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (dr[i] >= 0 && c < H) {
                    float h0, l0, h1, l1;
                    split_pair_f16(v[i].x, v[i].y, h0, l0);
                    split_pair_f16(v[i].z, v[i].w, h1, l1);
                    am = fmaxf(am, fmaxf(fmaxf(fabsf(v[i].x), fabsf(v[i].y)), fmaxf(fabsf(v[i].z), fabsf(v[i].w))));
                    bad |= !(v[i].x == v[i].x && v[i].y == v[i].y && v[i].z == v[i].z && v[i].w == v[i].w);
                    char* oc = reinterpret_cast<char*>(out + (size_t)dr[i] * ldo) + (c >> 5) * 128 + (c & 31) * 2;
                    *reinterpret_cast<float2*>(oc) = make_float2(h0, h1);
                    *reinterpret_cast<float2*>(oc + 64) = make_float2(l0, l1);
                }
        }
    }
    // range guard on the converted rows; a NaN -- a result, or a shared row still at the identity pattern 0xFFFFFFFF because no atomic
    // reached it (would be a bug: both tiles of a boundary write the row) -- is raised by its own test (fmaxf hides it)
    if (bad || !(am < FP16_RANGE_GUARD)) *ovf = 1;
}

static int split_boundary_rows(const BoundaryJob* jobs, int n, hipStream_t s) {
    BoundaryJobs js = {};
    int m = 0, most = 0;
    for (int i = 0; i < n; ++i) if (jobs[i].n_cand > 0) { js.j[m++] = jobs[i]; most = jobs[i].n_cand > most ? jobs[i].n_cand : most; }
    if (m == 0) return MORIG_OK;
    hipLaunchKernelGGL(split_boundary_rows_kernel, dim3(cdiv(most, 64), m), dim3(256), 0, s, js);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

// ------------------------------------------------------------------------------------------------
template <int BN, int KC, int LOAD, int MODE, int PREC>
static int launch_tile_row(bool fast, const TileParams& p, int nblocks, hipStream_t s) {
    if constexpr (tile_has_fast(BN, KC, LOAD, MODE)) {
        if (fast) {
            hipLaunchKernelGGL((tile_kernel<BN, KC, LOAD, MODE, PREC, true>), dim3(nblocks), dim3(256), 0, s, p);
            MORIG_LAUNCH_CHECK();
            return MORIG_OK;
        }
    }
    hipLaunchKernelGGL((tile_kernel<BN, KC, LOAD, MODE, PREC>), dim3(nblocks), dim3(256), 0, s, p);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

// The one launcher of the tile engine: every row of MORIG_TILE_TABLE (dispatch_core.h) is instantiated here and nowhere else.
static int launch_tile(const TileInst& t, const TileParams& p0, int nblocks, hipStream_t s) {
    TileParams p = p0;
    p.dbg = debug_flags();
    switch (tile_key(t)) {
#define MORIG_TILE_ROW(BN, KC, LOAD, MODE, PREC) \
        case tile_key(BN, KC, LOAD, MODE, PREC): return launch_tile_row<BN, KC, LOAD, MODE, PREC>(t.fast, p, nblocks, s);
        MORIG_TILE_TABLE(MORIG_TILE_ROW)
#undef MORIG_TILE_ROW
        default: return MORIG_E_UNSUPPORTED;
    }
}

// scatter_max semantics for segments that received no row (a graph id without vertices): torch_scatter fills 0; the
// integer-atomic max leaves its identity pattern 0xFFFFFFFF (a NaN) there, which would then flag every split of the row
__global__ void pool_identity_to_zero_kernel(float* __restrict__ pool, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned* u = reinterpret_cast<unsigned*>(pool);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) if (u[i] == 0xFFFFFFFFu) u[i] = 0u;
}
static int pool_finalize(float* pool, int n_seg, int ld_pool, hipStream_t s) {
    const int64_t n = (int64_t)n_seg * ld_pool;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pool_identity_to_zero_kernel, dim3((int)blocks), dim3(256), 0, s, pool, n);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // namespace morig

using namespace morig;

// Every entry point below: take the arguments, ask dispatch_core.h for the plan, return on a refusal, fill the parameter struct of the
// engine the plan names, open the ProfScope, run the boundary passes, launch. Why a call takes which kernel is written in the plans.

extern "C" int morig_gemm(const morig_gemm_args* a_in, void* stream) {
    morig_gemm_args mine;
    if (!take_args(a_in, mine, MORIG_GEMM_ARGS_V3_SIZE)) return MORIG_E_INVALID;
    const morig_gemm_args* a = &mine;
    const GemmPlan pl = gemm_plan(mine, gemm_switches());
    if (pl.status != MORIG_OK || pl.engine == GEMM_NONE) return pl.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool pool = a->pool != nullptr, f16 = a->W_split != nullptr;
    const double flops = 2.0 * a->M * (double)a->N * a->K;
    const double bytes = 4.0 * ((double)a->M * a->K + (double)a->N * a->K + (pool ? 0.0 : (double)a->M * a->N));
    // identity of the integer-atomic float max
    if (pool) MORIG_HIP_TRY(hipMemsetAsync(a->pool, 0xFF, (size_t)a->n_seg * a->ld_pool * sizeof(float), s));
    ProfScope ps(pl.kind, s, flops, bytes);
    if (pl.retag >= 0) prof_retag(pl.retag);
    int st;
    if (pl.engine == GEMM_FEW_ROWS) {
        st = launch_few_rows_gemm(a->X, a->ldx, a->M, a->W, a->ldw, a->N, a->K, a->bias, a->scale, a->shift, a->relu, a->Y, a->ldy, s);
    } else if (pl.engine == GEMM_TILE) {
        TileParams p = {};
        p.M = a->M; p.N = a->N; p.K = a->K;
        p.W = f16 ? static_cast<const float*>(a->W_split) : a->W; p.ldw = a->ldw;
        p.bias = a->bias; p.scale = a->scale; p.shift = a->shift; p.relu = a->relu;
        p.X = a->X; p.ldx = a->ldx;
        p.rowbias = a->rowbias; p.ld_rowbias = a->ld_rowbias; p.seg = a->seg;
        p.Y = pool ? a->pool : a->Y; p.ldy = pool ? a->ld_pool : a->ldy;
        p.tiles_n = pl.tiles_n;
        if (f16) p.ovf = a->overflow;
        p.x16 = a->x_split ? 1 : 0; p.y16 = a->y_split ? 1 : 0;
        st = launch_tile(pl.tile, p, pl.blocks, s);
    } else {
        GemmDmaParams q = {};
        q.M = a->M; q.N = a->N; q.K = a->K; q.X = a->X; q.ldx = a->ldx;
        q.W = static_cast<const float*>(a->W_split); q.ldw = a->ldw;
        q.bias = a->bias; q.scale = a->scale; q.shift = a->shift; q.relu = a->relu; q.seg = a->seg; q.ovf = a->overflow;
        if (pool) { q.pool = a->pool; q.ld_pool = a->ld_pool; }
        else {
            q.rowbias = a->rowbias; q.ld_rowbias = a->ld_rowbias;
            q.Y = a->Y; q.ldy = a->ldy; q.y16 = a->y_split ? 1 : 0;
            if (pl.tail) { q.Xt = a->X_tail; q.ldt = a->ld_tail; q.tail_rows = a->tail_rows; q.tail_chunks = a->tail_cols / 32; }
        }
        st = launch_gemm16_dma(q, pl, s);
    }
    return (st != MORIG_OK || !pool) ? st : pool_finalize(a->pool, a->n_seg, a->ld_pool, s);
}

// the tile engine's parameters of an EdgeConv / edge-hidden launch
static TileParams edge_tile_params(const morig_edgeconv_args* a) {
    TileParams p = {};
    p.M = a->edge_capacity; p.N = a->H; p.K = a->H;
    p.W = a->W2_split ? static_cast<const float*>(a->W2_split) : a->W2; p.ldw = a->ldw;
    p.bias = a->b2; p.scale = a->s2; p.shift = a->t2; p.relu = 1;
    p.A = a->A; p.lda = a->lda; p.B = a->B; p.ldb = a->ldb;
    p.rowptr = a->rowptr; p.srcS = a->src_sorted; p.dstS = a->dst_sorted;
    p.n_nodes = a->n_nodes; p.rep_in = a->in_rep_stride; p.rep_out = a->out_rep_stride;
    p.s1 = a->s1; p.t1 = a->t1;
    p.Y = a->out; p.ldy = a->ldo;
    p.tiles_per_rep = cdiv(a->edge_capacity, 128);
    p.tiles_n = 1;
    if (a->W2_split) p.ovf = a->overflow;
    return p;
}

extern "C" int morig_edge_hidden(const morig_edgeconv_args* a_in, void* stream) {
    morig_edgeconv_args mine;
    if (!take_args(a_in, mine, MORIG_EDGECONV_ARGS_V3_SIZE)) return MORIG_E_INVALID;
    const morig_edgeconv_args* a = &mine;
    const EdgePlan pl = edge_hidden_plan(mine, switches());
    if (pl.status != MORIG_OK) return pl.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double E = (double)(a->edge_count > 0 ? a->edge_count : a->edge_capacity);
    ProfScope ps(pl.kind, s, 2.0 * E * a->H * (double)a->H, 4.0 * 3.0 * E * a->H);
    return launch_tile(pl.tile, edge_tile_params(a), pl.blocks, s);
}

extern "C" int morig_segmax_gemm(const morig_segmax_args* a_in, void* stream) {
    morig_segmax_args mine;
    if (!take_args(a_in, mine, MORIG_SEGMAX_ARGS_V3_SIZE)) return MORIG_E_INVALID;
    const morig_segmax_args* a = &mine;
    const EdgePlan pl = segmax_plan(mine, switches());
    if (pl.status != MORIG_OK) return pl.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TileParams p = {};
    p.M = a->edge_capacity; p.N = a->N; p.K = a->K;
    p.W = a->W_split ? static_cast<const float*>(a->W_split) : a->W; p.ldw = a->ldw;
    p.bias = a->bias; p.scale = a->scale; p.shift = a->shift; p.relu = a->relu;
    p.X = a->X; p.ldx = a->ldx;
    p.rowptr = a->rowptr; p.dstS = a->dst_sorted; p.n_nodes = a->n_nodes;
    p.Y = a->out; p.ldy = a->ldo;
    p.tiles_per_rep = pl.blocks;
    p.tiles_n = 1;
    if (a->W_split) p.ovf = a->overflow;
    { const int st = init_boundary_rows(a->rowptr, a->dst_sorted, a->n_nodes, a->edge_capacity, a->N, a->out, a->ldo, 0, 1, s);
      if (st != MORIG_OK) return st; }
    const double E = (double)(a->edge_count > 0 ? a->edge_count : a->edge_capacity);
    ProfScope ps(pl.kind, s, 2.0 * E * a->N * (double)a->K, 4.0 * E * a->K);
    return launch_tile(pl.tile, p, pl.blocks, s);
}

extern "C" int morig_edgeconv_can_split_out(const morig_edgeconv_args* a_in) {
    morig_edgeconv_args mine;
    if (!take_args(a_in, mine, MORIG_EDGECONV_ARGS_V3_SIZE)) return 0;
    return edge_plan(mine, edge_switches(), true).split_ok ? 1 : 0;
}

extern "C" int morig_edgeconv(const morig_edgeconv_args* a_in, void* stream) {
    morig_edgeconv_args mine;
    if (!take_args(a_in, mine, MORIG_EDGECONV_ARGS_V3_SIZE)) return MORIG_E_INVALID;
    const morig_edgeconv_args* a = &mine;
    const Switches sw = edge_switches();
    const EdgePlan pl = edge_plan(mine, sw);
    if (pl.status != MORIG_OK && !pl.late) return pl.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    // tile-straddling target segments combine through integer-atomic float max: identity in exactly those rows -- of this launch and,
    // with init_with, of the partner launch that follows (which then comes with skip_init). With out_split the rows two tiles share were
    // combined as fp32 atomics and go into the split layout behind the kernel (skip_split: the partner's pass does it, behind its own
    // kernel; split_with: this pass also converts the partner's rows, whose kernel ran in front of this one).
    auto job_of = [](const morig_edgeconv_args* q, const EdgePlan& qp) {
        return boundary_job(q->rowptr, q->dst_sorted, q->n_nodes, q->edge_capacity, q->H, q->out, q->ldo, q->out_rep_stride, q->replicas,
                            qp.tile_rows, qp.run, q->overflow);
    };
    // the partner's arguments, checked as its own call will check them (nothing of it is launched here but the pass over its rows)
    morig_edgeconv_args other;
    auto partner = [&](const morig_edgeconv_args* q_in, EdgePlan& qp) -> int {
        if (!take_args(q_in, other, MORIG_EDGECONV_ARGS_V3_SIZE)) return MORIG_E_INVALID;
        qp = edge_plan(other, sw);
        return qp.late ? MORIG_OK : qp.status;
    };
    BoundaryJob init_jobs[2], split_jobs[2];
    int n_init = 0, n_split = 0;
    if (!a->skip_init) {
        init_jobs[n_init++] = job_of(a, pl);
        if (a->init_with) {
            EdgePlan qp;
            const int stp = partner(a->init_with, qp);
            if (stp != MORIG_OK) return stp;
            init_jobs[n_init++] = job_of(&other, qp);
        }
    }
    if (pl.status != MORIG_OK) return pl.status;
    if (edge_splits(pl) && a->out_split && !a->skip_split) {
        split_jobs[n_split++] = job_of(a, pl);
        if (a->split_with) {
            EdgePlan qp;
            const int stp = partner(a->split_with, qp);
            if (stp != MORIG_OK) return stp;
            if (!other.out_split || !edge_splits(qp)) return MORIG_E_INVALID;
            split_jobs[n_split++] = job_of(&other, qp);
        }
    }
    { const int st = init_boundary_rows(init_jobs, n_init, s);
      if (st != MORIG_OK) return st; }

    const double E = (double)(a->edge_count > 0 ? a->edge_count : a->edge_capacity) * a->replicas;
    const double flops = 2.0 * E * a->H * (double)a->H;
    // compulsory bytes: every row of the [A | B] operand tables and every result row ONCE (the per-edge re-reads of gathered rows are L2
    // hits: what they cost shows as traffic ABOVE this figure in bench.py's roofline.traffic_over_algorithmic)
    const double bytes = 4.0 * a->H * (double)a->n_nodes * (2.0 * (a->in_rep_stride > 0 ? a->replicas : 1) + a->replicas);
    ProfScope ps(pl.kind, s, flops, bytes);
    if (pl.retag >= 0) prof_retag(pl.retag);
    if (pl.engine == EDGE_TILE) return launch_tile(pl.tile, edge_tile_params(a), pl.blocks, s);
    if (pl.engine == EDGE_X3) {
        EdgeX3Params q = {};
        q.A = a->A; q.lda = a->lda; q.B = a->B; q.ldb = a->ldb;
        q.W2s = static_cast<const float*>(a->W2_split); q.ldw = a->ldw;
        q.bias = a->b2; q.scale = a->s2; q.shift = a->t2;
        q.rowptr = a->rowptr; q.srcS = a->src_sorted; q.dstS = a->dst_sorted; q.n_nodes = a->n_nodes; q.cap = a->edge_capacity;
        q.rep_in = a->in_rep_stride; q.rep_out = a->out_rep_stride; q.replicas = a->replicas;
        q.Y = a->out; q.ldy = a->ldo; q.ovf = a->overflow;
        return launch_edge_x3(q, pl.blocks, s);
    }
    // H = 256 / 128: the wave-specialised kernels
    EdgePcParams q = {};
    q.H = a->H; q.W = static_cast<const float*>(a->W2_split); q.ldw = a->ldw; q.bias = a->b2; q.scale = a->s2; q.shift = a->t2;
    q.A = a->A; q.lda = a->lda; q.B = a->B; q.ldb = a->ldb;
    q.rowptr = a->rowptr; q.srcS = a->src_sorted; q.dstS = a->dst_sorted; q.n_nodes = a->n_nodes;
    q.rep_in = a->in_rep_stride; q.rep_out = a->out_rep_stride; q.tiles_per_rep = cdiv(a->edge_capacity, 128); q.replicas = a->replicas;
    q.Y = a->out; q.ldy = a->ldo; q.ovf = a->overflow; q.quad = a->quad_aligned ? 1 : 0; q.min4 = a->seg_min4 ? 1 : 0;
    q.y16 = a->out_split ? 1 : 0; q.run = pl.run;
    int st;
    switch (pl.engine) {
        case EDGE_RL: st = launch_edge_rl(q, pl.blocks, s); break;
        case EDGE_PC: st = launch_edge_pc(q, pl.blocks, s); break;
        case EDGE_PP: st = launch_edge_pp(q, pl.blocks, s); break;
        default:      st = launch_edge_ws(q, pl.blocks, s); break;      // EDGE_WS, EDGE_WS_MIX
    }
    return st != MORIG_OK ? st : split_boundary_rows(split_jobs, n_split, s);
}

// EdgeConv whose vertex input has 3 channels: first Linear evaluated in the loader from the gathered endpoints (LOAD_EDGE3), then the
// 32-wide second layer + max exactly as morig_edgeconv. Replaces `morig_gemm` (K = 3 -> [A | B]) + `morig_edgeconv` for the position
// branches (models/basic_modules.py:193-195: nn_pos([pos_i, pos_j - pos_i])) and for motionNet's first unit (nn_x on the 3-channel flow).
extern "C" int morig_edgeconv_x3(const morig_edgeconv_x3_args* a_in, void* stream) {
    morig_edgeconv_x3_args mine;
    if (!take_args(a_in, mine, MORIG_EDGECONV_X3_ARGS_V3_SIZE)) return MORIG_E_INVALID;
    const morig_edgeconv_x3_args* a = &mine;
    const EdgePlan pl = edgeconv_x3_plan(mine, switches());
    if (pl.status != MORIG_OK) return pl.status;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!a->skip_init) {
        BoundaryJob jobs[2];
        int nj = 0;
        jobs[nj++] = boundary_job(a->rowptr, a->dst_sorted, a->n_nodes, a->edge_capacity, 32, a->out, a->ldo, a->out_rep_stride, a->replicas, 128, 1, nullptr);
        if (a->init_with) {                                // the partner launch that follows (with skip_init): its rows in the same pass
            morig_edgeconv_x3_args o;
            if (!take_args(a->init_with, o, MORIG_EDGECONV_X3_ARGS_V3_SIZE)) return MORIG_E_INVALID;
            if (!o.rowptr || !o.dst_sorted || !o.out || o.H != 32 || o.n_nodes <= 0 || o.replicas <= 0 || o.edge_capacity <= 0 || o.ldo < 32 ||
                (o.replicas > 1 && o.out_rep_stride < o.n_nodes)) return MORIG_E_INVALID;
            jobs[nj++] = boundary_job(o.rowptr, o.dst_sorted, o.n_nodes, o.edge_capacity, 32, o.out, o.ldo, o.out_rep_stride, o.replicas, 128, 1, nullptr);
        }
        const int st2 = init_boundary_rows(jobs, nj, s);
        if (st2 != MORIG_OK) return st2;
    }
    const double E = (double)(a->edge_count > 0 ? a->edge_count : a->edge_capacity) * a->replicas;
    // algorithmic work: second layer 2 H^2 + first layer 2 * 6 * H per edge row; bytes: the two gathered 16-byte inputs
    ProfScope ps(pl.kind, s, E * (2.0 * 32 * 32 + 12.0 * 32), 32.0 * E);
    if (pl.retag >= 0) prof_retag(pl.retag);
    if (pl.engine == EDGE_X3) {
        EdgeX3Params q = {};
        q.X = a->X; q.ldx = a->ldx; q.W1a = a->W1a; q.W1b = a->W1b; q.b1 = a->b1;
        q.W2s = static_cast<const float*>(a->W2_split); q.ldw = a->ldw;
        q.bias = a->b2; q.scale = a->s2; q.shift = a->t2;
        q.rowptr = a->rowptr; q.srcS = a->src_sorted; q.dstS = a->dst_sorted; q.n_nodes = a->n_nodes; q.cap = a->edge_capacity;
        q.rep_in = a->in_rep_stride; q.rep_out = a->out_rep_stride; q.replicas = a->replicas;
        q.Y = a->out; q.ldy = a->ldo; q.ovf = a->overflow;
        return launch_edge_x3(q, pl.blocks, s);
    }
    TileParams p = {};
    p.M = a->edge_capacity; p.N = 32; p.K = 32;
    p.W = a->W2_split ? static_cast<const float*>(a->W2_split) : a->W2; p.ldw = a->ldw;
    p.bias = a->b2; p.scale = a->s2; p.shift = a->t2; p.relu = 1;
    p.X3 = a->X; p.ldx3 = a->ldx; p.W1a = a->W1a; p.W1b = a->W1b; p.b1 = a->b1;
    p.rowptr = a->rowptr; p.srcS = a->src_sorted; p.dstS = a->dst_sorted;
    p.n_nodes = a->n_nodes; p.rep_in = a->in_rep_stride; p.rep_out = a->out_rep_stride;
    p.Y = a->out; p.ldy = a->ldo;
    p.tiles_per_rep = cdiv(a->edge_capacity, 128);
    p.tiles_n = 1;
    if (a->W2_split) p.ovf = a->overflow;
    return launch_tile(pl.tile, p, pl.blocks, s);
}
