/*
 * morig_hip.h -- C ABI of libmorig_hip.so: the MI355X (gfx950) kernels behind MoRig's
 * geometric-network forward path.
 *
 * Boundary contract:
 *   - plain `extern "C"` functions, plain pointers and sizes, no C++/torch types;
 *   - every buffer is DEVICE memory owned by the caller (PyTorch-ROCm allocates it); the library
 *     borrows pointers for the duration of the call and keeps nothing;
 *   - every call enqueues asynchronously on the given hipStream_t (passed as void*); no hidden
 *     device synchronisation (the profiling collector is the one documented exception);
 *   - every call returns 0 or a negative MORIG_E_* code; no exceptions, no abort().
 *
 * The reference has no FFI of its own: its native work is delegated to three un-vendored wheels.
 * Each entry point therefore names the reference CALL SITE (file:line under /root/reference) whose
 * third-party operator it replaces; INTEGRATION.md shows the Python binding a maintainer would add.
 *
 * All matrices are row-major fp32. "ld" = row stride in floats. Unless noted, ld and the column
 * offset of a matrix handed to a GEMM-type call must be multiples of 4 floats (16-byte rows).
 *
 * GRAMMAR. This file is also the source of the Python binding: morig_amd/abi.py reads it when the package is imported and builds the
 * ctypes structs, signatures and constants from it (there is no second copy to keep in step), and refuses what it cannot read. So,
 * with comments, preprocessor lines and the `extern "C"` braces taken away, every statement here is one of
 *     typedef struct NAME { members } NAME;          (tag and typedef name equal; members `TYPE a, b;`, several to a line allowed)
 *     RET morig_name(TYPE name, ...);                 (or `(void)`; every parameter named)
 * over the types int, int32_t, uint32_t, int64_t, uint64_t, float, double, one-level pointers to those, to void, char, uint8_t or to an
 * argument struct declared above (or, in a member, the struct itself), and void**. No arrays, unions, enums, function pointers, nested
 * structs, bit fields or line continuations. A constant the binding should see is an object-like `#define MORIG_X <integer>[u]`.
 */
#ifndef MORIG_HIP_H
#define MORIG_HIP_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): morig_gemm_args.w_split_format and morig_edgeconv_args.out_split appended to their structs; morig_gemm_tn_shift,
 * morig_edgeconv_can_split_out, morig_ubench_mfma added.
 * 3 (round 6): every argument struct STARTS with `uint32_t struct_size` (see below): appending a member no longer lets the library read
 * past the end of an older caller's struct. morig_gemm_args gained X_tail / ld_tail / tail_rows / tail_cols; morig_pack_tails added. */
#define MORIG_ABI_VERSION 3

/* Argument structs (morig_gemm_args, morig_edgeconv_args, morig_edgeconv_x3_args, morig_segmax_args, morig_pointconv_args):
 * the first member, struct_size, is sizeof() of the struct AS THE CALLER WAS COMPILED (MORIG_INIT_ARGS sets it and zeroes the rest).
 * Members are only ever appended. The library copies min(struct_size, its own sizeof) bytes into a zeroed struct of its own, so members
 * the caller does not know read as 0 / NULL; a struct_size below the ABI-3 size of the struct (MORIG_*_ARGS_V3_SIZE: what a version-1 / -2
 * caller's memory would spell there, or garbage) is MORIG_E_INVALID. */
#define MORIG_INIT_ARGS(type, var) type var; memset(&(var), 0, sizeof(var)); (var).struct_size = (uint32_t)sizeof(var)
#define MORIG_GEMM_ARGS_V3_SIZE        192u
#define MORIG_EDGECONV_ARGS_V3_SIZE    192u
#define MORIG_EDGECONV_X3_ARGS_V3_SIZE 168u
#define MORIG_SEGMAX_ARGS_V3_SIZE      144u
#define MORIG_POINTCONV_ARGS_V3_SIZE   176u
/* members appended since (a struct only grows at its end; a caller built against the smaller struct passes its own size and the library reads
 * the new members as 0): round 6 -- init_with / split_with / skip_init / skip_split of morig_edgeconv_args, init_with / skip_init of
 * morig_edgeconv_x3_args. sizeof of the CURRENT structs: */
#define MORIG_EDGECONV_ARGS_SIZE       216u
#define MORIG_EDGECONV_X3_ARGS_SIZE    184u

/* status codes */
#define MORIG_OK              0
#define MORIG_E_INVALID      -1   /* null pointer, negative size, misaligned ld ...            */
#define MORIG_E_UNSUPPORTED  -2   /* width / shape the kernels are not instantiated for        */
#define MORIG_E_HIP          -3   /* a HIP runtime call failed; see morig_last_hip_error()      */
#define MORIG_E_NODEVICE     -4   /* no gfx950 device visible                                   */

int         morig_abi_version(void);
/* Scheduling hint, process-wide: leave n CUs (rounded up to 8) free of the persistent EdgeConv workgroups launched from now
 * on. The host sets it while single-CU-per-cloud kernels (FPS) run on a second stream, and back to 0 afterwards. */
int         morig_reserve_cus(int n);
const char* morig_strerror(int status);
int         morig_last_hip_error(void);            /* raw hipError_t of the last MORIG_E_HIP   */
/* device facts used by the host side for roofline arithmetic; arch must start with "gfx950" */
int         morig_device_info(int* cu_count, int* lds_bytes_per_cu, int* clock_khz, char* arch, int arch_len);

/* --------------------------------------------------------------------------------------------
 * Graph preparation: COO -> self-loop-normalised CSR by destination.
 * Replaces, once per forward instead of once per conv:
 *   remove_self_loops + add_self_loops            models/basic_modules.py:149-150, 188-189
 *   the implicit sort-free scatter of MessagePassing.propagate(aggr='max')  (:151, :190)
 *
 * edge_index : int64 [2, n_edges] contiguous (row 0 = source j, row 1 = target i), as PyG batches it
 * rowptr     : int32 [n_nodes + 1]   out; rowptr[n_nodes] = E' = #(non-loop edges) + n_nodes
 * src_sorted : int32 [n_edges + n_nodes] out (capacity; entries beyond E' untouched)
 * dst_sorted : int32 [n_edges + n_nodes] out (target of every sorted edge, i.e. expanded rowptr)
 * cursor     : int32 [n_nodes + 1]   scratch
 * status     : int32 [1] out; set non-zero when an index is outside [0, n_nodes)
 * Order inside a target's segment is unspecified (max-aggregation is order-free => results are
 * bit-identical for any order).
 */
int morig_csr_build(const int64_t* edge_index, int64_t n_edges, int32_t n_nodes,
                    int32_t* rowptr, int32_t* src_sorted, int32_t* dst_sorted,
                    int32_t* cursor, int32_t* status, void* stream);
/* bipartite form used by PointConv (PyG applies remove_self_loops/add_self_loops(num_nodes =
 * min(N_src, N_dst)) to the raw (source, target) index pairs even though they index different sets):
 * sources in [0, n_src_nodes), targets in [0, n_nodes), n_src_nodes >= n_nodes; pairs with a negative
 * index (unused ball-query slots) are skipped with MORIG_CSR_SKIP_NEGATIVE. */
#define MORIG_CSR_SKIP_NEGATIVE 1   /* pairs with a negative index are skipped instead of flagged            */
#define MORIG_CSR_PAD4          2   /* every target's segment is padded to a multiple of 4 entries by repeating
                                       its self loop (max-aggregation is idempotent); capacity n_edges + 4*n_nodes.
                                       morig_edgeconv's `quad_aligned` fast epilogue requires it.              */
#define MORIG_CSR_MIN4          4   /* morig_csr_build_bipartite (not with PAD4) / morig_csr_build_dual: every segment of the PLAIN CSR holds at least 4 rows (a shorter one is filled
                                       up with copies of its self loop; capacity n_edges + 4*n_nodes). A quad of 4 consecutive rows then
                                       never holds more than two segments, which is what morig_edgeconv's `seg_min4` form needs: the
                                       H = 256 kernel reduces a quad that straddles two segments into two values instead of requiring
                                       4-ALIGNED segments (MORIG_CSR_PAD4 costs 9-14 % extra rows on the rig graphs, this ~0).           */
int morig_csr_build_bipartite(const int64_t* edge_index, int64_t n_edges, int32_t n_src_nodes, int32_t n_nodes,
                              int32_t flags, int32_t* rowptr, int32_t* src_sorted, int32_t* dst_sorted,
                              int32_t* cursor, int32_t* status, void* stream);

/* --------------------------------------------------------------------------------------------
 * Arithmetic. Default: fp32 operands on v_mfma_f32_32x32x2_f32 (exact fp32 products, k-ordered fma).
 * Split-fp16 fast path (selected per call by passing W_split): each fp32 operand x is split on the fly
 * into hi = fp16(x), lo = fp16(x - hi) and the product evaluated as hi*hi + hi*lo + lo*hi on
 * v_mfma_f32_32x32x16_f16 with fp32 accumulation -- fp16 products are exact in fp32 and the omitted
 * lo*lo term is 2^-22 relative, so the result is fp32-class (measured ~1e-6 of scale) at 5.3x the
 * fp32-MFMA rate. Weights are pre-split by the host: every 32-float chunk of a packed weight row is
 * replaced by [32 halves hi | 32 halves lo] (same bytes, same strides). Operands must stay inside the
 * fp16 range (|x| < 65000); otherwise the kernel raises *overflow and the caller must redo the layer
 * on the fp32 path (morig_amd.models does this for the whole forward).
 *
 * Fused dense layer:  Y = scale * act(X * W^T + bias + rowbias[seg[row]]) + shift
 *                     and/or  P[seg[row]] = max over rows (column-wise)            (pool != NULL)
 * Replaces nn.Linear -> ReLU -> BatchNorm1d(eval) chains of MLP()   models/basic_modules.py:31-36
 * and, with `pool`, scatter_max(x, batch) + repeat_interleave       models/rignet.py:62-64, 175-179,
 *                                                                   models/corrnet.py:43-45
 * (the broadcast is never materialised: the pooled vector enters the next layer as `rowbias`).
 */
#define MORIG_SPLIT_F16 0
#define MORIG_SPLIT_BF16 1
#define MORIG_SPLIT_BF16X6 2   /* [ABI 3] W_split == NULL: plain fp32 X and W, both split into three bf16 limbs IN the kernel, six MFMAs per
                                  product: float32-class results (dropped terms <= 2^-24 relative), float32's exponent range (no range word),
                                  2.7x the fp32-MFMA rate. What the train-mode forward and the exact re-run behind the range guard take
                                  instead of v_mfma_f32_32x32x2_f32. Plain stores and pooled launches. */
typedef struct morig_gemm_args {
    uint32_t struct_size;     /* sizeof(morig_gemm_args) of the caller's build (ABI 3)                */
    int32_t M, N, K;          /* logical sizes: Y is M x N, X is M x K                            */
    const float* X; int32_t ldx;
    const float* W; int32_t ldw;     /* packed weights [Npad][ldw]: row n = output channel n, ldw >= roundup(K,32),
                                        zero padded; Npad = N rounded up to the column tile (32/64/128; with `pool` always 128:
                                        the pooled launch reads W / bias / scale / shift up to that row whatever N is) */
    const float* bias;        /* [Npad] or NULL                                                   */
    const float* scale;       /* [Npad] or NULL (=1): BatchNorm eval scale  gamma/sqrt(var+eps)   */
    const float* shift;       /* [Npad] or NULL (=0): BatchNorm eval shift  beta - mean*scale     */
    int32_t relu;             /* 1: act = ReLU, 0: identity                                       */
    const float* rowbias; int32_t ld_rowbias;   /* optional [n_seg][ld_rowbias] added before act  */
    const int32_t* seg;       /* [M] segment (mesh) id of every row; required with rowbias / pool */
    float* Y; int32_t ldy;    /* optional output                                                  */
    float* pool; int32_t ld_pool; int32_t n_seg;  /* optional [n_seg][ld_pool] column max per segment; a segment without rows
                                                   * receives 0 (torch_scatter's fill) */
    /* optional fast path (see "split-fp16" below): W_split has the shape/stride of W; overflow is an int32
     * on the device that the kernel sets to 1 if an operand left the fp16 range (result then invalid).
     * w_split_format = MORIG_SPLIT_BF16 selects the bf16 split instead: W_split then holds bf16 halves
     * (hi = bf16(w), lo = bf16(w - hi), same layout), X is split the same way in the kernel and the three products
     * run on v_mfma_f32_32x32x16_bf16 -- bf16 keeps float32's exponent range, so there is no range condition to
     * report (overflow may be NULL); ~16 mantissa bits per operand. Plain stores only (no pool, no split
     * activations): the gradient contractions of the training path (dX = dU W). With MORIG_SPLIT_F16 (= 0) a
     * missing overflow word is MORIG_E_INVALID: the format is never inferred from a NULL pointer. */
    const void* W_split; int32_t* overflow;
    /* split-fp16 ACTIVATIONS (only with W_split): a matrix window whose first column and row stride are
     * multiples of 32 floats and whose every aligned 32-column chunk holds [32 halves hi | 32 halves lo].
     * x_split: X is in that layout (loader becomes a plain copy: the hi/lo split was done once by the
     * producer instead of once per column tile); y_split: write Y in that layout. */
    int32_t x_split, y_split;
    int32_t w_split_format;   /* MORIG_SPLIT_F16 (0) or MORIG_SPLIT_BF16 (1): what W_split holds */
    /* [ABI 3] optional K TAIL (x_split launches only): the last tail_cols columns of X -- columns [K - tail_cols, K); tail_cols % 32 == 0,
     * K % 32 == 0, K > tail_cols -- are read from X_tail[row % tail_rows] instead of X[row]: 128-byte aligned rows of ld_tail floats
     * (ld_tail % 32 == 0, >= tail_cols) in the split-fp16 chunk layout. This is how a replica-invariant block of a concatenated input
     * enters without being copied into every replica's row: the position-branch features [pos_tpl | pos_geo] of a GCUMotion unit under
     * the keyframe loop (models/basic_modules.py:216-217 inside models/rignet.py:85-86; rows r * n + v of the 5 replicas all read tail
     * row v). X then needs only ldx >= K - tail_cols. MORIG_E_UNSUPPORTED where the launch would not take the LDS-DMA store kernel
     * (N % 256 != 0, pool, misaligned Y): the caller copies the block into X instead (morig_copy2d_pad_rep). */
    const float* X_tail; int32_t ld_tail, tail_rows, tail_cols;
} morig_gemm_args;
int morig_gemm(const morig_gemm_args* a, void* stream);

/* --------------------------------------------------------------------------------------------
 * Fused EdgeConv: gather -> 2-layer edge MLP -> segmented max, one pass, no per-edge tensor in HBM.
 * Replaces EdgeConv / EdgeConvMotion .propagate()           models/basic_modules.py:151-155, 190-195
 *
 * For every sorted edge e = (j -> i) and replica r (keyframe), row(i) = r*rep_stride + i
 * (separate strides for the inputs and the output so a replica-invariant branch, e.g. the position
 * branch of EdgeConvMotion under the keyframe loop models/rignet.py:85-86, is gathered from ONE copy):
 *     h1 = s1 * relu(A[row(i)] + B[row(j)]) + t1                  (layer 1 split per vertex:
 *                                                                  W1 [x_i ; x_j - x_i] = (W1a-W1b) x_i + W1b x_j)
 *     z  = s2 * relu(W2 h1 + b2) + t2
 *     out[row(i)] = max over incoming edges of z
 * H = hidden = output width; supported H: 16, 32, 64, 128, 256.
 */
typedef struct morig_edgeconv_args {
    uint32_t struct_size;              /* sizeof(morig_edgeconv_args) of the caller's build (ABI 3) */
    int32_t H;
    int32_t n_nodes, replicas;
    int32_t in_rep_stride;             /* row offset of replica r in A/B: r*in_rep_stride (0 = shared by all replicas) */
    int32_t out_rep_stride;            /* row offset of replica r in out                                              */
    const float* A; int32_t lda;       /* per-vertex target term  (incl. layer-1 bias) */
    const float* B; int32_t ldb;       /* per-vertex source term                         */
    const int32_t* rowptr; const int32_t* src_sorted; const int32_t* dst_sorted;
    int32_t edge_capacity;             /* upper bound of E' used to size the launch      */
    int32_t edge_count;                /* exact E' if the host knows it (0 = unknown); only used for
                                          the algorithmic-FLOP accounting of morig_prof_collect      */
    const float* s1; const float* t1;  /* [Hpad] BatchNorm-1 eval affine                  */
    const float* W2; int32_t ldw;      /* packed [Hpad][ldw], ldw >= roundup(H,32)... see morig_gemm_args.W */
    const float* b2; const float* s2; const float* t2;   /* [Hpad]                        */
    float* out; int32_t ldo;           /* out[row][0..H)                                  */
    const void* W2_split; int32_t* overflow;   /* optional split-fp16 fast path (H >= 32), as in morig_gemm_args */
    int32_t quad_aligned;              /* the CSR was built with MORIG_CSR_PAD4: segments are 4-aligned */
    int32_t out_split;                 /* store `out` in the split-fp16 activation layout (morig_gemm_args.x_split: per 32-column chunk
                                          32 hi halves, then 32 lo halves) so that the unit's MLP (models/basic_modules.py:216-217,
                                          `self.mlp(torch.cat(...))`) reads it through the LDS-DMA GEMM without an fp32 -> fp16 pass.
                                          Needs W2_split + overflow, `out` 128-byte aligned, ldo % 32 == 0 and the launch on one of the
                                          4-aligned-CSR kernels (H = 128 / 256): ask morig_edgeconv_can_split_out first;
                                          MORIG_E_UNSUPPORTED otherwise. *overflow is raised when a result leaves the fp16 range. */
    int32_t exact_arith;               /* [ABI 3] arithmetic of the EXACT path (W2_split == NULL): 0 = v_mfma_f32_32x32x2_f32, 1 = the bf16 x 6
                                          split of MORIG_SPLIT_BF16X6 (H >= 32; morig_edgeconv, morig_edge_hidden) */
    int32_t seg_min4;                  /* [ABI 3] the CSR was built with MORIG_CSR_MIN4 (segments of >= 4 rows, NOT 4-aligned; quad_aligned = 0):
                                          H = 256 split-fp16 launches with out_split then take the mixed-quad form of the W2-stationary
                                          kernel (morig_edgeconv_can_split_out answers for it); everywhere else the flag is ignored -- a
                                          MIN4 CSR is a valid plain CSR for every other kernel (max over a repeated row is the same max). */
    /* [ABI 3, appended in round 6: callers built against the 192-byte struct leave these zero] the boundary passes of TWO launches in one
     * launch each. A launch whose target segments straddle tile boundaries is bracketed by two small passes over exactly those rows of
     * `out` (identity pattern in front of the kernel's atomics; with out_split the conversion of those rows behind it). The two EdgeConvs
     * of a unit -- template graph and geodesic graph, models/basic_modules.py:165-177, 205-219 -- write disjoint column blocks and do not
     * read each other's results, so their passes can share launches: call the FIRST launch with init_with = &second (its pass also
     * prepares the second's rows) and skip_split = 1, then the SECOND with skip_init = 1 and split_with = &first (its conversion pass
     * also converts the first's rows; both must be out_split launches for that half). Both structs must stay valid for both calls, the
     * calls go to the same stream in that order, and nothing may read `out` of the first before the second has been enqueued. */
    const struct morig_edgeconv_args* init_with;
    const struct morig_edgeconv_args* split_with;
    int32_t skip_init, skip_split;
} morig_edgeconv_args;
int morig_edgeconv(const morig_edgeconv_args* a, void* stream);
/* 1 when morig_edgeconv would honour out_split for these arguments (pointers, widths, CSR form and the library's environment
 * switches are looked at; out_split itself is ignored), 0 otherwise. Launches nothing. */
int morig_edgeconv_can_split_out(const morig_edgeconv_args* a);

/* The same EdgeConv for a vertex input of 3 channels (the position branches, models/basic_modules.py:193-195 `nn_pos([pos_i, pos_j - pos_i])`,
 * and motionNet's first unit, whose feature is the 3-channel keyframe flow, models/rignet.py:86): the first Linear is evaluated inside the
 * kernel from the two gathered endpoints -- z = relu(W1a x_i + W1b x_j + b1), W1a = W_a - W_b, W1b = W_b of the reference's
 * Linear(6 -> H) on [x_i, x_j - x_i] -- so no per-vertex [A | B] table is written or gathered (2 x 16 bytes per edge row instead of
 * 2 x 4 H). H == 32 (two 16-wide layers paired, or one 32-wide layer); BatchNorm-1 must be folded into W2 / b2 (packing.fold_hidden_affine).
 *   X [rows][ldx] (ldx >= 4, 16-byte aligned rows; columns 0..2 used), replica r reads rows r * in_rep_stride + vertex;
 *   W1a, W1b [32][4] (column 3 ignored), b1 [32]; everything else as morig_edgeconv_args. */
typedef struct morig_edgeconv_x3_args {
    uint32_t struct_size;              /* sizeof(morig_edgeconv_x3_args) of the caller's build (ABI 3) */
    int32_t H;
    int32_t n_nodes, replicas;
    int32_t in_rep_stride, out_rep_stride;
    const float* X; int32_t ldx;
    const float* W1a; const float* W1b; const float* b1;
    const int32_t* rowptr; const int32_t* src_sorted; const int32_t* dst_sorted;
    int32_t edge_capacity; int32_t edge_count;
    const float* W2; int32_t ldw;
    const float* b2; const float* s2; const float* t2;
    float* out; int32_t ldo;
    const void* W2_split; int32_t* overflow;
    /* [ABI 3, appended in round 6] as morig_edgeconv_args.init_with / skip_init: the first launch of a pair prepares the shared rows of
     * both, the second skips its pass (these launches never store split rows, so there is no conversion pass to share) */
    const struct morig_edgeconv_x3_args* init_with;
    int32_t skip_init, reserved0;
} morig_edgeconv_x3_args;
int morig_edgeconv_x3(const morig_edgeconv_x3_args* a, void* stream);

/* PointConv (3-layer local_nn, models/basic_modules.py:72,82-84; PyG PointConv.message) in two passes:
 *   morig_edge_hidden : Z[e] = s2*relu(W2 (s1*relu(A_i + B_j) + t1) + b2) + t2 for every sorted edge e (< E');
 *                       same arguments as morig_edgeconv, `out` = Z [edge_capacity][ldo], replicas = 1
 *   morig_segmax_gemm : out[i] = max_{e -> i} scale*act(W X[e] + bias) + shift   (layer 3 + aggr='max')
 * With x = None the message is the offset alone; with features it is [x_j ‖ pos_j - pos_i], whose first
 * Linear splits per vertex exactly like EdgeConv's: B_j = W1 [x_j ‖ pos_j] + b1, A_i = -W1p pos_i.        */
int morig_edge_hidden(const morig_edgeconv_args* a, void* stream);
typedef struct morig_segmax_args {
    uint32_t struct_size;                /* sizeof(morig_segmax_args) of the caller's build (ABI 3) */
    int32_t N, K;
    const float* X; int32_t ldx;         /* per-edge rows [edge_capacity][ldx]                       */
    const float* W; int32_t ldw;         /* packed like morig_gemm_args.W (rows padded to 32/64/128/256) */
    const float* bias; const float* scale; const float* shift; int32_t relu;
    const int32_t* rowptr; const int32_t* dst_sorted; int32_t n_nodes;
    int32_t edge_capacity; int32_t edge_count;
    float* out; int32_t ldo;             /* [n_nodes][ldo]                                          */
    const void* W_split; int32_t* overflow;
} morig_segmax_args;
int morig_segmax_gemm(const morig_segmax_args* a, void* stream);

/* The same PointConv in ONE launch pair, straight from the slot table of morig_ball_query (csrc/pointconv_fused.hip;
 * split-fp16 arithmetic only; (H, H3) in {(32, 64), (64, 128)}, max_nbrs == 64): per centre c the kept slots
 * (0 <= source < n_src, source != c) plus the self loop (c, c) -- the edge set morig_csr_from_slots builds, i.e.
 * PointConv's remove_self_loops / add_self_loops (basic_modules.py:82-84) -- without a CSR, per-edge rows in HBM or atomics.
 *   A [n_centres][lda] = -W1p pos_c, B [n_src][ldb] = W1 [x_j | pos_j] + b1 (as for morig_edge_hidden);
 *   W2_split [H][ldw2], b2 [H]: Linear2 with BN1 folded in (packing.fold_hidden_affine);
 *   W3_split [H3][ldw3], b3 [H3]: Linear3 with BN2 folded in the same way; s3 / t3: BN3 (NULL: identity); relu3.
 * *status is set to 1 when a slot names a source >= n_src (out is unspecified then); *overflow as in morig_gemm.
 * MORIG_E_UNSUPPORTED for other widths: the caller falls back to morig_edge_hidden + morig_segmax_gemm. */
typedef struct morig_pointconv_args {
    uint32_t struct_size;                /* sizeof(morig_pointconv_args) of the caller's build (ABI 3) */
    const float* A; int32_t lda;
    const float* B; int32_t ldb;
    const int64_t* slots; int32_t max_nbrs;
    int32_t n_centres, n_src;
    int32_t H, H3;
    const void* W2_split; int32_t ldw2; const float* b2;
    const void* W3_split; int32_t ldw3; const float* b3; const float* s3; const float* t3; int32_t relu3;
    float* out; int32_t ldo;
    int32_t* overflow; int32_t* status;
} morig_pointconv_args;
int morig_pointconv_fused(const morig_pointconv_args* a, void* stream);

/* --------------------------------------------------------------------------------------------
 * Small vertex-parallel operators.
 */
/* strided 2-D copy  dst[r*ldd + c] = src[r*lds + c]  (feature slicing input_flow[:, 3t:3t+3],
 * models/rignet.py:86; torch.cat column placement :65). No alignment requirement. */
int morig_copy2d(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t rows, int32_t cols, void* stream);
/* copy into a zero-padded slot: dst[r][c] = c < cols ? src[r][c] : 0 for c < slot_cols; with split != 0 the slot
 * (slot_cols % 32 == 0, 128-byte aligned) is written in the split-fp16 activation layout; *overflow as in morig_gemm. */
int morig_copy2d_pad(const float* src, int32_t lds, int32_t rows, int32_t cols, float* dst, int32_t ldd,
                     int32_t slot_cols, int32_t split, int32_t* overflow, void* stream);
/* `replicas` such copies in one launch: copy r reads the source window shifted by r * src_col_step columns and writes
 * the destination window shifted by r * dst_row_step rows. Keyframe features (input_flow[:, 3t:3t+3] -> replica t,
 * rignet.py:86): src_col_step = 3; position rows / position-branch columns of the motion replicas: src_col_step = 0. */
int morig_copy2d_pad_rep(const float* src, int32_t lds, int32_t rows, int32_t cols, int32_t src_col_step, float* dst,
                         int32_t ldd, int32_t slot_cols, int32_t replicas, int64_t dst_row_step, int32_t split,
                         int32_t* overflow, void* stream);
/* K tails (morig_gemm_args.X_tail) of up to MORIG_MAX_TAILS concatenations in ONE launch: tail t, row v =
 * [src[v][col_a[t] .. + wa) | src[v][col_b[t] .. + wb) | zeros up to 32] as one split-fp16 chunk at dst + t * tail_stride + v * 32 floats
 * (wa + wb <= 32; dst 128-byte aligned, tail_stride % 32 == 0). Builds [pos_tpl | pos_geo] (models/basic_modules.py:216-217) of every
 * GCUMotion unit of a forward from the buffer the paired position branches wrote (morig_edgeconv_x3). *overflow as in morig_gemm. */
#define MORIG_MAX_TAILS 8
int morig_pack_tails(const float* src, int32_t lds, int32_t rows, const int32_t* col_a /* host [n_tails] */,
                     const int32_t* col_b /* host [n_tails] */, int32_t wa, int32_t wb, int32_t n_tails, float* dst,
                     int64_t tail_stride, int32_t* overflow, void* stream);

/* gather columns: dst[r*ldd + c] = src[r*lds + cols[c]]  (skin_input column selection,
 * models/rignet.py:158-171). cols: int32 [n_cols] on device. */
int morig_gather_cols(const float* src, int32_t lds, const int32_t* cols, int32_t n_cols,
                      float* dst, int32_t ldd, int32_t rows, void* stream);

/* seg_out[r*n_nodes + v] = r*n_graphs + batch[v]  for r < replicas (int64 PyG batch vector in) */
int morig_make_seg(const int64_t* batch, int32_t n_nodes, int32_t n_graphs, int32_t replicas,
                   int32_t* seg_out, void* stream);

/* row-wise L2 normalisation  y = x / max(||x||_2, 1e-12)  (F.normalize, models/rignet.py:87,98;
 * models/corrnet.py:48,60) with a replica-to-token transposition on the way out:
 * input row m = r*rows_per_rep + v  ->  output address y + v*ld_row + r*ld_rep.               */
int morig_rownorm(const float* x, int32_t ldx, int32_t rows_per_rep, int32_t replicas, int32_t cols,
                  float* y, int32_t ld_row, int32_t ld_rep, void* stream);

/* CLS-token temporal attention, exact restructuring of TemporalAttn.forward up to (not incl.) w_o
 * (models/rignet.py:36-45): only token 0 of the output is consumed, so per vertex and head h
 *     score_t = <tok_t, g_h>,  g_h = W_k,h^T (W_q,h cls) / sqrt(d)      (tok_0 = cls, tok_1..T = frames)
 *     y_h     = sum_t softmax(score)_t * tok_t
 * x: [n][T][C] frames; g: [heads][C]; cls: [C]; y: [n][heads*C] (then one GEMM with W_o,h W_v,h). */
int morig_cls_attention(const float* x, int32_t n, int32_t T, int32_t C, int32_t heads,
                        const float* g, const float* cls, float* y, int32_t ldy, void* stream);

/* reductions over keyframes for aggr_method 'mean' / 'max' (models/rignet.py:92-95):
 * x: [n][T][C] -> y[n][C]; mode 0 = mean, 1 = max */
int morig_frame_reduce(const float* x, int32_t n, int32_t T, int32_t C, int32_t mode, float* y, int32_t ldy, void* stream);

/* --------------------------------------------------------------------------------------------
 * CorrNet point branch (models/corrnet.py:50-73, models/basic_modules.py:66-138). Clouds are contiguous
 * row ranges given by int32 offset arrays ptr[n_clouds + 1] (PyG's sorted `batch` vector).
 */
/* The plain AND the 4-aligned (MORIG_CSR_PAD4) CSR of one square graph from ONE pass over the COO: the count pass and the edge
 * ranks inside a segment are shared, both fills happen in one kernel (the rig networks need both per graph and per forward:
 * models/basic_modules.py:188-189 is normalised once instead of once per layer). Same results as two morig_csr_build_bipartite
 * calls up to the order of a target's edges inside its segment. ws: 2 * n_nodes + 1 ints of scratch. */
/* [ABI 3] flags: 0, or MORIG_CSR_MIN4 (the plain CSR's segments are filled up to 4 rows; src_sorted / dst_sorted then need the padded
 * CSR's capacity n_edges + 4 * n_nodes). */
int morig_csr_build_dual(const int64_t* edge_index, int64_t n_edges, int32_t n_nodes, int32_t* rowptr, int32_t* src_sorted,
                         int32_t* dst_sorted, int32_t* rowptr4, int32_t* src_sorted4, int32_t* dst_sorted4, int32_t* ws,
                         int32_t flags, int32_t* status, void* stream);
/* The same normalised CSR as morig_csr_build_bipartite(MORIG_CSR_SKIP_NEGATIVE) for the slot table morig_ball_query
 * writes (target k owns slots [k*max_nbrs, (k+1)*max_nbrs) of row 0 of `coo`, max_nbrs <= 64, unused = -1): counted
 * and filled per target without atomics (replaces torch_cluster.radius -> PointConv's remove/add_self_loops,
 * basic_modules.py:77-84). Capacity of src_sorted / dst_sorted: n_nodes * (max_nbrs + 1); cursor: n_nodes + 1 ints. */
int morig_csr_from_slots(const int64_t* coo, int32_t n_nodes, int32_t max_nbrs, int32_t n_src_nodes,
                         int32_t* rowptr, int32_t* src_sorted, int32_t* dst_sorted, int32_t* cursor, int32_t* status,
                         void* stream);
/* torch_cluster.fps (basic_modules.py:75): per cloud out_ptr[b+1]-out_ptr[b] samples, first = ptr[b] +
 * start[b] (start == NULL: first point), then repeatedly the point farthest from the chosen set
 * (lowest index on ties). idx_out: GLOBAL row indices, clouds concatenated. */
int morig_fps(const float* pos, int32_t ldp, const int32_t* ptr, const int32_t* out_ptr, const int32_t* start,
              int32_t n_clouds, int32_t max_cloud_points, int32_t* idx_out, void* stream);
/* torch_cluster.radius, CUDA-kernel semantics (basic_modules.py:77): for every centre y the first max_nbrs
 * points x of its cloud, in index order, with |x-y|^2 < r^2. coo: int64 [2][n_centres*max_nbrs]
 * (row 0 = x index, row 1 = centre index; unused slots -1), the layout morig_csr_build_bipartite reads. */
int morig_ball_query(const float* x, int32_t ldx, const int32_t* ptr_x, const float* y, int32_t ldy,
                     const int32_t* ptr_y, int32_t n_clouds, int32_t n_centres, float radius,
                     int32_t max_nbrs, int64_t* coo, void* stream);
/* radius_cpu (basic_modules.py:9-29), the ball query of the reference's no-CUDA branch: for every y ALL x with
 * |x-y| <= r (inclusive; no batch vector); a row with more than max_nbrs (<= 64) hits keeps a uniformly random
 * subset of exactly max_nbrs (the reference: torch.multinomial on the 0/1 row; here Algorithm-R reservoir sampling
 * with a counter-based hash of (seed, row, hit number): same distribution over subsets, a different random stream).
 * coo: the slot table of morig_ball_query; counts[ny]: hits per row before the cap. */
int morig_radius_sample(const float* x, int32_t ldx, int32_t nx, const float* y, int32_t ldy, int32_t ny, float radius,
                        int32_t max_nbrs, uint32_t seed, int64_t* coo, int32_t* counts, void* stream);
/* torch_geometric.nn.knn_interpolate (basic_modules.py:134), k <= 3: weights 1/clamp(d^2, 1e-16).
 * idx_ws/wgt_ws: scratch [n_targets][3]. */
int morig_knn_interpolate(const float* feat, int32_t ldf, int32_t C, const float* pos_x, int32_t ldx,
                          const int32_t* ptr_x, const float* pos_y, int32_t ldy, const int32_t* ptr_y,
                          int32_t n_clouds, int32_t n_targets, int32_t max_targets_per_cloud, int32_t k,
                          int32_t* idx_ws, float* wgt_ws, float* out, int32_t ldo, void* stream);
/* The two halves of morig_knn_interpolate, for callers that know the geometry before the features (the CorrNet point branch
 * runs the three searches on its geometry stream, under the convolutions): the k nearest sources of every target and their
 * weights -- slots past k, or past the cloud's point count, carry weight 0 -- then the weighted mean of feature rows. */
int morig_knn_search(const float* pos_x, int32_t ldx, const int32_t* ptr_x, const float* pos_y, int32_t ldy,
                     const int32_t* ptr_y, int32_t n_clouds, int32_t n_targets, int32_t max_targets_per_cloud, int32_t k,
                     int32_t* idx, float* wgt, void* stream);
int morig_knn_apply(const float* feat, int32_t ldf, int32_t C, const int32_t* idx, const float* wgt, int32_t n_targets,
                    float* out, int32_t ldo, void* stream);
/* knn(out_pts, out_vtx, 1, cosine=True) on L2-normalised rows (corrnet.py:64): arg-max dot product
 * within the cloud; C must be 64. */
int morig_cosine_nn(const float* v, int32_t ldv, const int32_t* ptr_v, const float* p, int32_t ldp,
                    const int32_t* ptr_p, int32_t n_clouds, int32_t max_rows_per_cloud, int32_t C,
                    int32_t* nn, float* sim, void* stream);
/* ---- DeformNet glue (/root/reference/models/deformnet.py) ----
 * pred_vismask = sigmoid(logit), then (m - min) / (max - min) per mesh (deformnet.py:42-46). ptr: [n_meshes + 1]
 * vertex offsets. A constant mask gives 0/0 = NaN, as the reference. */
int morig_sigmoid_minmax(const float* x, int32_t ldx, const int32_t* ptr, int32_t n_meshes, float* out, int32_t ldo,
                         void* stream);
/* knn(x, y, k, batch_x, batch_y, cosine=True) on L2-normalised rows (deformnet.py:49 and :92), 1 <= k <= 8, C must
 * be 64: idx[i][t] = global x row of the t-th most similar candidate of the same cloud (lowest index on ties), -1 where
 * there are fewer than k. split = 1 (x == y, ptr_x == ptr_y, vis required): rows with vis < 0.5 query the rows with
 * vis >= 0.5 -- the visible / invisible partition of :57-63 without the compaction; other rows get -1. */
int morig_cosine_knn(const float* y, int32_t ldy, const int32_t* ptr_y, const float* x, int32_t ldx,
                     const int32_t* ptr_x, int32_t n_clouds, int32_t max_rows_per_cloud, int32_t C, int32_t k,
                     const float* vis, int32_t ld_vis, int32_t split, int32_t* idx, void* stream);
/* scatter_add(v * w) / scatter_add(w) over the k neighbours of every vertex (deformnet.py:50-54 and :93-95); l1 rows
 * are [flow(3) | vis] = the feature of GCNDeform (:97).
 *   mode 0: every vertex i, w = <feat_s[j], feat_q[i]> * vis[i], v = pos_s[j] - pos_q[i]; also writes l1[i][3] = vis[i]
 *   mode 1: vertices with vis < 0.5, w = <feat_s[j], feat_q[i]>, v = l1[j][0:3] (the flow of visible vertex j). */
int morig_flow_vote(int32_t mode, const int32_t* idx, int32_t k, int32_t n, const float* feat_q, int32_t ldq,
                    const float* feat_s, int32_t lds, int32_t C, const float* pos_q, int32_t ldpq,
                    const float* pos_s, int32_t ldps, const float* vis, int32_t ld_vis, float* l1, int32_t ld_l1,
                    void* stream);
/* ---- joint extraction after the path (/root/reference/evaluate/eval_rigging.py:80-95). The reference
 * runs these steps in numpy float64, one mesh at a time; all point arrays here are float64 [n][3], contiguous. ----
 * inside_check (utils/mst_utils.py:15-29): keep[i] = 1 when round((p - translate) / scale * dims0) (half to even) lies
 * inside the 88^3 grid (hard-coded there) on a filled voxel. vox88: [88][88][88] bytes; translate: 3 HOST doubles. */
int morig_inside_check(const double* pts, int32_t n, const uint8_t* vox88, const double* translate, double scale,
                       double dims0, uint8_t* keep, void* stream);
/* sklearn.cluster.estimate_bandwidth (eval_rigging.py:89): *bandwidth (device) = mean over points of the distance to
 * the k-th nearest neighbour, the point itself included; the caller passes k = max(int(n * quantile), 1).
 * kth_ws: scratch [n] doubles. */
int morig_knn_bandwidth(const double* pts, int32_t n, int32_t k, double* kth_ws, double* bandwidth, void* stream);
/* meanshift_cluster (utils/cluster_utils.py:14-38): at most max_iter - 1 steps of p_j += 0.3 (weighted mean - p_j) with
 * kernel max(h^2 - d^2, 0) * weights[source] (weights may be NULL); the loop condition "total displacement > 1e-3" is
 * evaluated on the device (state: [max_iter] doubles, step t accumulates its squared displacement in state[t]), so the
 * call enqueues max_iter - 1 launches and never synchronises. bandwidth: device pointer to one double.
 * The result is in buf_a when *result_in_a (HOST int, written before return) is 1, else in buf_b. */
int morig_meanshift(const double* pts, const float* weights, int32_t n, const double* bandwidth, int32_t max_iter,
                    double* buf_a, double* buf_b, double* state, int32_t* result_in_a, void* stream);
/* nms_meanshift (utils/cluster_utils.py:41-66), two steps around the caller's np.argsort(counts)[::-1] (numpy's
 * unstable sort fixes the visiting order among equal counts, so it stays in numpy):
 * counts[j] = #{i : |p_i - p_j| <= bandwidth}; then the greedy pass over `order` writes alive[n]. */
int morig_nms_counts(const double* pts, int32_t n, const double* bandwidth, int32_t* counts, void* stream);
int morig_nms_greedy(const double* pts, const float* attn, int32_t n, const double* bandwidth, const int32_t* order,
                     double thrd_density, float thrd_attn, uint8_t* alive, void* stream);
/* The same four stages over the point sets of SEVERAL meshes at once (the reference loops over models, eval_rigging.py:62-98):
 * sets concatenated, mesh b = rows [ptr[b], ptr[b + 1]) (int32 [n_meshes + 1] on the device), n_all rows in total, max_n = the
 * largest set (sizes the launch grids). Per mesh the arithmetic and its order are those of the one-set entry points.
 *   bandwidth [n_meshes]; k of mesh b = max(int(n_b * quantile), 1) (sklearn estimate_bandwidth);
 *   state [n_meshes][max_iter]; order_local: the visiting order of every mesh as indices LOCAL to the mesh, concatenated. */
int morig_knn_bandwidth_batched(const double* pts, const int32_t* ptr, int32_t n_meshes, int32_t n_all, int32_t max_n,
                                double quantile, double* kth_ws, double* bandwidth, void* stream);
int morig_meanshift_batched(const double* pts, const float* weights, const int32_t* ptr, int32_t n_meshes, int32_t n_all,
                            int32_t max_n, const double* bandwidth, int32_t max_iter, double* buf_a, double* buf_b,
                            double* state, int32_t* result_in_a, void* stream);
int morig_nms_counts_batched(const double* pts, const int32_t* ptr, int32_t n_meshes, int32_t n_all, int32_t max_n,
                             const double* bandwidth, int32_t* counts, void* stream);
int morig_nms_greedy_batched(const double* pts, const float* attn, const int32_t* ptr, int32_t n_meshes, int32_t n_all,
                             const double* bandwidth, const int32_t* order_local, double thrd_density, float thrd_attn,
                             uint8_t* alive, void* stream);
/* Mean-shift over SPATIALLY SORTED point sets: the caller sorts every mesh's points by morig_morton_keys (key = mesh index above a
 * 30-bit Morton code of the position inside [-2, 2)^3), runs morig_meanshift_sorted on the permuted points / weights and scatters the
 * result back. Source tiles whose bounding box lies farther than the bandwidth from a target block's are skipped: the skipped pairs
 * have kernel value 0 exactly, so the result is the unsorted one up to the order of the additions. bbox_ws: 2 * n_meshes * ceil(max_n / 32) * 6
 * doubles (one box per 32 consecutive points, two generations). */
int morig_morton_keys(const double* pts, const int32_t* ptr, int32_t n_meshes, int32_t n_all, int64_t* keys, void* stream);
/* morig_nms_counts_batched over point sets in the same sorted order (e.g. the modes as morig_meanshift_sorted leaves them): boxes
 * of 32 consecutive points farther than the bandwidth from a target block's are skipped -- they hold no neighbour. Counts are
 * integers: identical to the unsorted kernel's. bbox_ws: n_meshes * ceil(max_n / 32) * 6 doubles. */
int morig_nms_counts_sorted(const double* pts, const int32_t* ptr, int32_t n_meshes, int32_t n_all, int32_t max_n,
                            const double* bandwidth, double* bbox_ws, int32_t* counts, void* stream);
int morig_meanshift_sorted(const double* pts, const float* weights, const int32_t* ptr, int32_t n_meshes, int32_t n_all,
                           int32_t max_n, const double* bandwidth, int32_t max_iter, double* buf_a, double* buf_b,
                           double* state, double* bbox_ws, int32_t* result_in_a, void* stream);
/* dst[r] = src[idx[r]] (pos[idx], out_pts[nn]); idx < 0 -> zeros */
int morig_gather_rows(const float* src, int32_t lds, const int32_t* idx, int32_t rows, int32_t cols,
                      float* dst, int32_t ldd, void* stream);

/* --------------------------------------------------------------------------------------------
 * Geodesic-ball graph on the device: data_proc/common_ops.py:214-226 get_geo_edges (radius = 0.06, max_nn = 15), the producer of
 * `geo_edge_index` (datasets/dataset_rig.py:86,122), batched over the meshes of a batch. For every vertex i: the members j != i
 * of its mesh with dist(i, j) <= radius (inclusive) in index order; a row with more than max_nn (<= 64) members keeps a uniformly
 * random subset of exactly max_nn (the reference: np.random.choice(members, max_nn, replace=False) on numpy's global stream;
 * here Algorithm-R reservoir sampling on a counter hash of (seed, row, member number): the same distribution over subsets).
 *   slots   [n_nodes][max_nn] int32, unused = -1        counts [n_nodes] = min(members, max_nn)
 *   members [n_nodes] uncapped member counts (may be NULL)
 *   offsets [n_nodes + 1] exclusive prefix sums of counts (offsets[n_nodes] = number of edges)
 *   scan_ws scratch, >= ceil(n_nodes / 2048) ints
 * morig_geo_ball_graph: Euclidean distance between positions (what SURVEY 8(d)'s synthetic recipe puts in the geodesic's place):
 *   LDS-tiled brute force, d^2 = (dx*dx + dy*dy) + dz*dz in fp32 (no fma) against fp32(radius)^2; meshes = contiguous row
 *   ranges mesh_ptr[n_meshes + 1].
 * morig_geo_ball_graph_dist: the reference's own input, a precomputed n x n float64 distance matrix of ONE mesh
 *   (calc_surface_geodesic, common_ops.py:162-211); the diagonal counts as dist + 10 (common_ops.py:218).
 * morig_geo_ball_fill: rows [i, member] in row order into an int64 COO [2][n_out] (row 0 = i, row 1 = member: the layout of
 *   np.loadtxt(geo_e).T, dataset_rig.py:86); self_loops != 0 appends the n_nodes pairs (i, i) that add_self_loops appends
 *   (dataset_rig.py:122): n_out = offsets[n_nodes] (+ n_nodes). */
int morig_geo_ball_graph(const float* pos, int32_t ldp, const int32_t* mesh_ptr, int32_t n_meshes, int32_t n_nodes,
                         float radius, int32_t max_nn, uint32_t seed, int32_t* slots, int32_t* counts, int32_t* members,
                         int32_t* offsets, int32_t* scan_ws, void* stream);
int morig_geo_ball_graph_dist(const double* dist, int64_t ldd, int32_t n_nodes, double radius, int32_t max_nn, uint32_t seed,
                              int32_t* slots, int32_t* counts, int32_t* members, int32_t* offsets, int32_t* scan_ws,
                              void* stream);
int morig_geo_ball_fill(const int32_t* slots, const int32_t* offsets, int32_t n_nodes, int32_t max_nn, int32_t self_loops,
                        int64_t* coo, int64_t n_out, void* stream);

/* ---- skinning on either side of SkinNet (csrc/skin.hip). The reference computes these offline in numpy / scipy
 * (data_proc/common_ops.py:275-328, data_proc/gen_skin_data.py:14-135) and in per-vertex loops of its eval code
 * (training/train_skin.py:40-66,232-244; evaluate/joint2rig.py:447-462). Meshes of a batch are contiguous row ranges.
 * morig_vol_geodesic: calc_volumetric_geodesic for every (mesh, bone) job. vox: [n_meshes][88^3] occupancy bytes; vox_tf:
 *   [n_meshes][5] doubles (translate x, y, z, scale, dims[0]); pos: float64 [n_vertices][3]; vtx_ptr / bone_ptr: [n_meshes + 1]
 *   prefix sums of the vertex and bone counts; bones: float64 [n_jobs][6] (parent xyz, child xyz), mesh-major; dist: int32,
 *   mesh b's [V_b][nb_b] block at dist_off[b]. n_slots: persistent workgroups (one per CU); workspace: device memory of
 *   morig_vol_geodesic_workspace(n_meshes, n_slots) bytes. status: 2 device ints, zeroed here; status[0] after the call: 0, 1 = a
 *   layer above 65535, 2 = a bone with more than 2^24 samples (dist is then incomplete).
 * morig_skin_bind: the k nearest bones per vertex by dist (stable: ascending bone id among equal distances), bind_ids [n][k]
 *   (-1 past the bone count), bind_invd = 1 / (D + 1e-10) fp64, and the dataset's tensors: skin_input float [n][8k], skin_nn,
 *   loss_mask, skin_nnjids int64 [n][k] (an invalid slot repeats slot 0 with mask 0). is_leaf / start_jid: per bone (start joint
 *   index within its rig). skins: float64 [n][ld_skins] per-vertex joint weights (at most 64 joints) or NULL; labels [n][k] with it.
 * morig_skin_scatter: mode 0 softmax(logits) * loss_mask, mode 1 softmax(logits * loss_mask) (float32), the mask-1 slots into
 *   P [n][ldp] fp64 (zeroed here) at skin_nn; columns >= n_bones[batch[v]] are left 0.
 * morig_skin_filter: W [n][ldw] fp64 = mean of P over the CSR row (rowptr [n + 1] / cols: unique 1-ring neighbours, self excluded;
 *   an empty row keeps the vertex's own row), entries < ratio * row max set to 0, divided by row sum + 1e-10. */
int64_t morig_vol_geodesic_workspace(int32_t n_meshes, int32_t n_slots);
int morig_vol_geodesic(const uint8_t* vox, int32_t n_meshes, const double* vox_tf, const double* pos, const int32_t* vtx_ptr,
                       const double* bones, const int32_t* bone_ptr, int32_t n_jobs, const int64_t* dist_off, int32_t n_slots,
                       void* workspace, int64_t workspace_bytes, int32_t* status, int32_t* dist, void* stream);
int morig_skin_bind(const int32_t* dist, const int64_t* dist_off, const int32_t* vtx_ptr, const int32_t* bone_ptr, int32_t n_meshes,
                    int32_t n_vertices, const double* bones, const uint8_t* is_leaf, const int32_t* start_jid, const double* skins,
                    int32_t ld_skins, int32_t k, int32_t* bind_ids, double* bind_invd, double* labels, float* skin_input,
                    int64_t* skin_nn, int64_t* loss_mask, int64_t* skin_nnjids, void* stream);
int morig_skin_scatter(const float* logits, int32_t ldl, const int64_t* skin_nn, const int64_t* loss_mask, const int64_t* batch,
                       const int32_t* n_bones, int32_t n, int32_t k, int32_t mode, double* P, int32_t ldp, void* stream);
int morig_skin_filter(const double* P, int32_t ldp, const int32_t* rowptr, const int32_t* cols, const int64_t* batch,
                      const int32_t* n_bones, int32_t n, double ratio, double* W, int32_t ldw, void* stream);

/* ---- surface geodesics and vertex-to-bone distances (csrc/geodesic.hip): the inference-side skinning inputs the reference computes
 * on the CPU (data_proc/common_ops.py:175-211 calc_surface_geodesic; evaluate/joint2rig.py:41-94, 307-360, 413-442). Everything is
 * float64; meshes of a batch are contiguous ranges given by [n_meshes + 1] prefix sums.
 * morig_surface_geodesic: pts / normals [total_samples][3], s_ptr the samples' prefix sums (every mesh 6 .. 65535 samples, none above
 *   max_samples); out: mesh b's [S_b][S_b] matrix at out_off[b]. One job = nsrc consecutive sources of one mesh; job_ptr: prefix sums of
 *   ceil(S_b / nsrc); n_jobs = job_ptr[n_meshes]. use_lds = 1: the distance vectors live in LDS, nsrc in {1, 2, 4} with
 *   nsrc * max_samples <= 16384; use_lds = 0: in the workspace, nsrc = 4. n_slots: persistent workgroups. workspace: device memory of
 *   morig_surface_geodesic_workspace(...) bytes. status: 8 device ints, zeroed here; after the call status[0] = 0, 1 = a job passed
 *   S sweeps without settling, 2 = a mesh larger than max_samples (out is then incomplete); status[2] / status[3] = the largest /
 *   the summed sweep count of the jobs, status[4] = the directed adjacency entries of all meshes.
 * morig_nearest_point: out[i] = the index (within its mesh) of the first nearest of the mesh's pts to q[i]; squared = 0 compares
 *   sqrt of the squared distance (common_ops.py:206-207), 1 the squared distance (joint2rig.py:356-357).
 * morig_bone_point_distance: pts2line for every (vertex, bone) pair; pair (v, c) of mesh b is element off[b] + v * nb_b + c of
 *   origins [n_pairs][3] / dist [n_pairs]; bones [n_bones][6] mesh-major.
 * morig_bone_visibility: vis[pair] = 1 where no triangle of the mesh's occluder (tri_pos / tp_ptr, faces int32 [F][3] local indices /
 *   f_ptr) is hit nearer than the vertex by the ray from the bone's nearest point; blk_ptr: prefix sums of ceil(V_b * nb_b / 256).
 * morig_bone_geodesic: calc_geodesic_matrix given dist and vis: vis_after (the 15th-percentile rule applied), n_vis / pct per bone,
 *   out [n_pairs], nn [n_pairs] (the arg-min vertex of an invisible pair, else -1). sg: mesh b's [V_b][V_b] matrix at sg_off[b].
 * morig_skin_bind_geo: predict_skinning's bind loop on float64 distances: skin_input float [n][8k], skin_nn, loss_mask int64 [n][k]. */
int64_t morig_surface_geodesic_workspace(int64_t total_samples, int32_t n_meshes, int32_t max_samples, int32_t n_slots, int32_t use_lds);
int morig_surface_geodesic(const double* pts, const double* normals, const int32_t* s_ptr, const int32_t* job_ptr, int32_t n_meshes,
                           int64_t total_samples, int32_t max_samples, int32_t n_jobs, int32_t nsrc, int32_t use_lds,
                           const int64_t* out_off, int32_t n_slots, void* workspace, int64_t workspace_bytes, int32_t* status,
                           double* out, void* stream);
int morig_nearest_point(const double* q, const int32_t* q_ptr, const double* pts, const int32_t* p_ptr, int32_t n_meshes, int32_t n_q,
                        int32_t squared, int32_t* out, void* stream);
int morig_bone_point_distance(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, int32_t n_meshes,
                              const int64_t* off, int64_t n_pairs, double* origins, double* dist, void* stream);
int morig_bone_visibility(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, const double* tri_pos,
                          const int32_t* tp_ptr, const int32_t* faces, const int32_t* f_ptr, const int64_t* off, const int32_t* blk_ptr,
                          int32_t n_meshes, int32_t n_blocks, uint8_t* vis, void* stream);
int morig_bone_geodesic(const double* dist, const uint8_t* vis, const double* sg, const int64_t* sg_off, const int32_t* vtx_ptr,
                        const int32_t* bone_ptr, const int64_t* off, int32_t n_meshes, int32_t n_bones, int64_t n_pairs,
                        uint8_t* vis_after, int32_t* n_vis, double* pct, double* out, int32_t* nn, void* stream);
int morig_skin_bind_geo(const double* dist, const int64_t* off, const int32_t* vtx_ptr, const int32_t* bone_ptr, int32_t n_meshes,
                        int32_t n_vertices, const double* bones, const uint8_t* is_leaf, int32_t k, float* skin_input, int64_t* skin_nn,
                        int64_t* loss_mask, void* stream);

/* --------------------------------------------------------------------------------------------
 * The path's one collective (the reference has no distributed code, this is the build's own sharding): meshes are
 * sharded whole, one process per GPU, and the per-mesh output rows are all-gathered over RCCL / xGMI once per forward.
 * The product's Python layer issues it through torch.distributed (backend "nccl" IS RCCL on ROCm: morig_amd/dist.py); these
 * exports are the same collective for a host that owns its communicator: `comm` is an ncclComm_t created once per process
 * (morig_rccl_unique_id on rank 0, the 128 bytes handed to every rank by the host's own means, then morig_rccl_comm_init).
 * Equal row counts per rank: one morig_allgather_rows; ragged meshes: morig_allgather_counts first, then a padded gather.
 * Status MORIG_E_HIP + morig_rccl_last_error() = the ncclResult_t. */
#define MORIG_RCCL_UNIQUE_ID_BYTES 128
int morig_rccl_unique_id(void* id_out /* MORIG_RCCL_UNIQUE_ID_BYTES */);
int morig_rccl_comm_init(int32_t n_ranks, int32_t rank, const void* unique_id, void** comm_out);
int morig_rccl_comm_destroy(void* comm);
int morig_rccl_last_error(void);
/* recv [n_ranks * rows][cols] <- every rank's send [rows][cols], rank-major (ncclAllGather on `stream`) */
int morig_allgather_rows(void* comm, const float* send, float* recv, int64_t rows, int32_t cols, void* stream);
int morig_allgather_counts(void* comm, const int64_t* send_one, int64_t* recv_n_ranks, void* stream);

/* --------------------------------------------------------------------------------------------
 * Live per-kernel timing (HIP events on the launch stream) for bench.py's roofline object.
 */
#define MORIG_PROF_KINDS 96
int         morig_prof_enable(int on);                 /* returns previous state */
int         morig_prof_reset(void);
const char* morig_prof_name(int kind);                  /* NULL past the last kind */
/* the ONE kernel symbol every launch of this kind runs, as rocprofv3 --kernel-trace prints it (a prefix: template arguments
 * that do not matter are cut); NULL for kinds that cover several kernels (index / copy / point-cloud helpers) */
const char* morig_prof_symbol(int kind);
/* synchronises the recorded events; per kind: launches, total ms, algorithmic flops, algorithmic bytes */
int         morig_prof_collect(int kind, int64_t* launches, double* total_ms, double* flops, double* bytes);

/* Probe of the matrix pipes' POWER-CAPPED rate (bench.py `roofline.mfma_power_capped_tflops`; SURVEY 8(d) "verify on the box"): enqueues
 * `launches` persistent kernels in which every wave of the chip issues `iters` x 24 v_mfma_f32_32x32x16_f16 from registers
 * (mode 0: random fp16 operands, mode 1: zeros). scratch: >= 1 float of device memory; *flops (optional): dense f16 flops enqueued. */
int morig_ubench_mfma(int mode, int iters, int launches, float* scratch, double* flops, void* stream);

/* ---- train-mode forward support (forward half; training/train_rig.py:136-195) -------------------------------
 * In model.train() every BatchNorm1d normalises with the statistics of the current batch -- over vertices in the dense
 * MLPs, over EDGES inside the per-edge MLPs (models/basic_modules.py:31-36, 153-155, 192-195) -- so the layers run unfused:
 * contraction (morig_gemm / morig_edge_hidden) -> statistics -> affine. */
/* per-column mean and BIASED variance of x[rows][cols] (fp64 accumulation, fixed summation order). rows_dev != NULL: the row
 * count is read on the device (E' = rowptr[n]) and `rows` is only the capacity. workspace: >= ceil(rows/256)*2*cols doubles.
 * count (optional): receives the row count as a float. */
int morig_col_stats(const float* x, int32_t ldx, int32_t rows, const int32_t* rows_dev, int32_t cols, double* workspace,
                    int64_t workspace_doubles, float* mean, float* var, float* count, void* stream);
/* out[r][c] = scale[c] * x[r][c] + shift[c] (BatchNorm once its statistics are known); out == NULL: in place */
int morig_col_affine(float* x, int32_t ldx, int32_t rows, const int32_t* rows_dev, int32_t cols, const float* scale,
                     const float* shift, float* out, int32_t ldo, void* stream);
/* BatchNorm1d in training mode after the column statistics (torch.nn.functional.batch_norm; models/basic_modules.py:31-36): the batch
 * affine s = gamma / sqrt(var + eps), t = beta - mean * s, rstd = 1 / sqrt(var + eps) (may be NULL), and -- when running_mean /
 * running_var are given -- their update with momentum and the UNBIASED variance (count: [1] float on the device, the rows the
 * statistics were taken over), num_batches_tracked += 1 (may be NULL). gamma / beta NULL: 1 / 0. */
int morig_bn_finalize(const float* mean, const float* var, const float* count, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      float* s, float* t, float* rstd, int32_t n, void* stream);
/* Z[e] = relu(A[dst_e] + B[src_e]) for the E' = rowptr[n_nodes] edges of a CSR: the first edge ReLU
 * (models/basic_modules.py:193-195 after the per-vertex split of Linear1), materialised for its batch statistics. With mean != NULL
 * the same pass also takes them: mean / var / count exactly as morig_col_stats over the E' rows of Z would (fp64, fixed order;
 * workspace as there, sized on edge_capacity); mean == NULL: workspace / var / count are not used. */
int morig_edge_gather_relu(const float* A, int32_t lda, const float* B, int32_t ldb, const int32_t* rowptr, int32_t n_nodes,
                           const int32_t* src_sorted, const int32_t* dst_sorted, int32_t edge_capacity, int32_t H,
                           float* Z, int32_t ldz, double* workspace, int64_t workspace_doubles, float* mean, float* var, float* count,
                           void* stream);
/* out[v][c] = max over rows e in [rowptr[v], rowptr[v+1]) of scale[c] * Z[e][c] + shift[c] (scale == shift == NULL: plain max;
 * empty segment: 0 as torch_scatter): max aggregation behind the last BatchNorm of an edge MLP, and scatter_max over a mesh's
 * vertices (models/rignet.py:63) */
int morig_segmax_affine(const float* Z, int32_t ldz, const int32_t* rowptr, int32_t n_segments, int32_t H, const float* scale,
                        const float* shift, float* out, int32_t ldo, void* stream);

/* --------------------------------------------------------------------------------------------
 * Train-mode BACKWARD operators (backward half; csrc/train_bwd.hip): what torch.autograd computes for the two
 * starred blocks in model.train() -- Seq(Linear, ReLU, BatchNorm1d) over vertices (models/basic_modules.py:31-36) and the
 * per-edge MLP with BatchNorm statistics over edges and max aggregation (:153-155, :179-202). dX = dU W goes through morig_gemm.
 */
/* per column: sum_dz[c] = sum_r dz[r][c] (= dbeta) and sum_dzx[c] = sum_r dz[r][c] * (y[r][c] - mean[c]) * rstd[c] (= dgamma) of
 * a training-mode BatchNorm1d whose INPUT was y; y == NULL: the plain column sum only (= dbias of a Linear). fp64 accumulation,
 * fixed order. workspace: >= ceil(rows/256) * 2 * cols doubles; rows_dev as in morig_col_stats. */
int morig_bn_backward_stats(const float* dz, int32_t ldz, const float* y, int32_t ldy, int32_t rows, const int32_t* rows_dev,
                            int32_t cols, const float* mean, const float* rstd, double* workspace, int64_t workspace_doubles,
                            float* sum_dz, float* sum_dzx, void* stream);
/* du[r][c] = [y > 0] * gamma * rstd * (dz - sum_dz / n - xhat * sum_dzx / n): the BatchNorm and the ReLU in front of it
 * (y = ReLU output = BatchNorm input, n = rows). du may alias dz. sum_du (NULL or [cols]): the column sums of du (fp64 accumulation,
 * fixed order: the bias gradient of the Linear in front) from the same pass; workspace as morig_bn_backward_stats, needed only then. */
int morig_bn_relu_backward(const float* dz, int32_t ldz, const float* y, int32_t ldy, int32_t rows, const int32_t* rows_dev,
                           int32_t cols, const float* mean, const float* rstd, const float* gamma, const float* sum_dz,
                           const float* sum_dzx, float* du, int32_t ldu, double* workspace, int64_t workspace_doubles, float* sum_du,
                           void* stream);
/* morig_segmax_affine that also records which row won: arg[v][c] = row index (first on ties), -1 for an empty segment; zwin
 * (NULL or [n_segments][ldw]) receives Z[arg[v][c]][c], the winner's value in front of the affine (0 for an empty segment): the
 * backward statistics then need no gather. Few long segments (per-mesh pooling) and many short ones (edges) take different kernels. */
int morig_segmax_affine_arg(const float* Z, int32_t ldz, const int32_t* rowptr, int32_t n_segments, int32_t H, const float* scale,
                            const float* shift, float* out, int32_t ldo, int32_t* arg, int32_t ld_arg, float* zwin, int32_t ldw,
                            void* stream);
/* the two BatchNorm sums for the BatchNorm in FRONT of a max aggregation, from the per-segment gradient dout [n_segments][cols]
 * and the arg-max table (the per-row gradient is one-hot per (segment, column) and never materialised); the BatchNorm input of
 * the winning rows comes from zwin [n_segments][ldw] when given (coalesced), otherwise it is gathered from the rows Z */
int morig_segmax_bn_backward_stats(const float* dout, int32_t ldd, const int32_t* arg, int32_t ld_arg, const float* Z, int32_t ldz,
                                   const float* zwin, int32_t ldw, int32_t n_segments, int32_t cols, const float* mean,
                                   const float* rstd, double* workspace, int64_t workspace_doubles, float* sum_dz, float* sum_dzx,
                                   void* stream);
/* du[e][c] for every row e < rowptr[n_segments] (seg_of_row[e] = its segment): the BatchNorm (+ the ReLU in front of it when
 * relu != 0) applied to that one-hot gradient; n = rowptr[n_segments]. Rows rowptr[n_segments] <= e < row_capacity are set to 0.
 * sum_du (NULL or [cols]): the column sums of du over the live rows, fp64 accumulation in a fixed order (the bias gradient of the
 * Linear behind the BatchNorm, from the same pass); workspace: >= ceil(row_capacity / slab) * 2 * cols doubles as in
 * morig_bn_backward_stats, needed only with sum_du. */
int morig_segmax_bn_relu_backward(const float* dout, int32_t ldd, const int32_t* arg, int32_t ld_arg, const float* Z, int32_t ldz,
                                  const int32_t* rowptr, int32_t n_segments, const int32_t* seg_of_row, int32_t row_capacity,
                                  int32_t cols, const float* mean, const float* rstd, const float* gamma, const float* sum_dz,
                                  const float* sum_dzx, int32_t relu, float* du, int32_t ldu, double* workspace,
                                  int64_t workspace_doubles, float* sum_du, void* stream);
/* morig_bn_relu_backward and morig_edge_scatter_backward in one, deterministic: with d[e] = [Y > 0] gamma rstd (dG - sum_dz / n -
 * xhat sum_dzx / n) (n = rowptr[n_nodes]; mean == NULL: d = dG), dA[v] = sum of d over the CSR segment of v and dB[u] = sum of d
 * over the edges out of u, walked through the transposed graph: rowptr_t [n_src_nodes + 1], perm_t[k] = row e of the k-th edge in
 * (source, row) order. d is evaluated where it is summed and never stored; both sums run in a fixed order (no atomics).
 * ZA / ZB (NULL, or [n_nodes][ldza] / [n_src_nodes][ldzb] with src_sorted / dst_sorted): Y is not read, Y[e] = relu(ZA[dst e] + ZB[src e])
 * is rebuilt where it is needed (what morig_edge_gather_relu stored, same expression, same bits): one of the two rows is fixed for a
 * whole segment, the other comes out of the caches, and the edges x H buffer is not read from HBM again. */
int morig_edge_bn_scatter_backward(const float* dG, int32_t ldg, const float* Y, int32_t ldy, const int32_t* rowptr,
                                   const int32_t* rowptr_t, const int32_t* perm_t, int32_t n_nodes, int32_t n_src_nodes, int32_t H,
                                   const float* mean, const float* rstd, const float* gamma, const float* sum_dz, const float* sum_dzx,
                                   float* dA, int32_t lda, float* dB, int32_t ldb, const float* ZA, int32_t ldza, const float* ZB,
                                   int32_t ldzb, const int32_t* src_sorted, const int32_t* dst_sorted, void* stream);
/* backward of Z[e] = A[dst_e] + B[src_e]: dA[v] = sum of dG over the CSR segment of v (fixed order), dB[u] = sum of dG over the
 * edges with source u (float atomics: summation order, hence the last bits, vary run to run). dB ([n_src_nodes][ldb]) is zeroed here. */
int morig_edge_scatter_backward(const float* dG, int32_t ldg, const int32_t* rowptr, const int32_t* src_sorted, int32_t n_nodes,
                                int32_t n_src_nodes, int32_t H, float* dA, int32_t lda, float* dB, int32_t ldb, void* stream);
/* the sums morig_bn_backward_stats would take over dh = dU2 W2 and Z1 (the BatchNorm of the FIRST layer of an edge MLP), from
 * products that exist already: M = dU2^T Z1 [h_out][h_in] (morig_gemm_tn, what dW2 is made of), db2 = column sums of dU2 [h_out], W2
 * [h_out][h_in] (Linear2, out x in): sum_dz[c] = sum_k db2[k] W2[k][c], sum_dzx[c] = rstd[c] sum_k W2[k][c] (M[k][c] - db2[k] mean[c]);
 * fp64, no pass over the edge rows. */
int morig_edge_bn_sums_from_products(const float* M, int32_t ldm, const float* db2, const float* W2, int32_t ldw, const float* mean,
                                     const float* rstd, int32_t h_out, int32_t h_in, float* sum_dz, float* sum_dzx, void* stream);
/* out[N][K] = A^T B over the rows (A [rows][N], B [rows][K], fp32 MFMA): the weight gradient dW = dU^T X. The row range is split
 * over workgroups and the partial products are summed in a fixed order. workspace: morig_gemm_tn_workspace(rows, N, K) floats.
 * Arithmetic: bf16 x 3 split MFMAs by default (both operands split in the kernel: ~16 mantissa bits, float32 exponent range, 2x the
 * exact kernel's rate); the environment variable MORIG_TRAIN_BWD=f32 selects the exact-float32 MFMA kernel. N, K <= 32: plain
 * float32 FMAs (exact products) on a kernel without MFMA tiles, whatever the setting. */
int64_t morig_gemm_tn_workspace(int32_t rows, int32_t N, int32_t K);
int morig_gemm_tn(const float* A, int32_t lda, const float* B, int32_t ldb, int32_t rows, const int32_t* rows_dev, int32_t N, int32_t K,
                  float* workspace, int64_t workspace_floats, float* out, int32_t ldo, void* stream);
/* the same with every row of B centred on b_shift [K] first: C = A^T (B - 1 b_shift^T); b_shift = NULL: plain A^T B. For products that are
 * used as  M - colsum(A) (x) mean  afterwards (the BatchNorm sums of the first edge layer, morig_edge_bn_sums_from_products): with the rows
 * centred on that mean the split contraction itself carries no cancellation */
int morig_gemm_tn_shift(const float* A, int32_t lda, const float* B, int32_t ldb, const float* b_shift, int32_t rows, const int32_t* rows_dev,
                        int32_t N, int32_t K, float* workspace, int64_t workspace_floats, float* out, int32_t ldo, void* stream);

/* ---- skeleton connection (csrc/skeleton.hip): evaluate/joint2rig.py:197-264 (create_one_data's pair loop, predict_skeleton) with
 * utils/mst_utils.py:63-108 (minKey / primMST) and :269-291 (increase_cost_for_outside_bone). Meshes of a batch are contiguous joint
 * ranges: joint_ptr [n_meshes + 1] prefix sums of the joint counts J_b, pair_ptr [n_meshes + 1] prefix sums of J_b (J_b - 1) / 2; the
 * pairs of a mesh are in itertools.combinations order. vox / vox_tf as morig_vol_geodesic (88^3 occupancy bytes; translate, scale, dims[0]).
 * morig_pair_attr: joints64 [n_joints][3] are the float64 joints create_one_data receives, joints32 their float32 cast (Data.joints, what
 *   the cost loop reads). pairs int64 [n_pairs][2]: joint rows within the batch (joint_ptr[b] + i, joint_ptr[b] + j), i < j.
 *   pair_attr float [n_pairs][3]: distance, inside samples / (samples + 1e-10) of sample_on_bone(step 0.01) on joints64 (float64, then
 *   cast), 1. outside_count int32 [n_pairs]: samples outside the mask on joints32, length / step count / unit step in float32 as NumPy 2
 *   leaves them, sample positions float64. status: 1 device int, zeroed here; 1 = a bone with more than 2^24 samples.
 * morig_skeleton_cost: mesh b's symmetric [J_b][J_b] float64 matrix at cost_off[b]: -log(double(sigmoid_f32(logit)) + 1e-10); 2 * count
 *   where outside_count > 1; halved where |x| < 2e-2 (float32) at both joints; diagonal -log(1e-10). sigmoid_f32 = the float32 nearest to
 *   the float64 sigmoid. pair_logits [n_pairs] / root_logits [n_joints] with element strides ld_pair / ld_root. root [n_meshes]: arg-max of
 *   sigmoid_f32(root_logits) over the mesh's joints, first index on ties. max_joints: an upper bound of J_b (sizes the grid).
 * morig_prim_mst: primMST from root[b]: keys start at infinity, the root's at 0; the first index among equal smallest keys is taken;
 *   an edge exists where cost > 0; a key is replaced by a strictly smaller cost only. parent int32 [n_joints] (within the mesh, -1 at the
 *   root), key float64 [n_joints]. status int32 [n_meshes]: 0, 1 = disconnected graph (parent all -1; the reference raises), 2 = root
 *   outside [0, J_b), 3 = J_b above MORIG_PRIM_MAX_JOINTS. max_joints above that limit: MORIG_E_UNSUPPORTED. */
#define MORIG_PRIM_MAX_JOINTS 1024
int morig_pair_attr(const double* joints64, const float* joints32, const int32_t* joint_ptr, const int32_t* pair_ptr, int32_t n_meshes,
                    int32_t n_pairs, const uint8_t* vox, const double* vox_tf, int64_t* pairs, float* pair_attr, int32_t* outside_count,
                    int32_t* status, void* stream);
int morig_skeleton_cost(const float* pair_logits, int32_t ld_pair, const float* root_logits, int32_t ld_root, const float* joints32,
                        const int32_t* outside_count, const int32_t* joint_ptr, const int32_t* pair_ptr, const int64_t* cost_off,
                        int32_t n_meshes, int32_t max_joints, double* cost, int32_t* root, void* stream);
int morig_prim_mst(const double* cost, const int64_t* cost_off, const int32_t* joint_ptr, const int32_t* root, int32_t n_meshes,
                   int32_t max_joints, int32_t* parent, double* key, int32_t* status, void* stream);

/* ---- rig tracking (csrc/track.hip): evaluate/eval_tracking.py:56-154 (ik_drag) on utils/deform_ik.py (Deform_IK.run).
 * morig_ik_solve: a batch of inverse-kinematics problems in ONE launch, one workgroup per problem, every Adam iteration inside the kernel
 *   (workgroup barriers only). Problem b owns the joints joint_ptr[b] .. joint_ptr[b + 1] and the vertices vert_ptr[b] .. vert_ptr[b + 1] of
 *   the concatenated arrays; joint and vertex indices inside a problem are local to it.
 *   locals_in [n_joints][9], offsets [n_joints][3], parent [n_joints] (-1 at the root), root [n_problems].
 *   order [n_joints]: the problem's joints breadth first from its root; level_ptr: per problem the offsets of the tree levels in order
 *   (level_off [n_problems + 1] prefix sums of levels + 1 into level_ptr); child_lo / child_hi [n_joints]: a joint's children as a range of
 *   order. Skin: only non-zero weights, twice: vertex-major (vptr [n_vertices + 1] entry offsets, vent_j the joint, vent_xw = x y z w: the
 *   vertex in that joint's frame and the weight, 16-byte aligned) and joint-major (jptr [n_joints + 1], jent_v the vertex, jent_xw).
 *   constraints [n_vertices][3], vismask [n_vertices]; mask = vismask > thrd[b] ? 1 : w_invis[b]. iter_time, lr (float64; the angles step with
 *   lr * pi), bias1 / bias2_sqrt [max_iter] float64: 1 - 0.9^t and sqrt(1 - 0.999^t) for t = 1 .. max_iter (Adam's bias corrections, computed
 *   by the caller as torch computes them). Angles and translation start at 0.01.
 *   Results: angles [n_joints][3] and trans [n_problems][3] after the last step; locals / globals [n_joints][9] and jpos [n_joints][3] of the
 *   LAST iteration's forward (the parameters before the last step, as the reference returns them). Optional (NULL to skip): loss
 *   [n_problems], grad_angles, grad_trans of the last iteration (without the weight decay). status [n_problems]: 0, 1 = sizes outside
 *   max_joints / max_vertices / max_iter or an empty problem, 2 = an index out of range (nothing of that problem is written).
 *   max_joints / max_vertices size the workgroup's LDS (morig_ik_solve_lds_bytes); a launch that does not fit: MORIG_E_UNSUPPORTED. No
 *   floating-point atomics: two runs are bit-identical.
 * morig_corr_select: nn / sim [n_vtx] (morig_cosine_nn's row arg-max and maximum; nn are rows of the point array) -> per point the vertex with the
 *   largest similarity among those that chose it, the first vertex on ties, similarity > 0; winner -1 / winner_sim 0 where none.
 *   keys: n_pts 64-bit words of workspace. */
#define MORIG_IK_SOLVE_STRUCT_BYTES 304u
typedef struct morig_ik_args {
    uint32_t struct_size;                /* sizeof(morig_ik_args) of the caller's build (ABI 3) */
    int32_t n_problems, max_joints, max_vertices, max_iter, reserved0;
    int64_t n_entries;
    const int32_t* joint_ptr; const int32_t* vert_ptr; const int32_t* level_off;
    const float* locals_in; const float* offsets;
    const int32_t* parent; const int32_t* order; const int32_t* level_ptr; const int32_t* child_lo; const int32_t* child_hi;
    const int32_t* vptr; const int32_t* vent_j; const float* vent_xw;
    const int32_t* jptr; const int32_t* jent_v; const float* jent_xw;
    const float* constraints; const float* vismask;
    const int32_t* root; const int32_t* iter_time; const double* lr; const float* w_invis; const float* thrd;
    const double* bias1; const double* bias2_sqrt;
    float* angles; float* trans; float* locals; float* globals; float* jpos;
    float* loss; float* grad_angles; float* grad_trans;
    int32_t* status;
} morig_ik_args;
int64_t morig_ik_solve_lds_bytes(int32_t max_joints, int32_t max_vertices);
int morig_ik_solve(const morig_ik_args* a, void* stream);
int morig_corr_select(const int32_t* nn, const float* sim, int32_t n_vtx, int32_t n_pts, uint64_t* keys, int32_t* winner, float* winner_sim,
                      void* stream);

/* ---- training losses (csrc/losses.hip): models/customized_losses.py infoNCE (:107-134), multi_pos_infoNCE (:137-158) and
 * chamfer_distance_with_average (:231-251), batched over the pairs / meshes of a batch, forward and backward. No floating-point atomics:
 * two runs on the same inputs are bit-identical. Nothing is read back: what a kernel finds wrong with its inputs it ORs into status (one
 * device int, zeroed by the caller), clamps the index so that no access leaves its array, and the loss comes out NaN.
 * morig_loss_segment_ptr: ptr [n_segments + 1] = row offsets of the segments of a sorted int64 batch vector (ptr must be zero-filled).
 * morig_infonce_forward / _backward: pair b owns rows ptr_vtx[b] .. ptr_vtx[b + 1] of vtx, ptr_pts of pts, ptr_v2p / ptr_p2v of the
 *   correspondence rows; corr_* int64 [rows][2] = (anchor, label), local to the pair: v2p anchors are vertices and labels points, p2v the
 *   other way round. Per pair and direction the mean over rows of the cross-entropy of anchor . keys^T / tau against the label; a pair
 *   without v2p rows contributes nothing (its p2v rows neither); the sum is divided by n_pairs. C must be 64 (MORIG_E_UNSUPPORTED otherwise).
 *   The logits run on the exact float32 MFMA and are never written to memory. forward writes lse [n_v2p + n_p2v] (v2p rows first), the
 *   workspace row_loss (same size) and loss [1]. backward recomputes the tiles from lse: upstream [1] is the gradient of the loss;
 *   workspaces d_rows [n_v2p + n_p2v][64], d_key_pts [n_pts][64], d_key_vtx [n_vtx][64] (all 16-byte aligned); rowptr_vtx [n_vtx + 1] /
 *   order_v2p [n_v2p] = the v2p rows grouped by their GLOBAL anchor vertex in row order (a stable sort), rowptr_pts / order_p2v the same
 *   for the p2v rows; grad_vtx [n_vtx][ld_gv], grad_pts [n_pts][ld_gp] = anchor-side sum in that order, then the key-side sum. An
 *   array of no entries (corr_* / order_* of a direction without rows, a feature matrix and its gradient without rows) may be NULL.
 * morig_multipos_forward / _backward: F [n_meshes * n_sample][ldf] the sampled feature rows (D a multiple of 4, at most 128), pos_ids
 *   [rows][n_pos <= 64] / neg_ids [rows][n_neg <= 256] indices into the mesh's samples. row_loss = (1 / n_pos) sum_j [log(exp(p_j) +
 *   sum_negs exp(n)) - p_j], loss = sum of rows / rows; neg_max / neg_sum [rows] are kept for the backward. backward: G [n_meshes]
 *   [n_sample][n_sample] workspace (a row's coefficients, duplicates added in slot order), grad[rows[i]] = sum_k (G[i][k] + G[k][i]) F[k];
 *   rows int32 [n_meshes * n_sample] without duplicates; rows of grad that are not sampled are not written.
 * morig_chamfer_forward / _backward: p [n_p][3], q [n_q][3], mesh b owns ptr_p[b] .. ptr_p[b + 1] and ptr_q[b] .. ptr_q[b + 1] (at most
 *   MORIG_CHAMFER_MAX_JOINTS rows of q per mesh: status bit MORIG_LOSS_ST_SIZE). loss = mean over meshes of 0.5 (mean_i min_j |p_i - q_j| +
 *   mean_j min_i |p_i - q_j|). arg1 / d1 [n_p]: nearest q row (local, smallest index on ties) and its distance; key2 [n_q]: distance bits
 *   << 32 | nearest p row. A zero distance has a zero gradient. */
#define MORIG_LOSS_ST_INDEX 1            /* an index outside its pair / mesh */
#define MORIG_LOSS_ST_UNSORTED 2         /* a batch vector that is not sorted */
#define MORIG_LOSS_ST_SEGMENT 4          /* a batch value outside [0, n_segments) */
#define MORIG_LOSS_ST_SIZE 8             /* a mesh with more than MORIG_CHAMFER_MAX_JOINTS joints */
#define MORIG_CHAMFER_MAX_JOINTS 1024
#define MORIG_NCE_STRUCT_BYTES 224u
typedef struct morig_nce_args {
    uint32_t struct_size;                /* sizeof(morig_nce_args) of the caller's build (ABI 3) */
    int32_t n_pairs, C; float tau;
    int32_t n_vtx, n_pts, n_v2p, n_p2v, ld_vtx, ld_pts, ld_gv, ld_gp;
    const float* vtx; const float* pts;
    const int64_t* corr_v2p; const int64_t* corr_p2v;
    const int32_t* ptr_vtx; const int32_t* ptr_pts; const int32_t* ptr_v2p; const int32_t* ptr_p2v;
    float* lse; float* row_loss; float* loss;
    const float* upstream;
    float* d_rows; float* d_key_pts; float* d_key_vtx;
    const int32_t* rowptr_vtx; const int32_t* order_v2p; const int32_t* rowptr_pts; const int32_t* order_p2v;
    float* grad_vtx; float* grad_pts;
    int32_t* status;
} morig_nce_args;
int morig_loss_segment_ptr(const int64_t* batch, int32_t n, int32_t n_segments, int32_t* ptr, int32_t* status, void* stream);
int morig_infonce_forward(const morig_nce_args* a, void* stream);
int morig_infonce_backward(const morig_nce_args* a, void* stream);
int morig_multipos_forward(const float* F, int32_t ldf, int32_t D, const int32_t* pos_ids, int32_t n_pos, const int32_t* neg_ids,
                           int32_t n_neg, int32_t n_meshes, int32_t n_sample, float* neg_max, float* neg_sum, float* row_loss,
                           float* loss, int32_t* status, void* stream);
int morig_multipos_backward(const float* F, int32_t ldf, int32_t D, const int32_t* pos_ids, int32_t n_pos, const int32_t* neg_ids,
                            int32_t n_neg, int32_t n_meshes, int32_t n_sample, const float* neg_max, const float* neg_sum,
                            const float* upstream, float* G, const int32_t* rows, float* grad, int32_t ld_grad, int32_t* status,
                            void* stream);
int morig_chamfer_forward(const float* p, const float* q, const int32_t* ptr_p, const int32_t* ptr_q, int32_t n_meshes, int32_t n_p,
                          int32_t n_q, int32_t* arg1, float* d1, uint64_t* key2, float* loss, int32_t* status, void* stream);
int morig_chamfer_backward(const float* p, const float* q, const int32_t* ptr_p, const int32_t* ptr_q, int32_t n_meshes, int32_t n_p,
                           int32_t n_q, const int32_t* arg1, const float* d1, const uint64_t* key2, const float* upstream, float* grad_p,
                           float* grad_q, const int32_t* status, void* stream);

/* ---- the losses of training/train_skin.py (csrc/losses_skin.hip): log_ratio_loss (models/customized_losses.py:11-44), the masked
 * soft-label cross-entropy of train_skin.py:168-174 and cross_entropy_with_probs (:216-228). Same rules as above: no floating-point atomics,
 * nothing read back, wrong data through the status word.
 * morig_logratio_forward / _backward: one workgroup per (mesh, feature set). Set t < n_all is the matrix feat_all + t * set_stride with row
 *   stride ld_all (the views motion_all[:, t, :] of an [n_rows][n_all][D] tensor: set_stride = D, ld_all = n_all * D); set n_all, present
 *   when n_sets == n_all + 1, is feat_aggr. D and W (the width of gt) are multiples of 4 up to MORIG_LOGRATIO_MAX_WIDTH, n_sample lies in
 *   [3, MORIG_LOGRATIO_MAX_SAMPLE] (MORIG_E_UNSUPPORTED otherwise). ptr [n_meshes + 1] from morig_loss_segment_ptr; samples int32 [n_sets]
 *   [n_meshes][n_sample] row ids local to the mesh, distinct inside a mesh (an id outside its mesh or a repeated one: MORIG_LOSS_ST_INDEX,
 *   clamped, loss NaN). With L[i][j] = log(|f_i - f_j|^2 + 1e-6) - log(|g_i - g_j|^2 + 1e-6) on the sampled rows (squared distances in
 *   difference form, float32, channels in order) and the pairs p = (a_p, b_p), a < b, in lexicographic order, a mesh's term is the mean over
 *   p < q of (L[a_q][b_p] - L[a_p][b_q])^2; loss [1] = sum over the sets, in set order, of (sum over meshes / n_meshes), float64 down to
 *   the last rounding; a mesh without vertices adds nothing. Workspaces: tab float [n_sets][n_meshes][2][n_sample][n_sample] (L and the
 *   feature distances, kept for the backward), wg_loss double [n_sets][n_meshes]. backward: upstream [1]; the sampled rows of grad_all
 *   (row stride ldg_all, set stride gset_stride) and grad_aggr are written, the other rows are not touched (zero-fill them); gt gets none.
 * morig_skin_ce_forward / _backward: x [n][ldx], label [n][ld_label], mask [n][ld_mask] (0 / 1 as float), the first K <= MORIG_SKIN_CE_MAX_K
 *   columns of each. g = label * mask, q = g / (sum |g| + 1e-8), vert_mask = |sum q - 1| < 1e-8 with both sums in index order in plain
 *   float32 (an exact-equality test on a rounded sum: the order is part of the contract); loss = sum (-q log_softmax(x) mask vert_mask) /
 *   sum (mask vert_mask), 0 / 0 = NaN. part double [2 ceil(n / 256)] workspace, sums double [2] = numerator, denominator (kept for the
 *   backward), grad [n][K] contiguous.
 * morig_ce_probs_forward / _backward: x, target, weight (NULL: none) [n][K] contiguous, K <= MORIG_CE_PROBS_MAX_K; reduction 0 none (cum
 *   [n][K] = -target log_softmax(x) weight, upstream [n][K]), 1 mean (sum / n), 2 sum (loss [1], upstream [1]; part double
 *   [2 ceil(n / 256)], sums double [2] workspaces). */
#define MORIG_LOGRATIO_MAX_SAMPLE 64
#define MORIG_LOGRATIO_MAX_WIDTH 128
#define MORIG_SKIN_CE_MAX_K 8
#define MORIG_CE_PROBS_MAX_K 128
#define MORIG_LOGRATIO_STRUCT_BYTES 184u
typedef struct morig_logratio_args {
    uint32_t struct_size;                /* sizeof(morig_logratio_args) of the caller's build (ABI 3) */
    int32_t n_meshes, n_rows, n_sets, n_all, n_sample, D, W;
    int64_t ld_all, set_stride, ld_aggr, ld_gt, ldg_all, gset_stride, ldg_aggr;
    const float* feat_all; const float* feat_aggr; const float* gt;
    const int32_t* ptr; const int32_t* samples;
    float* tab; double* wg_loss; float* loss;
    const float* upstream;
    float* grad_all; float* grad_aggr;
    int32_t* status;
} morig_logratio_args;
int morig_logratio_forward(const morig_logratio_args* a, void* stream);
int morig_logratio_backward(const morig_logratio_args* a, void* stream);
int morig_skin_ce_forward(const float* x, int32_t ldx, const float* label, int32_t ld_label, const float* mask, int32_t ld_mask, int32_t n,
                          int32_t K, float* vert_mask, double* part, double* sums, float* loss, void* stream);
int morig_skin_ce_backward(const float* x, int32_t ldx, const float* label, int32_t ld_label, const float* mask, int32_t ld_mask, int32_t n,
                           int32_t K, const double* sums, const float* upstream, float* grad, void* stream);
int morig_ce_probs_forward(const float* x, const float* target, const float* weight, int32_t n, int32_t K, int32_t reduction, float* cum,
                           double* part, double* sums, float* loss, void* stream);
int morig_ce_probs_backward(const float* x, const float* target, const float* weight, int32_t n, int32_t K, int32_t reduction,
                            const float* upstream, float* grad, void* stream);

/* ---- rig evaluation metrics (csrc/metrics.hip; morig_amd/metrics.py): what evaluate/eval_rigging.py:107-131 and utils/eval_utils.py:72-119
 * report. Everything is float64 with products and sums rounded separately, ragged over the meshes of a batch through int32 ptr arrays
 * [n_meshes + 1] that ascend inside [0, rows] (rows no segment names belong to no mesh); no floating-point atomics; nothing is read
 * back. The entry points take plain parameters (no argument struct). A ptr that does not ascend or leaves its array makes the kernels
 * skip the rows concerned; nothing is read out of bounds.
 * morig_bone_sample_counts: bones int32 [n_bones][2] = (parent, child) rows of joints [n_joints][3]; counts[b] = rint(len / 0.005) + 1 with
 *   len = sqrt((dx^2 + dy^2) + dz^2) (utils/eval_utils.py:72-80; rint rounds half to even as np.round does); a bone whose joints lie
 *   outside [0, n_joints) or whose count exceeds MORIG_BONE_MAX_SAMPLES gets 0, and so does one with a NaN joint. A zero-length bone is
 *   1 sample, so 0 always means a refused bone: metrics.sample_skel raises on one instead of sampling the skeleton without it.
 * morig_bone_samples: off int64 [n_bones + 1] = exclusive prefix sum of counts; out [n_samples][3], sample k of a bone is
 *   p + (ray / (n + 1e-30)) * k, a multiply and then an add.
 * morig_nearest_distance: out[i] = min over the rows of b in the mesh of a's row i of sqrt((dx^2 + dy^2) + dz^2) (squared != 0: without the
 *   square root); b goes through LDS in tiles of MORIG_NEAREST_TILE rows. A mesh that has rows in a and none in b sets flags[mesh] = 1
 *   (zero flags first) and its out rows are NaN. NaN follows np.min: a row of a with a NaN coordinate gives NaN, and a NaN row of b makes
 *   every row of a in that mesh NaN (any candidate whose squared distance is NaN does), with and without the square root.
 * morig_segment_mean: out[m] = (sum of x[ptr[m] .. ptr[m + 1]) in a fixed order inside one workgroup) / count; 0 rows give NaN.
 * morig_assign_joints: the optimal one-to-one assignment on dist[g][p] = |pred_p - gt_g| per mesh by shortest augmenting paths with dual
 *   potentials, one wave per mesh, the problem transposed when ground-truth rows outnumber predictions. match_ptr [n_meshes + 1] ascends by
 *   min(n_gt, n_pred); row_ind (ascending inside a mesh) / col_ind are local to the mesh, dist is the matched distance. cost double
 *   [cost_off[n_meshes]] is the workspace of the cost matrices (cost_off int64 [n_meshes + 1]; a mesh needs n_gt * n_pred). A mesh whose
 *   smaller side exceeds MORIG_ASSIGN_MAX_SMALL or whose larger side exceeds MORIG_ASSIGN_MAX_LARGE (or whose workspace is too small) is
 *   refused: status[mesh] = MORIG_ASSIGN_ST_SIZE, its pairs are -1 / NaN; the other meshes are solved. status [n_meshes] is written whole.
 *   Non-finite joints (this product's rule; scipy raises on them): a column of the solver's matrix whose cost is NaN or infinite is never
 *   chosen. When the remaining columns suffice status is 0 and the matching is the optimum of the matrix without that column; when they do
 *   not, status[mesh] = MORIG_ASSIGN_ST_INFEASIBLE, the mesh's pairs are -1 / NaN (so morig_joint_scores counts 0 hits for it) and the other
 *   meshes are untouched. ptr arrays that do not describe a mesh (a pred_ptr / gt_ptr / match_ptr segment that descends, is negative, leaves
 *   its array, or a match segment that is not min(n_gt, n_pred) long) give MORIG_ASSIGN_ST_PTR and NOTHING of that mesh is written.
 * morig_joint_scores: hits[m] = #(dist < fs[fs_ptr[m] + row_ind]) (strict; pairs with row_ind < 0 or past the mesh's feature sizes count
 *   nothing), out double [3][n_meshes] = IoU 2 hits / (n_pred + n_gt), precision hits / n_pred, recall hits / n_gt.
 * morig_valid_mean: x double [n_rows][n]; out[r] = (sum of x[r][i] over valid[i] != 0, in index order, by one thread) / #valid. */
#define MORIG_BONE_MAX_SAMPLES 16777216
#define MORIG_NEAREST_TILE 1024
#define MORIG_ASSIGN_MAX_SMALL 128
#define MORIG_ASSIGN_MAX_LARGE 256
#define MORIG_ASSIGN_ST_SIZE 1             /* a mesh beyond the supported size (or a workspace too small for it) */
#define MORIG_ASSIGN_ST_PTR 2              /* ptr arrays that do not describe the mesh: nothing of it is written */
#define MORIG_ASSIGN_ST_INFEASIBLE 4       /* a NaN or infinite distance: no assignment of finite cost */
int morig_bone_sample_counts(const double* joints, int32_t n_joints, const int32_t* bones, int32_t n_bones, int64_t* counts, void* stream);
int morig_bone_samples(const double* joints, int32_t n_joints, const int32_t* bones, const int64_t* off, int32_t n_bones, int64_t n_samples,
                       double* out, void* stream);
int morig_nearest_distance(const double* a, const int32_t* a_ptr, int32_t n_a, const double* b, const int32_t* b_ptr, int32_t n_b,
                           int32_t n_meshes, int32_t squared, double* out, int32_t* flags, void* stream);
int morig_segment_mean(const double* x, const int32_t* ptr, int32_t n, int32_t n_meshes, double* out, void* stream);
int morig_assign_joints(const double* pred, const int32_t* pred_ptr, int32_t n_pred, const double* gt, const int32_t* gt_ptr, int32_t n_gt,
                        int32_t n_meshes, const int32_t* match_ptr, int32_t n_match, double* cost, const int64_t* cost_off, int64_t n_cost,
                        int32_t* row_ind, int32_t* col_ind, double* dist, int32_t* status, void* stream);
int morig_joint_scores(const int32_t* row_ind, const double* dist, const int32_t* match_ptr, int32_t n_match, const int32_t* pred_ptr,
                       const int32_t* gt_ptr, const double* fs, const int32_t* fs_ptr, int32_t n_fs, int32_t n_meshes, int32_t* hits,
                       double* out, void* stream);
int morig_valid_mean(const double* x, const int32_t* valid, int32_t n_rows, int32_t n, double* out, void* stream);

/* ---- rig assembly (csrc/rig_assemble.hip; morig_amd/rigging.py): the last two statements of the rigging driver, assemble_skel_skin
 * (evaluate/joint2rig.py:147-162) and remove_dup_joints (:363-394), on the numbers: per-bone skin weights -> per-joint skins. float64
 * copies and fixed-order sums, ragged over the meshes of a batch, no atomics, nothing read back; plain parameters (no argument struct).
 * The tree bookkeeping is the host's and arrives as two CSR tables (int32, every ptr ascending from 0):
 *   vtx_ptr [n_meshes + 1] rows of W / out per mesh; joint_ptr [n_meshes + 1] output joints per mesh (global joint g = joint_ptr[m] + j);
 *   seg_ptr [n_joints + 1] segments of every output joint; bone_ptr [n_segs + 1] bones of every segment; bones [n_bones] columns of W
 *   (local to the mesh), ascending inside a segment.
 * morig_rig_assemble: W double [n_rows][ldw] (ldw in doubles, only columns < n_cols are read), out double [n_rows][ld_out] written whole.
 *   A segment's value is W[v][b] of its LAST bone b with W[v][b] > 1e-5 (strict; NaN counts as false), 0 without one; with
 *   MORIG_RIG_RAW in flags it is W[v][b] of its last bone, whatever the value. out[v][j] = the left-to-right sum of the values of joint
 *   j's segments, starting from the first segment's value itself; 0 for j past the mesh's joints and for rows no mesh names. A table
 *   entry that leaves its array is skipped; nothing is read out of bounds.
 * morig_rig_skin_entries: the entries != 0 of x double [n_rows][ld] (columns < n_cols), vertex-major with ascending joint, in two passes
 *   around the caller's prefix sum. ent_ptr == NULL: counts[v] = the entries of row v. Otherwise ent_ptr int32 [n_rows + 1] is the
 *   exclusive prefix sum of the counts and n_entries its last value: vertex (local to the mesh by vtx_ptr; -1 for a row no mesh names),
 *   joint, weight [n_entries] are filled. */
#define MORIG_RIG_RAW 1
int morig_rig_assemble(const double* W, int64_t ldw, int32_t n_cols, int32_t n_rows, const int32_t* vtx_ptr, const int32_t* joint_ptr,
                       int32_t n_meshes, const int32_t* seg_ptr, int32_t n_joints, const int32_t* bone_ptr, int32_t n_segs,
                       const int32_t* bones, int32_t n_bones, int32_t flags, double* out, int32_t ld_out, void* stream);
int morig_rig_skin_entries(const double* x, int32_t ld, int32_t n_rows, int32_t n_cols, const int32_t* vtx_ptr, int32_t n_meshes,
                           int32_t* counts, const int32_t* ent_ptr, int32_t n_entries, int32_t* vertex, int32_t* joint, double* weight,
                           void* stream);

/* ---- tracking without a rig (csrc/piecewise.hip, csrc/kabsch_core.h; morig_amd/piecewise.py): the reference's Piecewise_RANSAC
 * (utils/piecewise_ransac.py:12-45, :78-92) and KernelKMeans (utils/kernel_kmeans.py:11-27, :40-49, :67-98) for a ragged batch. float64
 * arithmetic, every sum in a fixed order, no floating-point atomics: two runs give the same bits. Plain parameters (no argument struct).
 * The RANSAC calls share: src, dst double [n_rows][3] (the vertices of all meshes, and their targets); a problem is a segment with >= 4
 *   handles; handles int32 [n_handles] rows of src / dst, hptr int32 [n_problems + 1] ascending from 0: problem p owns
 *   handles[hptr[p] .. hptr[p + 1]) in ascending vertex order; samples int32 [n_problems][n_iter][3] positions in the problem's handle
 *   list. An index that leaves its array is never followed: the hypothesis then counts 0 inliers with an infinite sum.
 * morig_ransac_vote: count int32, dsum double [n_problems][n_iter]: per hypothesis (the rigid fit to its three samples) the handles
 *   with |R s + t - d| < inlier_dist, and the sum of these distances over the handles.
 * morig_ransac_fit: per problem the reference's selection -- chosen int32 [n_problems][2] = the first hypothesis with the largest count
 *   (-1 while no count exceeds 0) and the first with the smallest sum (-1 while none is below 1e10); best_count int32 [n_problems];
 *   flag int32 [n_problems]: MORIG_RANSAC_REFIT when best_count > refit_share * (handles of the problem) as doubles -- Rt is then the
 *   fit to that hypothesis' inliers --, MORIG_RANSAC_SMALLEST_SUM -- Rt is the smallest-sum hypothesis --, MORIG_RANSAC_NONE when
 *   neither exists (the reference ends on None; Rt is the identity). Rt double [n_problems][12] = R row-major, then t.
 * morig_ransac_apply: out double [n_rows][3]; problem_of int32 [n_rows]: R v + t of that problem, dst[v] for a value outside
 *   [0, n_problems) (a segment with < 4 handles), src[v] under MORIG_RANSAC_NONE.
 * morig_kernel_kmeans: one workgroup per mesh. X [n_rows][D] float32 (x_is_f64 = 0) or float64, contiguous; pos double [n_rows][3];
 *   vptr int32 [n_meshes + 1]; first int32 [n_meshes] the first seed (local, clipped into the mesh). label_scratch int32 [n_rows],
 *   dist_scratch double [n_rows]. Results: labels int64 [n_rows] (rank among the kept clusters), seeds int32 [n_meshes][n_clusters],
 *   info int32 [n_meshes][4] = (MORIG_KMEANS_* status, iterations run, kept clusters, 0), members int32 [n_meshes][n_clusters] the
 *   member counts before the prune, centres_emb double [n_meshes][n_clusters][D] (float32-rounded values when X is float32), centres_euc
 *   double [n_meshes][n_clusters][3], fit double [n_meshes] the last fit sum. n_clusters above MORIG_KMEANS_MAX_CLUSTERS or D above
 *   MORIG_KMEANS_MAX_DIM: MORIG_E_UNSUPPORTED before anything is launched. */
#define MORIG_RANSAC_SMALLEST_SUM 0
#define MORIG_RANSAC_REFIT 1
#define MORIG_RANSAC_NONE 2
#define MORIG_KMEANS_OK 0
#define MORIG_KMEANS_BAD_MESH 1
#define MORIG_KMEANS_NO_CLUSTER 2
#define MORIG_KMEANS_MAX_CLUSTERS 64
#define MORIG_KMEANS_MAX_DIM 128
int morig_ransac_vote(const double* src, const double* dst, int32_t n_rows, const int32_t* handles, int32_t n_handles, const int32_t* hptr,
                      int32_t n_problems, const int32_t* samples, int32_t n_iter, double inlier_dist, int32_t* count, double* dsum,
                      void* stream);
int morig_ransac_fit(const double* src, const double* dst, int32_t n_rows, const int32_t* handles, int32_t n_handles, const int32_t* hptr,
                     int32_t n_problems, const int32_t* samples, int32_t n_iter, const int32_t* count, const double* dsum, double inlier_dist,
                     double refit_share, int32_t* chosen, int32_t* best_count, int32_t* flag, double* Rt, void* stream);
int morig_ransac_apply(const double* src, const double* dst, int32_t n_rows, const int32_t* problem_of, int32_t n_problems, const int32_t* flag,
                       const double* Rt, double* out, void* stream);
int morig_kernel_kmeans(const void* X, int32_t x_is_f64, const double* pos, int32_t n_rows, int32_t D, const int32_t* vptr, int32_t n_meshes,
                        const int32_t* first, int32_t n_clusters, int32_t max_iter, double w_euc, double tol, int32_t* label_scratch,
                        double* dist_scratch, int64_t* labels, int32_t* seeds, int32_t* info, int32_t* members, double* centres_emb,
                        double* centres_euc, double* fit, void* stream);

/* ---- the mesh front end (csrc/meshprep.hip, csrc/tribox_core.h; morig_amd/meshprep.py): from (vertices, faces) of a ragged batch to the
 * inputs of the other stages -- the reference's normalize (data_proc/common_ops.py:123-138) and get_tpl_edges (:15-32), and in place of
 * open3d's samples and the binvox program the product's own sampler and voxeliser. float64 in the written order, no
 * floating-point atomics: two runs give the same bits, a mesh alone the bits it gives in a batch. Plain parameters (no argument struct).
 * Shared: verts double [n_rows][3], the vertices of all meshes; vptr int32 [n_meshes + 1] ascending from 0; faces int32 [n_faces][3] vertex
 *   indices LOCAL to the face's mesh; fptr int32 [n_meshes + 1] ascending from 0. A face with an index outside its mesh is never followed:
 *   it gives no edge, no voxel and no area.
 * morig_mesh_bbox: bbox double [n_meshes][6] = minimum x, y, z, maximum x, y, z (+inf / -inf for a mesh without vertices).
 * morig_mesh_affine: frame double [n_meshes][4] = (t, s) per mesh; out [n_rows][3] = (v - t) * s under MORIG_MESH_NORMALIZE,
 *   (v - t) / s * mul under MORIG_MESH_GRID (the grid coordinate of the voxeliser, mul = dims).
 * morig_tpl_edge_keys: keys int64 [6 n_faces]: per face its six directed pairs (vptr[b] + v) << 32 | (vptr[b] + n); a pair of equal indices
 *   or of an index outside the mesh is INT64_MAX, which sorts last. The caller sorts the keys ascending.
 * morig_tpl_edge_flags: flags int32 [n_keys] = 1 at the first key of every run of the SORTED keys, 0 at repeats and at INT64_MAX.
 * morig_tpl_edge_compact: rank int64 [n_keys] the inclusive prefix sum of flags, n_edges its last value; out int64 [2][n_edges]: row 0 the
 *   vertex, row 1 the neighbour of every flagged key at rank - 1, both local to their mesh.
 * morig_voxel_surface: grid double [n_rows][3] grid coordinates; surface uint32 [n_meshes][dims * dims][MORIG_VOXEL_ROW_WORDS], zeroed
 *   here: bit z of row (x, y) is set when a triangle, as a closed set, overlaps the closed cube [x, x + 1] x [y, y + 1] x [z, z + 1]
 *   (touching counts). A triangle with a coordinate that is no finite number sets nothing.
 * morig_voxel_fill: solid uint8 [n_meshes][dims][dims][dims] indexed [x][y][z]: 1 on the surface voxels and on those that cannot be
 *   reached from outside the grid through 6-connected non-surface voxels. info int32 [n_meshes][2] = (MORIG_VOXEL_OK or
 *   MORIG_VOXEL_SWEEP_BOUND: the loop was ended at dims^3 sweeps, solid is then not final; sweeps run).
 *   1 <= dims <= MORIG_VOXEL_MAX_DIMS, MORIG_E_UNSUPPORTED otherwise, before anything is launched.
 * morig_tri_area_cdf: cum double [n_faces]: per mesh the running sum of its triangle areas in ascending face order.
 * morig_surface_samples: uniforms double [n_cand][3] in [0, 1); cptr int32 [n_meshes + 1] the candidates of every mesh. Candidate q of mesh
 *   b takes the first face with cum > u0 * (total area of b), the point (1 - sqrt u1) A + sqrt u1 (1 - u2) B + sqrt u1 u2 C and the unit
 *   normal (B - A) x (C - A) of that face. pts, normals double [n_cand][3]; tri int32 [n_cand] the face, local to the mesh (-1: a mesh
 *   without faces, or a face that is never followed; the point is then the origin). */
#define MORIG_MESH_NORMALIZE 0
#define MORIG_MESH_GRID 1
#define MORIG_VOXEL_ROW_WORDS 3
#define MORIG_VOXEL_MAX_DIMS 96
#define MORIG_VOXEL_OK 0
#define MORIG_VOXEL_SWEEP_BOUND 1
int morig_mesh_bbox(const double* verts, const int32_t* vptr, int32_t n_meshes, double* bbox, void* stream);
int morig_mesh_affine(const double* verts, int32_t n_rows, const int32_t* vptr, int32_t n_meshes, const double* frame, int32_t mode, double mul,
                      double* out, void* stream);
int morig_tpl_edge_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int64_t* keys,
                        void* stream);
int morig_tpl_edge_flags(const int64_t* keys, int64_t n_keys, int32_t* flags, void* stream);
int morig_tpl_edge_compact(const int64_t* keys, const int32_t* flags, const int64_t* rank, int64_t n_keys, const int32_t* vptr, int32_t n_meshes,
                           int64_t n_edges, int64_t* out, void* stream);
int morig_voxel_surface(const double* grid, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes,
                        int32_t dims, uint32_t* surface, void* stream);
int morig_voxel_fill(const uint32_t* surface, int32_t n_meshes, int32_t dims, uint8_t* solid, int32_t* info, void* stream);
int morig_tri_area_cdf(const double* verts, const int32_t* faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, double* cum,
                       void* stream);
int morig_surface_samples(const double* verts, const int32_t* faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const double* cum,
                          const double* uniforms, const int32_t* cptr, int32_t n_cand, double* pts, double* normals, int32_t* tri, void* stream);

/* ---- motion playback (csrc/playback.hip, csrc/pose_core.h; morig_amd/playback.py): the reference's smooth_quats
 * (evaluate/visualize_tracking.py:43-61) over Rig.FK (utils/rig_parser.py:63-79) for a ragged batch of rigs and one clip length T, and the
 * per-frame trajectory errors. float64 in the written order, no floating-point atomics: two runs give the same bits,
 * a mesh alone the bits it gives in a batch. Plain parameters (no argument struct).
 * Shared: jptr int32 [n_meshes + 1] the joint rows of every mesh, vptr int32 [n_meshes + 1] its vertex rows, both ascending from 0;
 *   parent int32 [n_joints] the parent of every joint LOCAL to its mesh, -1 at a root; order int32 [n_joints] per mesh its joints, local,
 *   parent before child (tracking.tree_order); eptr int32 [n_rows + 1] the skin entries of every vertex row, ascending from 0 to n_entries;
 *   ent_joint int32 [n_entries] local joints, ascending inside a vertex; ent_weight double [n_entries].
 *   status int32 [n_meshes], zeroed by the caller: MORIG_POSE_BAD_QUAT and MORIG_POSE_BAD_INDEX are ORed in. A mesh with
 *   MORIG_POSE_BAD_INDEX is skipped whole by every call that takes status: nothing of it is read through an index or written.
 * morig_pose_validate: sets MORIG_POSE_BAD_INDEX where a parent is outside [-1, J), an order entry outside [0, J), the entry offsets of a
 *   vertex do not rise inside [0, n_entries], or an entry names a joint outside [0, J). order and eptr may be NULL (not checked then).
 *   Call it before the others: they follow these indices unchecked.
 * morig_pose_quats: quats double [n_joints][T][4] = (x, y, z, w). quats_out (another buffer) receives the copy -- with align_signs != 0
 *   frame t negated when its dot product with the already aligned frame t - 1 is < 0 -- after `passes` passes of
 *   q[t] = ((q[t] + 0.5 q[t + 1]) + 0.5 q[t - 1]) / 2.0 over 1 <= t <= T - 2, every pass read from the pass before; T < 3: no pass.
 *   R (may be NULL) double [n_joints][9][T]: the rotation matrix of quats_out / its norm, row-major components, t fastest; a norm that is
 *   zero or no finite number sets MORIG_POSE_BAD_QUAT (the matrix is then the identity).
 * morig_pose_fk: offsets double [n_joints][3]; root_pos double [n_meshes][T][3], already rounded to the rig's position type; pos_f32 int32
 *   [n_meshes] non-zero where that type is float32. xf double [n_joints][12][T]: per joint and frame the global matrix (9, row-major) and
 *   the position (3). A root takes R and root_pos; a child G = G_parent R and pos = G_parent offset + pos_parent, float64 products and sums
 *   in index order, the position rounded to float32 on store where pos_f32 says so.
 * morig_pose_local: bind double [n_joints][12] the transforms the rigs hold (matrix, position); vtx double [n_rows][3];
 *   local double [n_entries][3] = inverse(bind[joint]) [v; 1] by adjugate / determinant and the translation -(A^-1 p).
 * morig_pose_skin: out double [n_rows][T][3] = sum over the vertex's entries with weight != 0, in stored order, of
 *   w (G local + pos); a vertex without entries gives zeros. Offsets into out are 64-bit. One wave covers MORIG_POSE_FRAME_TILE frames.
 * morig_pose_traj_errors: pred, gt double [n_rows][T][3]; vis uint8 [n_rows][T]. full, visible double [n_meshes][T]: per frame the mean
 *   vertex distance, and the sum of distance * (vis != 0) over the count of vis != 0 (0 / 0 = NaN). Sums: vertex lane l of 16 adds the
 *   vertices l, l + 16, ... ascending, then the lanes ascending. */
#define MORIG_POSE_BAD_QUAT 1
#define MORIG_POSE_BAD_INDEX 2
#define MORIG_POSE_FRAME_TILE 64
int morig_pose_validate(const int32_t* jptr, const int32_t* parent, const int32_t* order, const int32_t* vptr, const int32_t* eptr,
                        const int32_t* ent_joint, int32_t n_meshes, int32_t n_joints, int32_t n_rows, int32_t n_entries, int32_t* status,
                        void* stream);
int morig_pose_quats(const double* quats, const int32_t* jptr, int32_t n_meshes, int32_t n_joints, int32_t T, int32_t passes, int32_t align_signs,
                     double* quats_out, double* R, int32_t* status, void* stream);
int morig_pose_fk(const double* R, const int32_t* jptr, const int32_t* parent, const int32_t* order, const double* offsets, const double* root_pos,
                  const int32_t* pos_f32, int32_t n_meshes, int32_t T, const int32_t* status, double* xf, void* stream);
int morig_pose_local(const double* bind, const double* vtx, const int32_t* vptr, const int32_t* jptr, const int32_t* eptr, const int32_t* ent_joint,
                     int32_t n_meshes, int32_t n_rows, const int32_t* status, double* local, void* stream);
int morig_pose_skin(const double* xf, const int32_t* jptr, const int32_t* vptr, const int32_t* eptr, const int32_t* ent_joint,
                    const double* ent_weight, const double* local, int32_t n_meshes, int32_t n_rows, int32_t T, const int32_t* status, double* out,
                    void* stream);
int morig_pose_traj_errors(const double* pred, const double* gt, const uint8_t* vis, const int32_t* vptr, int32_t n_meshes, int32_t T, double* full,
                           double* visible, void* stream);

/* ---- depth scans (csrc/scan.hip, csrc/raytri_core.h; morig_amd/scan.py): depth images, partial point clouds, vertex visibility and
 * nearest-neighbour correspondences for a ragged batch of VIEWS. The reference only loads such data; the rules are
 * this product's own. float64 in the written order; the one atomic is a 64-bit integer minimum: two runs give the same bits, a view alone
 * the bits it gives in a batch. Plain parameters (no argument struct).
 * Shared: view v owns the vertex rows [vptr[v], vptr[v + 1]) of verts double [n_rows][3]; views int32 [n_views][MORIG_SCAN_VIEW_INTS] =
 *   (mesh, W, H, MORIG_SCAN_ORTHOGRAPHIC or MORIG_SCAN_PINHOLE); faces int32 [n_faces][3] local to the mesh, fptr int32 [n_meshes + 1];
 *   cams double [n_views][MORIG_SCAN_CAM_DOUBLES] = eye, f, r, u, px, py, near, 0 (raytri_core.h states the pixel ray); kptr int64
 *   [n_views + 1] the pixels of every view, kptr[v + 1] - kptr[v] = W H, row-major. A face index is clamped into the view's vertex rows;
 *   a view whose table entry is out of range draws nothing.
 * morig_scan_raster: wptr int64 [n_views + 1] the prefix sum of the views' face counts (one wave per entry), n_work its last value;
 *   mesh_nv int32 [n_meshes] the vertex count the faces of a mesh are checked against: *status (zeroed here) becomes MORIG_SCAN_BAD_FACE
 *   when a face names a vertex outside [0, mesh_nv). keys uint64 [n_pixels], set to all ones here, receive per pixel the minimum of
 *   (bits of float32(t) << 32 | face) over the faces the pixel's ray meets at t > near. min_side / max_side: the smallest and largest
 *   W or H of the call as the host knows them; outside 1 .. MORIG_SCAN_MAX_SIDE: MORIG_E_UNSUPPORTED before anything is launched.
 * morig_scan_resolve: per pixel depth double (t recomputed in float64 from the winning face, +inf without a hit), face int32 (-1), point
 *   double [3] = o + t d (+inf), flags int32 1 / 0.
 * morig_scan_compact: rank int64 [n_pixels] the inclusive prefix sum of flags, n_hits its last value. pts double [n_hits][3], pixel int32
 *   [n_hits] (row W + column inside the view), hit_face int32 [n_hits], in pixel order.
 * morig_scan_visibility: blk_ptr int32 [n_views + 1] the prefix sum of ceil(vertices / 256) per view, n_blocks its last value. vis uint8
 *   [n_rows]: 1 when the vertex projects into the closed image rectangle, its depth along f is > near, and no face that does not name it
 *   meets the segment from its camera point c (eye; orthographic: p - ((p - eye) . f) f) at 0 < t < 1 with t |d| < |d| - vis_eps.
 * morig_scan_nearest: segment b of n_segs: query rows [qptr[b], qptr[b + 1]) of q double [.][3], target rows [tptr[b], tptr[b + 1]) of t;
 *   mask uint8 per target row (NULL: all) -- a zero hides the row. blk_ptr as above over the query rows. idx int32 per query: the target,
 *   local to the segment, with the smallest (dx^2 + dy^2) + dz^2, the lowest index among equals, -1 when there is none; d2 double that
 *   squared distance (+inf). */
#define MORIG_SCAN_MAX_SIDE 1024
#define MORIG_SCAN_ORTHOGRAPHIC 0
#define MORIG_SCAN_PINHOLE 1
#define MORIG_SCAN_CAM_DOUBLES 16
#define MORIG_SCAN_VIEW_INTS 4
#define MORIG_SCAN_BAD_FACE 1
int morig_scan_raster(const double* verts, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* mesh_nv,
                      const double* cams, const int32_t* views, const int64_t* kptr, const int64_t* wptr, int32_t n_views, int32_t n_meshes,
                      int32_t min_side, int32_t max_side, int64_t n_pixels, int64_t n_work, uint64_t* keys, int32_t* status, void* stream);
int morig_scan_resolve(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams, const int32_t* views,
                       const int64_t* kptr, int32_t n_views, int32_t n_meshes, int64_t n_pixels, const uint64_t* keys, double* depth, int32_t* face,
                       double* point, int32_t* flags, void* stream);
int morig_scan_compact(const double* point, const int32_t* face, const int32_t* flags, const int64_t* rank, const int64_t* kptr, int32_t n_views,
                       int64_t n_pixels, int64_t n_hits, double* pts, int32_t* pixel, int32_t* hit_face, void* stream);
int morig_scan_visibility(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams, const int32_t* views,
                          const int32_t* blk_ptr, int32_t n_views, int32_t n_meshes, int32_t n_blocks, double vis_eps, uint8_t* vis, void* stream);
int morig_scan_nearest(const double* q, const int32_t* qptr, const double* t, const int32_t* tptr, const uint8_t* mask, const int32_t* blk_ptr,
                       int32_t n_segs, int32_t n_blocks, int32_t* idx, double* d2, void* stream);

/* ---- mesh simplification (csrc/simplify.hip, csrc/quadric_core.h; morig_amd/meshprep.py simplify): vertex clustering on a per-mesh grid
 * with a regularised quadric representative per occupied cell, where the reference calls open3d's
 * simplify_quadric_decimation. The rule is this product's own; no parity with the library exists or is claimed. float64 in the written
 * order, no floating-point atomics: two runs give the same bits, a mesh alone the bits it gives in a batch. Plain parameters (no argument
 * struct). verts, vptr, faces, fptr as in the mesh front end.
 * Shared: frame double [n_meshes][4] = (bounding-box minimum, largest extent); res int32 [n_meshes] the grid resolution r of every mesh,
 *   1 <= r <= MORIG_SIMPLIFY_MAX_RES. min_res / max_res: the smallest and largest r of the call as the host knows them; outside that range:
 *   MORIG_E_UNSUPPORTED before anything is launched. Output vertices ("cells") are numbered across the whole call in ascending
 *   (mesh, cell key) order; every such number must fit MORIG_SIMPLIFY_INDEX_BITS bits, so n_rows / n_cells above MORIG_SIMPLIFY_MAX_INDEX:
 *   MORIG_E_UNSUPPORTED before anything is launched.
 * morig_simplify_cell_keys: keys int64 [n_rows] = mesh << 30 | ((cx r + cy) r + cz) with g = (p - lo) / ext * r and, per axis,
 *   c = min((int)floor(g), r - 1) clamped into [0, r - 1]. The caller sorts them (stably: members stay in ascending vertex order), marks
 *   the first key of every run with morig_tpl_edge_flags and numbers the runs: that number is the vertex's cell.
 * morig_simplify_face_keys: cell int32 [n_rows] the cell of every vertex row. corner_cell int32 [3 n_faces] the cell of every corner
 *   (-1 where a face names a vertex outside its mesh: the face is never followed); keys int64 [n_faces] = the ascending triple of the
 *   face's cells at MORIG_SIMPLIFY_INDEX_BITS bits each, or INT64_MAX where two corners share a cell. The caller sorts them stably (the
 *   lowest input face stays first among equals) and marks the runs with morig_tpl_edge_flags.
 * morig_simplify_face_compact: order int64 [n_faces] the input face at every sorted position, flags its marks, rank int64 the inclusive
 *   prefix sum of the marks, n_out its last value; cptr int32 [n_meshes + 1] the cells of every mesh. out int64 [n_out][3]: the marked
 *   faces as cells LOCAL to their mesh, in the input face's orientation, rotated so that the smallest comes first.
 * morig_simplify_quadrics: one output vertex per cell. cell_key int64 [n_cells] the key of the cell; mptr int64 [n_cells + 1] its run in
 *   members int64 [n_rows] (vertex rows, ascending); kptr int64 [n_cells + 1] its run in corners int64 [3 n_faces] (3 face + corner,
 *   ascending; the corners of faces that are never followed lie in no run). Both tables are clamped into their arrays. out double [n_cells][3]: cen = the mean of the
 *   members; per corner n = (B - A) x (C - A) of its face, d = n . (A - cen), M += n n^T, b += n d; x = cen where trace M is not > 0,
 *   else cen + solve(M + 1e-3 trace(M) I, b) by Cholesky; x clamped per axis to the closed cell [lo + c h, lo + (c + 1) h], h = ext / r.
 *   Sums: lane l of 64 adds the terms l, l + 64, ... ascending, then the lanes are added under a fixed butterfly: the order depends on
 *   the run alone. */
#define MORIG_SIMPLIFY_MAX_RES 1024
#define MORIG_SIMPLIFY_INDEX_BITS 21
#define MORIG_SIMPLIFY_MAX_INDEX 2097152
#define MORIG_SIMPLIFY_MESH_SHIFT 30
int morig_simplify_cell_keys(const double* verts, int32_t n_rows, const int32_t* vptr, int32_t n_meshes, const double* frame, const int32_t* res,
                             int32_t min_res, int32_t max_res, int64_t* keys, void* stream);
int morig_simplify_face_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* cell,
                             int32_t n_rows, int32_t n_cells, int32_t* corner_cell, int64_t* keys, void* stream);
int morig_simplify_face_compact(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes,
                                const int32_t* cell, const int32_t* cptr, const int64_t* order, const int32_t* flags, const int64_t* rank,
                                int64_t n_out, int64_t* out, void* stream);
int morig_simplify_quadrics(const double* verts, int32_t n_rows, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr,
                            int32_t n_meshes, const double* frame, const int32_t* res, int32_t min_res, int32_t max_res, const int64_t* cell_key,
                            const int64_t* mptr, const int64_t* members, const int64_t* kptr, const int64_t* corners, int32_t n_cells,
                            double* out, void* stream);

/* ---- bone rays (csrc/labels.hip, csrc/boneray_core.h, csrc/raytri_core.h; morig_amd/labels.py): the nearest hit of arbitrary rays on the
 * meshes of a ragged batch, the per-joint statistics of the hit distances and the per-vertex attention label. The
 * reference only loads such labels ({id}_attn.txt, joint_featuresize/{id}.txt); the rule is this product's own. float64 in the written
 * order, no floating-point atomics: two runs give the same bits, a mesh alone the bits it gives in a batch. Plain parameters (no argument
 * struct). verts, vptr, faces, fptr as in the mesh front end (faces local to their mesh).
 * morig_ray_cast: mesh b owns the rays [ray_ptr[b], ray_ptr[b + 1]) of origins / dirs double [n_rays][3]. One wave per ray over the faces
 *   of its mesh through raytri_core.h with near = 0. t double [n_rays]: the smallest t > 0 (+inf: a miss); face int32: the lowest face
 *   among those with that t (-1); point double [n_rays][3] = o + t d (NaN). orientation, with n = (B - A) x (C - A): 0 any hit, +1 only
 *   hits with d . n > 0 (det < 0), -1 the opposite; a nearest hit of the wrong orientation makes the ray a miss, the ray does not continue.
 *   *status (zeroed here) collects MORIG_RAY_BAD_FACE (a face names a vertex outside its mesh: the index is clamped) and
 *   MORIG_RAY_BAD_TABLE (a ray outside every segment of ray_ptr: it misses).
 * morig_ray_select: joint j owns the values [joint_ptr[j], joint_ptr[j + 1]) of t. max_rays: the largest such count as the host knows it;
 *   above MORIG_RAY_MAX_PER_JOINT: MORIG_E_UNSUPPORTED before anything is launched. With s the joint's t < +inf sorted ascending and n
 *   their number: h = 0.2 (n - 1), lo = floor(h), p20 = s[lo] + (h - lo) (s[min(lo + 1, n - 1)] - s[lo]); kept uint8 per ray: t < +inf
 *   and t <= keep_factor p20; stats double [n_joints][MORIG_RAY_STATS] = (n, the number kept, p20 (NaN when n = 0), the sum of the kept t
 *   in ascending ray order over their number, or fill when nothing is kept).
 * morig_ray_attention: blk_ptr int32 [n_meshes + 1] the prefix sum of ceil(vertices / 256) per mesh, n_blocks its last value. attn float
 *   per vertex row: 1 when a kept ray of the vertex's mesh has a hit point with (dx^2 + dy^2) + dz^2 <= radius radius, else 0. */
#define MORIG_RAY_MAX_PER_JOINT 1024
#define MORIG_RAY_BAD_FACE 1
#define MORIG_RAY_BAD_TABLE 2
#define MORIG_RAY_STATS 4
int morig_ray_cast(const double* origins, const double* dirs, const int32_t* ray_ptr, int32_t n_rays, const double* verts, const int32_t* vptr,
                   const int32_t* faces, const int32_t* fptr, int32_t n_meshes, int32_t orientation, double* t, int32_t* face, double* point,
                   int32_t* status, void* stream);
int morig_ray_select(const double* t, const int32_t* joint_ptr, int32_t n_joints, int32_t max_rays, double keep_factor, double fill, uint8_t* kept,
                     double* stats, void* stream);
int morig_ray_attention(const double* verts, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* point,
                        const uint8_t* kept, const int32_t* ray_ptr, double radius, float* attn, void* stream);

/* ---- motion-stage evaluation (csrc/motion_metrics.hip, csrc/curve_core.h; morig_amd/motion_metrics.py): the integer tables behind
 * evaluate/eval_corr.py:17-22 (correspondence accuracy per tolerance) and evaluate/eval_attn.py:21, 31-34 (precision / recall per threshold)
 * for a ragged batch. Plain parameters (no argument struct). Every ptr comes from morig_loss_segment_ptr and *status
 * is the word that call wrote: with MORIG_LOSS_ST_UNSORTED or MORIG_LOSS_ST_SEGMENT in it nothing is read through the offsets and every
 * count is 0. Only integers are accumulated (no floating-point atomic): two runs give the same bits, a pair or mesh alone the counts it
 * gives in a batch. Ratios and means are the host's, in float64, from these tables. tol / thr are float arrays of 1 .. MORIG_CURVE_MAX_BINS
 * values (more: MORIG_E_UNSUPPORTED before anything is launched): the caller rounds its tolerances and thresholds to float32 ONCE, which
 * is how numpy 1.21 (the reference's) compares a Python float or a float64 scalar with a float32 array; numpy 2 compares the latter in
 * float64 and so moves every value equal to float32(t).
 * The rules, all in float32 with every operation rounded to nearest and never contracted:
 *   distance   d = a - b per component, s = (d0 d0 + d1 d1) + d2 d2 (the order of np.sum(axis=-1) on [n, 3]), dist = (float)sqrt((double)s),
 *              the correctly rounded float32 root. A hit: dist < tol, strict.
 *   normalise  mn, mx = the float32 minimum / maximum of the mesh, NaN as soon as one value is NaN (np.min); x' = (x - mn) / (mx - mn).
 *              A constant mesh gives 0 / 0 = NaN and counts nothing. A predicted positive: x' > thr, strict; a NaN never is one.
 * morig_corr_hits: pair b owns the points [ptr_pts[b], ptr_pts[b + 1]) of pts float [n_pts][3], the entries [ptr_vtx[b], ptr_vtx[b + 1]) of
 *   nn int32 [n_vtx] and the rows [ptr_corr[b], ptr_corr[b + 1]) of corr int64 [n_corr][2] = (v, p_gt), both local to the pair. nn[v] is
 *   the predicted point of vertex v: local to the pair (nn_global = 0, what the reference saves as _nnind.npy) or a row of pts
 *   (nn_global = 1, what morig_cosine_nn writes). hits int64 [n_pairs][n_tol] (zeroed here) counts per tolerance the rows with
 *   |pts[nn[v]] - pts[p_gt]| < tol. A row whose v, p_gt or nn[v] lies outside its pair counts nothing and sets MORIG_MOTION_ST_INDEX in
 *   *status.
 * morig_pr_counts: mesh b owns the rows [ptr[b], ptr[b + 1]) of pred float [n_rows] and gt uint8 [n_rows] (non-zero: a positive label).
 *   pp int64 [n_meshes][n_thr] counts the predicted positives per threshold, tp those with a positive label, gp int64 [n_meshes] the
 *   positive labels. normalize = 0 compares pred as it is. One workgroup per mesh; every entry of the three tables is written. */
#define MORIG_CURVE_MAX_BINS 32
#define MORIG_MOTION_ST_INDEX 16         /* shares the status word with the MORIG_LOSS_ST_ bits of morig_loss_segment_ptr */
int morig_corr_hits(const float* pts, int32_t n_pts, const int32_t* ptr_pts, const int32_t* nn, int32_t n_vtx, const int32_t* ptr_vtx,
                    int32_t nn_global, const int64_t* corr, int32_t n_corr, const int32_t* ptr_corr, int32_t n_pairs, const float* tol,
                    int32_t n_tol, int64_t* hits, int32_t* status, void* stream);
int morig_pr_counts(const float* pred, const uint8_t* gt, const int32_t* ptr, int32_t n_rows, int32_t n_meshes, const float* thr, int32_t n_thr,
                    int32_t normalize, int64_t* tp, int64_t* pp, int64_t* gp, const int32_t* status, void* stream);

/* ---- rig transfer between meshes (csrc/transfer.hip, csrc/pointtri_core.h; morig_amd/transfer.py): the reference's
 * transfer_rig_to_remesh (data_proc/common_ops.py:229-259) for a ragged batch, and the blend of skin rows at the closest surface point,
 * which is this product's own rule. float64 in the written order, no floating-point atomics: two runs give the same bits, a mesh alone
 * the bits it gives in a batch. Plain parameters (no argument struct). Every ptr is an int32 prefix sum [n_meshes + 1]; blk_ptr is the
 * prefix sum of ceil(vertices / MORIG_TRANSFER_BLOCK) per mesh and n_blocks its last value. No call zeroes *status: the caller does.
 * morig_transfer_keys: faces int32 [n_faces][3] local to their mesh. keys int64 [n_faces][per_face]: the directed pairs (v, n), n != v, as
 *   ((vptr[b] + v) << 32) | n. per_face 6: the pairs of the face's corners. per_face 15: for the corner position c (0, 1, 2) at which v
 *   stands, also the three vertices of face NUMBER c of the mesh (nothing where the mesh has no face c) -- the neighbour set the reference's
 *   faces[np.argwhere(faces == v)] yields. A slot without a pair holds INT64_MAX. A face with an index outside its mesh emits nothing and
 *   sets MORIG_TRANSFER_BAD_FACE in status[0].
 * morig_transfer_coincide: verts / ori double [..][3], the remeshed and the original vertices. coincident int32 per remeshed vertex: the
 *   lowest original vertex of its mesh with (dx^2 + dy^2) + dz^2 == 0, or -1; nearest: the lowest one with the smallest such value, or -1.
 *   A coordinate that is no finite number of magnitude <= 1e7 sets MORIG_TRANSFER_BAD_COORD in status[0] (the originals of a mesh without
 *   remeshed vertices are never read, so never checked).
 * morig_transfer_flood: one workgroup per mesh; max_verts: the largest vertex count as the host knows it, above MORIG_TRANSFER_MAX_FLOOD:
 *   MORIG_E_UNSUPPORTED before anything is launched. keys: the keys of morig_transfer_keys SORTED ascending; rowptr int32 [n_verts + 1]:
 *   rowptr[r] = the first key >= r << 32. sweep int32 per vertex: 0 coincident, else the sweep of the reference's loop that fills it, -1
 *   never. source int32: the original vertex whose row the vertex receives, the coincident vertex at the end of its chain of closest
 *   filled neighbours; never filled: nearest[v] when use_nearest, else -1. status[1 + b] += the vertices of mesh b with source -1.
 * morig_transfer_closest: per destination vertex the closest point over the faces of its source mesh (pointtri_core.h): face int32 the
 *   lowest face with the smallest squared distance (-1: none), bary double [..][3] (NaN), distance double (NaN) its root. A face index
 *   outside the mesh is clamped and sets MORIG_TRANSFER_BAD_FACE; a mesh with destination vertices and no face MORIG_TRANSFER_NO_FACES.
 * morig_transfer_rows: skins double, mesh b owning the row-major [src_vptr[b + 1] - src_vptr[b]][joints[b]] block at skin_ptr[b]; out
 *   alike at out_ptr[b] with one row per destination vertex. bary null: row = skins[pick[v]] (pick = source); else pick = face and
 *   row[j] = (b0 S[f0][j] + b1 S[f1][j]) + b2 S[f2][j]. Then row / (sum + 1e-8), the sum in ascending j. pick < 0: a row of zeros. */
#define MORIG_TRANSFER_BLOCK 256
#define MORIG_TRANSFER_MAX_FLOOD 8192
#define MORIG_TRANSFER_BAD_FACE 1
#define MORIG_TRANSFER_BAD_COORD 2
#define MORIG_TRANSFER_NO_FACES 4
int morig_transfer_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int32_t per_face,
                        int64_t* keys, int32_t* status, void* stream);
int morig_transfer_coincide(const double* verts, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* ori,
                            const int32_t* optr, int32_t* coincident, int32_t* nearest, int32_t* status, void* stream);
int morig_transfer_flood(const double* verts, const int32_t* vptr, int32_t n_meshes, int32_t max_verts, const int32_t* rowptr, const int64_t* keys,
                         const int32_t* coincident, const int32_t* nearest, int32_t use_nearest, int32_t* source, int32_t* sweep, int32_t* status,
                         void* stream);
int morig_transfer_closest(const double* dst, const int32_t* dptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const double* verts,
                           const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t* face, double* bary, double* distance,
                           int32_t* status, void* stream);
int morig_transfer_rows(const double* skins, const int32_t* skin_ptr, const int32_t* joints, const int32_t* src_vptr, const int32_t* faces,
                        const int32_t* fptr, const int32_t* vptr, const int32_t* blk_ptr, int32_t n_meshes, int32_t n_blocks, const int32_t* pick,
                        const double* bary, double* out, const int32_t* out_ptr, void* stream);

/* ---- local rigid motion (csrc/local_motion.hip, csrc/localfit_core.h; morig_amd/local_motion.py): the reference's
 * get_gt_rotation_icp (data_proc/common_ops.py:47-78) for a ragged batch and whole clips. float64 in the written order, no floating-point
 * atomics: two runs give the same bits, a mesh alone the bits it gives in a batch. Plain parameters. vptr is an int32 prefix sum
 * [n_meshes + 1]. status int32 [3], zeroed by the caller: [0] flags, [1] vertices in no face, [2] vertices with an empty patch.
 * morig_local_patches: one wave per vertex. keys: the keys of morig_transfer_keys with per_face 6, SORTED ascending; rowptr int32
 *   [n_verts + 1]: rowptr[r] = the first key >= r << 32. The candidates of v are the end points of the walks of exactly four edges from v
 *   (the reference's two rounds of list unions; with every edge in a proper triangle: breadth-first depth <= 4, v included); a candidate u
 *   is a member under a rung r when sqrt((d0^2 + d1^2) + d2^2) < r. rung0..2: the ladder, computed by the host. The first rung with at
 *   least 5 members is used, else rung2. ids null (first pass): counts [n_verts] receives the patch sizes, rung [n_verts] the rung used
 *   (0 / 1 / 2); a vertex in no face has the patch {v} and adds 1 to status[1]; a coordinate that is no finite number sets
 *   MORIG_LOCAL_BAD_COORD. ids given (second pass): counts is the exclusive prefix sum [n_verts + 1] of the first pass, rung is read, and
 *   ids [counts[n_verts]] receives the members, local to their mesh, in ascending index. max_verts: the largest vertex count of a mesh as
 *   the host knows it; above MORIG_LOCAL_MAX_VERTS: MORIG_E_UNSUPPORTED before anything is launched.
 * morig_local_fit: one lane per (vertex, frame). verts0 double [n_verts][3]; traj double, or float where traj_is_f32, [n_verts][frames][3];
 *   patch_ptr int32 [n_verts + 1] and ids int32 [n_ids] local to their mesh: the patches. Per fit: rot6d [..][6] the first then the second
 *   column of R, trans [..][3], gap = (l1 - l2) / l1 of Horn's matrix (0 where l1 <= 0), residual = the root-mean-square of |R p + t - q|
 *   over the patch. An empty patch gives NaN and adds 1 to status[2] (once per vertex); an id outside its mesh is clamped and sets
 *   MORIG_LOCAL_BAD_ID. n_verts * frames above (2^31 - 1) / 6: MORIG_E_UNSUPPORTED before anything is launched. */
#define MORIG_LOCAL_MAX_VERTS 32768
#define MORIG_LOCAL_BAD_FACE 1
#define MORIG_LOCAL_BAD_COORD 2
#define MORIG_LOCAL_BAD_ID 4
int morig_local_patches(const double* verts, const int32_t* vptr, int32_t n_meshes, int32_t n_verts, int32_t max_verts, const int32_t* rowptr,
                        const int64_t* keys, double rung0, double rung1, double rung2, int32_t* counts, int32_t* rung, int32_t* ids, int32_t* status,
                        void* stream);
int morig_local_fit(const double* verts0, const void* traj, int32_t traj_is_f32, const int32_t* vptr, int32_t n_meshes, int32_t n_verts, int32_t frames,
                    const int32_t* patch_ptr, const int32_t* ids, int32_t n_ids, double* rot6d, double* trans, double* gap, double* residual,
                    int32_t* status, void* stream);

/* ---- mesh BVH (csrc/bvh.hip, csrc/bvh_core.h; morig_amd/spatial.py): a 64-wide implicit tree per mesh of a ragged
 * batch, two queries on it that return what morig_ray_cast and morig_transfer_closest return, bit for bit, under the condition that
 * section states, and the any-hit test of segments. float64 in the written order, no floating-point atomics: two runs give the same
 * bits, a mesh alone the bits it gives in a batch. Plain parameters. verts, vptr, faces, fptr as in the mesh front end (faces local to their mesh).
 * morig_bvh_build_keys: bbox double [n_meshes][6] from morig_mesh_bbox. keys int64 [n_faces] = mesh << 30 | the 30-bit Morton code of the
 *   face's centroid ((A + B) + C) / 3 in the frame (bbox minimum, largest extent), 10 bits per axis, x highest; code 0 where the extent is
 *   not > 0 or the centroid is no finite number. The caller sorts the keys with a STABLE sort; order int32 [n_faces] is the row of faces at
 *   every sorted position.
 * morig_bvh_boxes: node_ptr int32 [4][n_meshes + 1]: mesh b owns the rows [node_ptr[k - 1][b], node_ptr[k - 1][b + 1]) of boxes at level
 *   k, the levels one after another; n1 .. n4 the nodes of every level over all meshes and max_faces the largest face count of a mesh, as
 *   the host knows them (max_faces above MORIG_BVH_MAX_FACES: MORIG_E_UNSUPPORTED before anything is launched). A mesh has
 *   ceil(faces / 64) nodes at level 1 and ceil(n / 64) at the level above one of n > 1 nodes. boxes double [n1 + n2 + n3 + n4][6]: the exact
 *   minimum x, y, z and maximum x, y, z of 64 consecutive sorted faces (level 1) or nodes of the level below; a face with a NaN corner
 *   adds nothing, the box of nothing is (+inf x 3, -inf x 3). flags int32 [n_meshes] (zeroed here): MORIG_BVH_BAD_FACE where a face names
 *   a vertex outside its mesh (the index is clamped, as in the brute-force kernels). Calling it again with other verts refits the tree.
 * morig_bvh_ray_cast: the arguments and results of morig_ray_cast, the same status bits. visits int32 [n_rays], may be null: the box and
 *   face tests made for the ray.
 * morig_bvh_closest: mesh b owns the points [pptr[b], pptr[b + 1]). face, bary, distance and the status bits of morig_transfer_closest
 *   (*status is NOT zeroed here either). visits int32 [n_points], may be null.
 * morig_bvh_blocked: mesh m owns the segments [seg_ptr[m], seg_ptr[m + 1]) from a to b, double [n_segments][3]. blocked uint8: 1 when a
 *   face of the segment's mesh that does not name vertex skip_vertex[q] (local to the mesh; none when negative or skip_vertex is null)
 *   is hit by the ray a + t (b - a) under raytri_core.h with near = 0 at t < t_max[q] (1 when t_max is null). Any hit: the walk ends with
 *   the first leaf that holds one. *status (zeroed here) collects the bits of morig_ray_cast. visits int32 [n_segments], may be null. */
#define MORIG_BVH_MAX_FACES 16777216
#define MORIG_BVH_BAD_FACE 1
int morig_bvh_build_keys(const double* verts, const int32_t* vptr, const int32_t* faces, int32_t n_faces, const int32_t* fptr, int32_t n_meshes,
                         const double* bbox, int64_t* keys, void* stream);
int morig_bvh_boxes(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t n_meshes, int64_t max_faces,
                    const int32_t* order, const int32_t* node_ptr, int32_t n1, int32_t n2, int32_t n3, int32_t n4, double* boxes, int32_t* flags,
                    void* stream);
int morig_bvh_ray_cast(const double* origins, const double* dirs, const int32_t* ray_ptr, int32_t n_rays, const double* verts, const int32_t* vptr,
                       const int32_t* faces, const int32_t* fptr, int32_t n_meshes, const int32_t* order, const double* boxes,
                       const int32_t* node_ptr, const int32_t* flags, int32_t orientation, double* t, int32_t* face, double* point, int32_t* visits,
                       int32_t* status, void* stream);
int morig_bvh_closest(const double* points, const int32_t* pptr, int32_t n_points, const double* verts, const int32_t* vptr, const int32_t* faces,
                      const int32_t* fptr, int32_t n_meshes, const int32_t* order, const double* boxes, const int32_t* node_ptr,
                      const int32_t* flags, int32_t* face, double* bary, double* distance, int32_t* visits, int32_t* status, void* stream);
int morig_bvh_blocked(const double* a, const double* b, const int32_t* seg_ptr, int32_t n_segments, const int32_t* skip_vertex, const double* t_max,
                      const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, int32_t n_meshes, const int32_t* order,
                      const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* blocked, int32_t* visits, int32_t* status,
                      void* stream);

/* ---- visibility on the mesh BVH (csrc/bvh.hip, csrc/bonevis_core.h): the rules of morig_scan_visibility and
 * morig_bone_visibility as walks of the tree, for the same bits under the conditions that section states. Plain parameters.
 * morig_bvh_view_boxes: a tree per VIEW of a scan. View v owns the vertex rows [vptr[v], vptr[v + 1]) of verts and draws the faces of
 *   mesh view_mesh[v] (int32 [n_views]) in that mesh's order (order int32 [n_faces] as for morig_bvh_boxes, one per mesh whatever pose
 *   sorted it). node_ptr int32 [4][n_views + 1] and n1 .. n4 as in morig_bvh_boxes with the view in the place of the mesh, from the face
 *   counts of the views' meshes; max_faces the largest of them. boxes exact for the view's own vertices; flags int32 [n_views] (zeroed
 *   here) as in morig_bvh_boxes. A view whose mesh is out of range gets empty boxes.
 * morig_bvh_scan_visibility: the tables of morig_scan_visibility and the view trees. vis uint8 [n_rows] as morig_scan_visibility writes
 *   it; visits int32 [n_rows], may be null: the box and face tests of the vertex, 0 for a vertex outside the frustum or of an invalid
 *   view. *status (zeroed here) becomes MORIG_SCAN_BAD_FACE where a walked view's flag word holds MORIG_BVH_BAD_FACE.
 * morig_bvh_bone_visibility: the tables of morig_bone_visibility, n_pairs = off[n_meshes], and the tree of the occluders (tri_pos, tp_ptr,
 *   faces, f_ptr in the places of verts, vptr, faces, fptr of morig_bvh_boxes). vis uint8 [n_pairs] as morig_bone_visibility writes it;
 *   visits int32 [n_pairs], may be null. *status (zeroed here) collects MORIG_BVH_BAD_FACE. */
int morig_bvh_view_boxes(const double* verts, const int32_t* vptr, const int32_t* view_mesh, int32_t n_views, const int32_t* faces, const int32_t* fptr,
                         int32_t n_meshes, int64_t max_faces, const int32_t* order, const int32_t* node_ptr, int32_t n1, int32_t n2, int32_t n3,
                         int32_t n4, double* boxes, int32_t* flags, void* stream);
int morig_bvh_scan_visibility(const double* verts, const int32_t* vptr, const int32_t* faces, const int32_t* fptr, const double* cams,
                              const int32_t* views, int32_t n_views, int32_t n_meshes, int32_t n_rows, double vis_eps, const int32_t* order,
                              const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* vis, int32_t* visits, int32_t* status,
                              void* stream);
int morig_bvh_bone_visibility(const double* pos, const int32_t* vtx_ptr, const double* bones, const int32_t* bone_ptr, const double* tri_pos,
                              const int32_t* tp_ptr, const int32_t* faces, const int32_t* f_ptr, const int64_t* off, int32_t n_meshes, int64_t n_pairs,
                              const int32_t* order, const double* boxes, const int32_t* node_ptr, const int32_t* flags, uint8_t* vis, int32_t* visits,
                              int32_t* status, void* stream);

/* ---- mesh diagnosis and cleaning (csrc/meshcheck.hip, csrc/topo_core.h; morig_amd/meshprep.py diagnose / clean):
 * weld classes, degenerate and duplicate faces, the edges of the kept faces and their classes, connected components and the compaction
 * of the cleaned mesh. The rule is this product's own; no parity with any mesh library exists or is claimed. Integers and float64 in the
 * written order; the only atomics are integer OR / add / min: two runs give the same bits, a mesh alone the bits it gives in a batch.
 * Plain parameters (no argument struct). verts, vptr, faces, fptr as in the mesh front end. A "row" is a vertex row of the batch; every
 * count is at most 2^31 - 257. Every export refuses a negative count and a null pointer with MORIG_E_INVALID and returns MORIG_OK for zero
 * meshes / zero rows before anything is launched. The caller sorts (stably where said) and takes prefix sums between the calls.
 * morig_meshcheck_coord_keys: keys int64 [3][n_rows] (x, y, z): key(a) < key(b) exactly when a < b, -0.0 keyed as +0.0: a non-negative
 *   double keeps its bit pattern, a negative one has its 63 magnitude bits flipped. nonfinite int32 [n_rows]: 1 where a coordinate of
 *   the row is an infinity or a NaN.
 * morig_meshcheck_weld_mark: order int64 [n_rows] the rows after stable sorts by the z, the y and the x key. flags int32 [n_rows] = 1 at
 *   the first row of every run of rows of ONE mesh with three equal keys; a non-finite row is a run of its own.
 * morig_meshcheck_run_rep: order / flags as above, rank int64 [n] the inclusive prefix sum of flags, dead int32 [n] per ITEM (may be
 *   null), start int32 [n] scratch. rep int32 [n]: for every item the first item of its run (stable sorts: the lowest), -1 where dead.
 * morig_meshcheck_face_keys: rep int32 [n_rows] the representative row of every row. tri int32 [n_faces][3] the representatives of the
 *   corners (-1 x 3 where the face names a vertex outside its mesh: *status |= MORIG_MESHCHECK_BAD_FACE, the face counts as degenerate;
 *   *status is NOT zeroed here); degenerate int32 [n_faces]: two corners in one class; major int64 = the lowest of the three rows,
 *   minor = middle << 32 | highest, both INT64_MAX where degenerate. The caller sorts stably by minor, then by major.
 * morig_meshcheck_face_mark: order int64 [n_faces] the faces so sorted; flags = 1 at the first face of every run of equal (major, minor),
 *   0 at the degenerate ones. morig_meshcheck_run_rep with dead = degenerate then gives surv int32 [n_faces]: the surviving (lowest)
 *   face of every vertex set, -1 where degenerate; a face is KEPT when it is its own survivor.
 * morig_meshcheck_face_edges: referenced int32 [n_rows] (zeroed here) = 1 where a kept face names the row; zero_area int32 [n_faces] = 1
 *   where a kept face's normal (B - A) x (C - A) is exactly (0, 0, 0); ekeys int64 [3 n_faces]: per kept face its edges a -> b, b -> c,
 *   c -> a as lo << 32 | hi << 1 | dir, dir = 1 where the face runs low -> high; INT64_MAX for the other faces.
 * morig_meshcheck_cc_round: one round of the component rule on the rows. With gp = cur[cur] and m[v] = min(gp[v], gp[n] over the
 *   neighbours n of v): next[v] = min(cur[v], m[v]), then next[cur[v]] = min(next[cur[v]], m[v]). Reads cur only (cur != next), writes
 *   all of next; changed int32 [n_meshes] (zeroed here) = 1 for every mesh whose rows differ between next and cur. ekeys in any order;
 *   INT64_MAX is skipped.
 * morig_meshcheck_edge_classify: keys the SORTED ekeys, label int32 [n_rows] the converged labels. eclass int32 [n_keys]: at the first
 *   key of every run MORIG_EDGE_MANIFOLD / _BOUNDARY (one face) / _NONMANIFOLD (three or more) / _CONFLICT (two faces, not exactly one
 *   of them low -> high), 0 elsewhere. root_boundary int32 [n_rows] (zeroed here): the boundary edges of the component whose label is
 *   that row.
 * morig_meshcheck_comp_counts: root_verts / root_faces int32 [n_rows] (zeroed here): referenced rows / kept faces per label; a face
 *   belongs to the component of its first corner. face_root int64 [n_faces]: that label, 2^31 - 1 for a face that is not kept.
 * morig_meshcheck_comp_area: order int64 [n_faces] the faces sorted stably by face_root, kptr int64 [n_comps + 1] the run of every
 *   component. area double [n_comps]: lane l of 64 adds 0.5 sqrt((nx^2 + ny^2) + nz^2) of the run's faces l, l + 64, ... in that order,
 *   then lane l takes lane l + h for h = 32, 16, 8, 4, 2, 1.
 * morig_meshcheck_keep_flags: keep_root int32 [n_rows]: whether the component of that label stays. vkeep int32 [n_rows] = the row is its
 *   own representative and (drop_unreferenced: is referenced and its component stays); fkeep int32 [n_faces] = kept and its component
 *   stays.
 * morig_meshcheck_compact: vrank / frank int64 the inclusive prefix sums of vkeep / fkeep, n_out_v / n_out_f their last values, ovptr /
 *   ofptr int64 [n_meshes + 1] the output rows in front of every mesh. out_verts double [n_out_v][3] the coordinates of the leaving
 *   rows; out_faces int64 [n_out_f][3] the leaving faces in input order, corners unrotated, as output vertices local to the mesh;
 *   vertex_map int64 [n_rows] / face_map int64 [n_faces]: the output vertex / face local to the mesh (a duplicate face: that of its
 *   survivor), -1 where none. */
#define MORIG_MESHCHECK_BAD_FACE 1
#define MORIG_MESHCHECK_ROUND_GUARD 2
#define MORIG_EDGE_MANIFOLD 1
#define MORIG_EDGE_BOUNDARY 2
#define MORIG_EDGE_NONMANIFOLD 3
#define MORIG_EDGE_CONFLICT 4
int morig_meshcheck_coord_keys(const double* verts, int32_t n_rows, int64_t* keys, int32_t* nonfinite, void* stream);
int morig_meshcheck_weld_mark(const int64_t* keys, const int32_t* nonfinite, const int64_t* order, int32_t n_rows, const int32_t* vptr,
                              int32_t n_meshes, int32_t* flags, void* stream);
int morig_meshcheck_run_rep(const int64_t* order, const int32_t* flags, const int64_t* rank, const int32_t* dead, int32_t n, int32_t* start,
                            int32_t* rep, void* stream);
int morig_meshcheck_face_keys(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* rep,
                              int32_t n_rows, int32_t* tri, int64_t* major, int64_t* minor, int32_t* degenerate, int32_t* status, void* stream);
int morig_meshcheck_face_mark(const int64_t* major, const int64_t* minor, const int64_t* order, int32_t n_faces, int32_t* flags, void* stream);
int morig_meshcheck_face_edges(const double* verts, int32_t n_rows, const int32_t* tri, const int32_t* surv, int32_t n_faces, int32_t* referenced,
                               int32_t* zero_area, int64_t* ekeys, void* stream);
int morig_meshcheck_cc_round(const int32_t* cur, int32_t* next, int32_t n_rows, const int64_t* ekeys, int64_t n_keys, const int32_t* vptr,
                             int32_t n_meshes, int32_t* changed, void* stream);
int morig_meshcheck_edge_classify(const int64_t* keys, int64_t n_keys, const int32_t* label, int32_t n_rows, int32_t* eclass, int32_t* root_boundary,
                                  void* stream);
int morig_meshcheck_comp_counts(const int32_t* tri, const int32_t* surv, int32_t n_faces, const int32_t* referenced, const int32_t* label,
                                int32_t n_rows, int32_t* root_verts, int32_t* root_faces, int64_t* face_root, void* stream);
int morig_meshcheck_comp_area(const double* verts, int32_t n_rows, const int32_t* tri, int32_t n_faces, const int64_t* order, const int64_t* kptr,
                              int32_t n_comps, double* area, void* stream);
int morig_meshcheck_keep_flags(const int32_t* rep, const int32_t* referenced, const int32_t* label, const int32_t* keep_root, int32_t drop_unreferenced,
                               int32_t n_rows, const int32_t* tri, const int32_t* surv, int32_t n_faces, int32_t* vkeep, int32_t* fkeep, void* stream);
int morig_meshcheck_compact(const double* verts, const int32_t* rep, const int32_t* vkeep, const int64_t* vrank, const int32_t* vptr,
                            const int64_t* ovptr, int32_t n_rows, int32_t n_meshes, const int32_t* tri, const int32_t* surv, const int32_t* fkeep,
                            const int64_t* frank, const int32_t* fptr, const int64_t* ofptr, int32_t n_faces, int64_t n_out_v, int64_t n_out_f,
                            double* out_verts, int64_t* out_faces, int64_t* vertex_map, int64_t* face_map, void* stream);

/* ---- mesh repair (csrc/meshfix.hip, csrc/orient_core.h; morig_amd/meshprep.py repair): a consistent orientation
 * per component by the double cover of the face graph, the boundary loops by pointer doubling, and a centroid fan for every simple loop.
 * The rule is this product's own; no parity with any mesh library exists or is claimed. The conventions of the section above hold:
 * integers and float64 in the written order, integer atomics only (OR, add, min) and relaxed stores of 1, plain parameters, every count
 * at most 2^31 - 257, MORIG_E_INVALID for a negative count or a null pointer, MORIG_OK for zero work before anything is launched. The
 * input is a CLEANED batch (no degenerate and no duplicate face). A "record" is one of the 3 n_faces face edges.
 * morig_meshfix_edge_records: tri int32 [n_faces][3] the corners as rows of the batch; per face and corner c the edge c -> c + 1 as
 *   keys int64 [3 n_faces] = lo << 32 | hi and vals int32 = face << 1 | dir (dir = 1: the face runs low -> high), in face-major order. A
 *   face that names a vertex outside its mesh or one vertex twice: *status |= MORIG_MESHCHECK_BAD_FACE (not zeroed here), tri -1, keys
 *   INT64_MAX. The caller sorts the records STABLY by key (the faces of a run ascend).
 * morig_meshfix_links: keys / vals the sorted records. A run of exactly two records (faces f < g) is a link of parity p = (dir_f ==
 *   dir_g): its first record gets cover[i] = (2f) << 32 | (2g + p) << 1, its second (2f + 1) << 32 | (2g + (1 ^ p)) << 1 -- edges of
 *   the double cover in morig_meshcheck_cc_round's key layout; every other record INT64_MAX. face_open int32 [n_faces] (zeroed here) = 1
 *   for a face with a record in a run that is not two long; bflag int32 [3 n_faces] = 1 at a run of one (a boundary half-edge).
 * morig_meshfix_orient_stats: lab int32 [2 n_faces] the converged labels of the cover (node 2f + s). root int32 [n_faces] = lab[2f] >> 1,
 *   parity int32 = lab[2f] & 1, face_root int64 = root (for the component sort), root_open int32 [n_faces] (zeroed here) = 1 at the root
 *   of a component with an open face.
 * morig_meshfix_signed_volume: order int64 [n_faces] the faces sorted stably by face_root, kptr int64 [n_comps + 1] the run of every
 *   component, roots int64 [n_comps] its root. Per component, one wave: lane l adds t(f) = (Ax (By Cz - Bz Cy) + Ay (Bz Cx - Bx Cz))
 *   + Az (Bx Cy - By Cx), negated where parity = 1, of the run's faces l, l + 64, ...; lane l takes lane l + h, h = 32 .. 1 -> vol
 *   double [n_faces] at the root; cnt / cnt1 int32 [n_faces] at the root: its faces / those of parity 1. All three zeroed here.
 * morig_meshfix_orient_apply: the decision per component. lab[2r] == lab[2r + 1]: not orientable, nothing flips. Else the class that
 *   flips is: closed (root_open = 0) and vol > 0: parity 1; closed and vol < 0: parity 0; otherwise (open, vol 0 or NaN) the class with
 *   fewer faces, parity 1 on a tie. out_faces int64 [n_faces][3] local to the mesh, corners 1 and 2 exchanged where flipped int32 = 1;
 *   rootinfo int32 [n_faces]: at a root MORIG_MESHFIX_ORIENTABLE or _NONORIENTABLE, | _CLOSED (orientable, no open face), | _INVERTED
 *   (closed, decided by the volume, every face flipped); 0 elsewhere.
 * morig_meshfix_boundary_init: per record with bflag the half-edge from -> to in the direction of its face AFTER the flips (hfrom / hto
 *   int32 [3 n_faces], -1 elsewhere); outdeg / indeg int32 [n_rows] count them (zeroed here), nxt[from] = the lowest to. vclass int32
 *   [n_rows]: MORIG_MESHFIX_REGULAR (one out, one in): lab = the row, nxt = to; MORIG_MESHFIX_TANGLED (any other boundary vertex):
 *   lab = -1, nxt = the row; 0 (no boundary vertex): lab = -1, nxt = the row.
 * morig_meshfix_loop_round: lab2[v] = min(lab[v], lab[nxt[v]]), nxt2[v] = nxt[nxt[v]]; reads lab / nxt only (lab2, nxt2 other arrays).
 * morig_meshfix_loop_centroid: order int64 [n_rows] the rows sorted stably by loop label, lptr int64 [n_loops + 1] the run of every
 *   loop, sel int64 [n_sel] the loops to fill. centroid double [n_sel][3]: per coordinate lane l adds the run's rows l, l + 64, ...,
 *   the fold as above, divided by the length.
 * morig_meshfix_fill_mark: slot int32 [n_rows]: at a loop's label its rank among the selected loops, else -1. emit int32 [n_rows] = 1
 *   for a regular row with lab >= 0 and slot[lab] >= 0.
 * morig_meshfix_fill_emit: nxt0 the nxt of boundary_init, erank int64 the inclusive prefix sum of emit, sptr int64 [n_meshes + 1] the
 *   selected loops in front of every mesh. Row v with emit writes out_faces[erank[v] - 1] = (nxt0[v], v, n_v + slot[lab[v]] - sptr[b]),
 *   the first two local to mesh b, n_v its vertex count. */
#define MORIG_MESHFIX_ORIENTABLE 1
#define MORIG_MESHFIX_NONORIENTABLE 2
#define MORIG_MESHFIX_CLOSED 4
#define MORIG_MESHFIX_INVERTED 8
#define MORIG_MESHFIX_REGULAR 1
#define MORIG_MESHFIX_TANGLED 2
int morig_meshfix_edge_records(const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, int32_t n_rows,
                               int32_t* tri, int64_t* keys, int32_t* vals, int32_t* status, void* stream);
int morig_meshfix_links(const int64_t* keys, const int32_t* vals, int64_t n_records, int32_t n_faces, int64_t* cover, int32_t* face_open,
                        int32_t* bflag, void* stream);
int morig_meshfix_orient_stats(const int32_t* lab, const int32_t* face_open, int32_t n_faces, int32_t* root, int32_t* parity, int64_t* face_root,
                               int32_t* root_open, void* stream);
int morig_meshfix_signed_volume(const double* verts, int32_t n_rows, const int32_t* tri, const int32_t* parity, int32_t n_faces,
                                const int64_t* order, const int64_t* kptr, const int64_t* roots, int32_t n_comps, double* vol, int32_t* cnt,
                                int32_t* cnt1, void* stream);
int morig_meshfix_orient_apply(const int32_t* tri, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, int32_t n_meshes, const int32_t* lab,
                               const int32_t* root, const int32_t* parity, const int32_t* root_open, const double* vol, const int32_t* cnt,
                               const int32_t* cnt1, int64_t* out_faces, int32_t* flipped, int32_t* rootinfo, void* stream);
int morig_meshfix_boundary_init(const int64_t* keys, const int32_t* vals, const int32_t* bflag, int64_t n_records, const int32_t* flipped,
                                int32_t n_faces, int32_t n_rows, int32_t* hfrom, int32_t* hto, int32_t* outdeg, int32_t* indeg, int32_t* nxt,
                                int32_t* lab, int32_t* vclass, void* stream);
int morig_meshfix_loop_round(const int32_t* lab, const int32_t* nxt, int32_t n_rows, int32_t* lab2, int32_t* nxt2, void* stream);
int morig_meshfix_loop_centroid(const double* verts, int32_t n_rows, const int64_t* order, const int64_t* lptr, int32_t n_loops, const int64_t* sel,
                                int32_t n_sel, double* centroid, void* stream);
int morig_meshfix_fill_mark(const int32_t* vclass, const int32_t* lab, const int32_t* slot, int32_t n_rows, int32_t* emit, void* stream);
int morig_meshfix_fill_emit(const int32_t* nxt0, const int32_t* emit, const int64_t* erank, const int32_t* lab, const int32_t* slot,
                            const int32_t* vptr, const int64_t* sptr, int32_t n_rows, int32_t n_meshes, int64_t n_out, int64_t* out_faces,
                            void* stream);

/* ---- mesh refinement (csrc/refine.hip, csrc/split_core.h; morig_amd/meshprep.py refine / interpolate): one pass of
 * edge splits over a ragged batch, and the interpolation of per-vertex values along the parents. The rule is this product's own; no
 * parity with any mesh library exists or is claimed. The conventions of the two sections above hold: integers and float64 in the
 * written order, no floating-point atomic (one integer atomic max, one integer OR), plain parameters, every count at most 2^31 - 257,
 * MORIG_E_INVALID for a negative count, a count the 32-bit rows cannot hold or a null pointer, MORIG_OK for zero work before anything is
 * launched. faces int32 [n_faces][3] are local to their mesh; a "record" is one of the 3 n_faces face edges, record 3 f + c the edge from
 * corner c to corner c + 1 of face f.
 * morig_refine_edge_records: keys int64 [3 n_faces] = lo << 32 | hi of the edge's rows, len2 double [3 n_faces] = (d0 d0 + d1 d1) + d2 d2
 *   with d = verts[hi] - verts[lo]; maxbits int64 [n_meshes], zeroed here: the largest bit pattern of a FINITE len2 of the mesh (integer
 *   atomic max; 0 where there is none). A face that names one vertex twice: degenerate[f] = 1, its three keys INT64_MAX and len2 0 (it
 *   is never split and takes part in nothing). A face that names a vertex outside its mesh: the same with degenerate 0, and
 *   *status |= MORIG_MESHCHECK_BAD_FACE (not zeroed here). n_faces at most (2^31 - 257) / 3.
 * morig_refine_mark: keys the SORTED record keys, order int64 the record at every sorted position, flags the run starts
 *   (morig_tpl_edge_flags). Per sorted position i of mesh b (that of its low row): mark int32 = 1 where i begins a run, len2 is finite and
 *   mode[b] is MORIG_REFINE_LENGTH and len2 > limit2, or mode[b] is MORIG_REFINE_LONGEST and len2 > 0.25 * (the double of maxbits[b]);
 *   else 0 (MORIG_REFINE_IDLE marks nothing). image int64 = the bit pattern of len2 where mark is set, else -1.
 * morig_refine_budget: perm int64 [n_records]: the sorted positions ordered by (mesh, image descending, position ascending), rptr int64
 *   [n_meshes + 1] the records in front of every mesh (records behind rptr[n_meshes] carry INT64_MAX). mark[perm[j]] = 0 where
 *   j - rptr[b] >= budget[b]: of the marked edges of mesh b the budget[b] longest stay, ties to the lower key.
 * morig_refine_number: erank int64 the inclusive prefix sum of mark, mptr int64 [n_meshes + 1] the marked edges in front of every mesh.
 *   edge_mid int32 [n_records], set to -1 here: at every record of a marked run the new vertex, local to the mesh: (vertices of the
 *   mesh) + erank - 1 - mptr[b]. One thread walks a run, so a run may be of any length.
 * morig_refine_pattern: per face pattern int32 = its marked edges (0 .. 3; 0 at a degenerate face) and nchild int32 = 1 + pattern.
 * morig_refine_emit: crank int64 [n_faces] the inclusive prefix sum of nchild; n_out_rows = n_rows + mptr[n_meshes], n_out_faces =
 *   crank[n_faces - 1]. Output row of input row v of mesh b: v + mptr[b], with its parents; the new vertex of the marked position i:
 *   row vptr[b + 1] + erank[i] - 1 = 0.5 * (verts[lo] + verts[hi]) per coordinate with parents (lo, hi) local to the mesh. The children
 *   of face f (split_core.h children: 3 marked edges: the three corner triangles in corner order, then the centre; 1: the two triangles
 *   on the median, frame beginning at the marked edge; 2: the corner at the apex, then the quad cut by its shorter diagonal, compared by
 *   len2 on the new positions, a tie to the diagonal with the lowest vertex) stand at crank[f] - nchild, with face_map of the input face.
 * morig_refine_interpolate: values [n_rows][row_len] of elt_size 4 (float) or 8 (double), in place: row v in [row0, row1) = 0.5 *
 *   (values[p0] + values[p1]) per element in that type, parents int64 [n_rows][2]. Both parents must lie below row0 (a row with a
 *   parent outside [0, row0) is left as it is). 16 bytes per thread where row_len * elt_size is a multiple of 16 and values is aligned. */
#define MORIG_REFINE_IDLE 0
#define MORIG_REFINE_LENGTH 1
#define MORIG_REFINE_LONGEST 2
int morig_refine_edge_records(const double* verts, int32_t n_rows, const int32_t* faces, int32_t n_faces, const int32_t* fptr, const int32_t* vptr,
                              int32_t n_meshes, int64_t* keys, double* len2, int64_t* maxbits, int32_t* degenerate, int32_t* status, void* stream);
int morig_refine_mark(const int64_t* keys, const int64_t* order, const int32_t* flags, const double* len2, int64_t n_records, const int32_t* vptr,
                      int32_t n_meshes, const int32_t* mode, double limit2, const int64_t* maxbits, int32_t* mark, int64_t* image, void* stream);
int morig_refine_budget(const int64_t* perm, int64_t n_records, const int64_t* rptr, const int64_t* budget, int32_t n_meshes, int32_t* mark,
                        void* stream);
int morig_refine_number(const int64_t* keys, const int64_t* order, const int32_t* mark, const int64_t* erank, int64_t n_records, const int32_t* vptr,
                        const int64_t* mptr, int32_t n_meshes, int32_t* edge_mid, void* stream);
int morig_refine_pattern(const int32_t* edge_mid, const int32_t* degenerate, int32_t n_faces, int32_t* nchild, int32_t* pattern, void* stream);
int morig_refine_emit(const double* verts, const int64_t* parents, int32_t n_rows, const int32_t* faces, const int64_t* face_map,
                      const int32_t* edge_mid, const int64_t* crank, int32_t n_faces, const int32_t* fptr, const int32_t* vptr, const int64_t* mptr,
                      int32_t n_meshes, const int64_t* keys, const int32_t* mark, const int64_t* erank, int64_t n_records, int64_t n_out_rows,
                      int64_t n_out_faces, double* out_verts, int64_t* out_parents, int32_t* out_faces, int64_t* out_face_map, void* stream);
int morig_refine_interpolate(void* values, int32_t elt_size, int64_t row_len, const int64_t* parents, int64_t row0, int64_t row1, int64_t n_rows,
                             void* stream);

/* ---- the tolerance weld (csrc/proxweld.hip, csrc/proxweld_core.h; morig_amd/meshprep.py diagnose / clean / repair with weld_tol;
 * DESIGN.md section 32): the links between the NODES of a ragged batch -- the rows that are their own representative in the exact weld
 * (rep[v] == v) and whose three coordinates are finite -- that lie within a tolerance of each other. The rule is this product's own; no
 * parity with any mesh library exists or is claimed. Two nodes u < w of one mesh are linked when (d0 d0 + d1 d1) + d2 d2 <= eps2 with
 * d the difference of their coordinates, no fused multiply-add, the comparison not strict; eps2 below 2^-1022 (0 or subnormal) links
 * nothing. The result is DEFINED
 * by that test over all pairs of nodes of a mesh; the grid below only finds them. The conventions of the three sections above hold:
 * integers and float64 in the written order, no floating-point atomic (integer minima and maxima), plain parameters, every count at
 * most 2^31 - 257, MORIG_E_INVALID for a negative count, a count the 32-bit rows cannot hold or a null pointer, MORIG_OK for zero work
 * before anything is launched.
 * morig_proxweld_cell_keys: eps double [n_meshes] the tolerance of every mesh. box int64 [n_meshes][6], set here: the minimum and the
 *   maximum of the coordinate keys (morig_meshcheck_coord_keys) of the rows of the mesh with nonfinite = 0 (INT64_MAX / INT64_MIN where
 *   there is none). frame double [n_meshes][4], set here: the low corner of that box and the cell side h = max(eps (1 + 2^-20),
 *   largest extent / 2^20), 1 where that is 0; (0, 0, 0, h of extent 0) for a mesh without a finite row. keys int64
 *   [n_rows]: for a node cx << 42 | cy << 21 | cz with c = floor((x - low) / h) clamped to [0, 2^21 - 2]; INT64_MAX for every other row.
 * morig_proxweld_count_links: keys int64 [n_rows] the cell keys in the order (mesh, key ascending, row ascending), order int64 [n_rows]
 *   the row at every sorted position and pos double [n_rows][3] its coordinates; the positions of mesh b are [vptr[b], vptr[b + 1]).
 *   eps2 double [n_meshes]. count int32 [n_rows]: per sorted position the nodes of its mesh with a HIGHER row that it is linked to (0
 *   for a position that holds no node). One thread walks the nine key ranges of the 3 x 3 x 3 neighbourhood of its cell.
 * morig_proxweld_emit_links: the same walk; lrank int64 [n_rows] the inclusive prefix sum of count, n_links = lrank[n_rows - 1]. links
 *   int64 [n_links], set to -1 here: the links of position i at lrank[i] - count[i] in visiting order (cell x, then y, then position
 *   ascending) as row << 32 | other << 1 | 1, the edge key that morig_meshcheck_cc_round reads (which skips a negative key).
 * morig_proxweld_spread: rep int32 [n_rows] the FINAL representative of every row. maxbits int64 [n_meshes], zeroed here: the largest
 *   bit pattern of a finite squared distance (the expression above) between a finite row and its representative (integer atomic max;
 *   0 where no row moved). */
int morig_proxweld_cell_keys(const double* verts, const int32_t* nonfinite, const int32_t* rep, int32_t n_rows, const int32_t* vptr,
                             int32_t n_meshes, const double* eps, int64_t* box, double* frame, int64_t* keys, void* stream);
int morig_proxweld_count_links(const int64_t* keys, const int64_t* order, const double* pos, int32_t n_rows, const int32_t* vptr,
                               int32_t n_meshes, const double* eps2, int32_t* count, void* stream);
int morig_proxweld_emit_links(const int64_t* keys, const int64_t* order, const double* pos, int32_t n_rows, const int32_t* vptr,
                              int32_t n_meshes, const double* eps2, const int32_t* count, const int64_t* lrank, int64_t n_links,
                              int64_t* links, void* stream);
int morig_proxweld_spread(const double* verts, const int32_t* rep, const int32_t* nonfinite, int32_t n_rows, const int32_t* vptr,
                          int32_t n_meshes, int64_t* maxbits, void* stream);

/* ---- splitting non-manifold edges and pinched vertices (csrc/meshsplit.hip, csrc/fan_core.h; morig_amd/meshprep.py split_nonmanifold /
 * repair with split): every FAN of faces around a vertex gets its own copy of that vertex. The rule is this
 * product's own; no parity with any mesh library exists or is claimed. The conventions of the sections above hold: integers only,
 * integer atomics only (a minimum and an add, both order-independent), plain parameters, every count at most 2^31 - 257, MORIG_E_INVALID
 * for a negative count, a count the 32-bit rows cannot hold or a null pointer, MORIG_OK for zero work before anything is launched. The
 * input is a CLEANED batch; record 3 f + c of morig_meshfix_edge_records is the edge from corner c to corner c + 1 of face f, and the
 * NODE of corner c of face f is 3 f + c.
 * morig_meshsplit_links: keys / vals the records sorted stably by key, order int64 [n_records] the record at every sorted position
 *   (n_records at most 3 n_faces). A run of exactly two records (faces f < g) links the corners of f and g at the LOW end of the edge
 *   (its first record) and those at the HIGH end (its second record): links int64 [n_records] = a << 32 | b << 1 with a < b the two
 *   nodes, morig_meshcheck_cc_round's key layout; every other record INT64_MAX. The corner at the low end of record r with dir = 1 is
 *   r % 3, else (r % 3 + 1) % 3; the directions decide nothing else. nm int32 [n_records] = 1 at the first record of a run of three or
 *   more (a non-manifold edge), else 0. A run may be of any length and lie across any workgroup boundary.
 * morig_meshsplit_fans: lab int32 [3 n_faces] the converged labels of the nodes, tri int32 [n_faces][3] the corners as rows of the
 *   batch. A node that is its own label is a fan of its row: first int32 [n_rows] (set to INT32_MAX here) = the lowest fan of the row by
 *   integer minimum, nfans int32 [n_rows] (zeroed here) = its fans by integer add. n_faces at most (2^31 - 257) / 3.
 * morig_meshsplit_apply: rank int64 [3 n_faces] the inclusive prefix sum of the flags "node is a fan and not the first of its row", aptr
 *   int64 [n_meshes + 1] the flagged nodes in front of every mesh, n_out_rows = n_rows + aptr[n_meshes]. The corner of node t of mesh b
 *   with label l: out_faces int64 [n_faces][3] = its row local to the mesh where first[row] == l, else (rows of the mesh) + rank[l] - 1
 *   - aptr[b]. Output row of input row v of mesh b: v + aptr[b]; of a flagged fan l: vptr[b + 1] + rank[l] - 1. source int64
 *   [n_out_rows] = the input row, local to the mesh, that an output row copies; out_verts double [n_out_rows][3] = its coordinates,
 *   copied as 64-bit words (a NaN stays the NaN it was). 3 n_faces + n_rows at most 2^31 - 257. */
int morig_meshsplit_links(const int64_t* keys, const int32_t* vals, const int64_t* order, int64_t n_records, int32_t n_faces, int64_t* links,
                          int32_t* nm, void* stream);
int morig_meshsplit_fans(const int32_t* lab, const int32_t* tri, int32_t n_faces, int32_t n_rows, int32_t* first, int32_t* nfans, void* stream);
int morig_meshsplit_apply(const int32_t* lab, const int32_t* tri, const int32_t* first, const int64_t* rank, int32_t n_faces, const int32_t* fptr,
                          const int32_t* vptr, const int64_t* aptr, int32_t n_meshes, const double* verts, int32_t n_rows, int64_t n_out_rows,
                          int64_t* out_faces, int64_t* source, double* out_verts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MORIG_HIP_H */
