// Which kernel a morig_gemm / morig_edgeconv / morig_edge_hidden / morig_segmax_gemm / morig_edgeconv_x3 call runs, as pure host code:
// the environment switches in one struct, one plan function per entry point, one table of the tile engine's instantiations.
// No HIP header, no launch, no environment read: tile_gemm.hip / gemm_dma.hip launch what a plan names, and
// tools/dispatch_host_check.cpp enumerates the plans as a plain program under the sanitizers (tests/test_dispatch_host.py).
#pragma once
#include <stdint.h>
#include "../../include/morig_hip.h"

namespace morig {

// profiling kinds (index into the live event accounting; names in prof.hip). They live here because a plan names them.
enum Kind : int {
    K_GEMM_BN128 = 0, K_GEMM_BN64, K_GEMM_BN32, K_GEMM_POOL,
    K_EDGE_H16, K_EDGE_H32, K_EDGE_H64, K_EDGE_H128, K_EDGE_H256,
    K_CSR, K_COPY, K_ROWNORM, K_ATTN, K_MISC,
    K_FPS, K_BALL, K_POINTCONV, K_KNN_INTERP, K_COSINE_NN,
    K_GEMM16_BN128, K_GEMM16_BN64, K_GEMM16_BN32, K_GEMM16_POOL,
    K_EDGE16_H32, K_EDGE16_H64, K_EDGE16_H128, K_EDGE16_H256, K_POINTCONV16, K_GEMM16_DMA,
    K_COSINE_KNN, K_FLOW_VOTE, K_JOINTS,
    K_GEMM16_DMAP, K_GEMM16_DMA128, K_EDGE16_H256_PP, K_EDGE16_H128_WS, K_EDGE16_PC, K_GEOGRAPH, K_EDGE16_X3, K_EDGE_X3, K_EDGE16_X3P, K_EDGE16_H128_RL,
    K_LOSS_NCE_FWD, K_LOSS_NCE_BWD, K_LOSS_MULTIPOS, K_LOSS_CHAMFER, K_LOSS_REDUCE,
    K_LOSS_LOGRATIO, K_LOSS_SKIN_CE,
    K_METRICS,
    K_RIG_ASSEMBLE, K_RIG_ENTRIES,
    K_RANSAC_VOTE, K_RANSAC_FIT, K_RANSAC_APPLY, K_KMEANS,
    K_MESH_PREP, K_VOXEL_SURFACE, K_VOXEL_FILL,
    K_POSE_PREP, K_POSE_SKIN, K_POSE_ERRORS,
    K_SCAN_RASTER, K_SCAN,
    K_SIMPLIFY_KEYS, K_SIMPLIFY_QUADRICS,
    K_RAY_CAST, K_RAY_SELECT, K_RAY_ATTENTION,
    K_TRANSFER_PAIRS, K_TRANSFER_FLOOD, K_TRANSFER_ROWS,
    K_BVH_BUILD, K_BVH_QUERY,
    K_MESHCHECK_WELD, K_MESHCHECK_FACES, K_MESHCHECK_EDGES, K_MESHCHECK_COMPONENTS, K_MESHCHECK_COMPACT,
    K_MESHFIX_ORIENT, K_MESHFIX_LOOPS, K_MESHFIX_FILL,
    K_REFINE_EDGES, K_REFINE_EMIT, K_REFINE_INTERPOLATE,
    K_PROXWELD_KEYS, K_PROXWELD_LINKS, K_PROXWELD_SPREAD,
    K_MESHSPLIT_LINKS, K_MESHSPLIT_APPLY,
    K_COUNT
};
static_assert(K_COUNT <= MORIG_PROF_KINDS, "raise MORIG_PROF_KINDS");

// ---- the environment switches ------------------------------------------------------------------------------------------------------
// Every MORIG_* variable the GEMM / EdgeConv launch path reads, each with its parse rule. The library's switches() (prof.hip) reads
// them ONCE per process, except MORIG_NO_DMA, which every morig_gemm call reads again, and MORIG_NO_EDGE_PC, which every morig_edgeconv
// call reads again (gemm_switches() / edge_switches(): they can be set between two launches of one process). "set" = the variable
// exists, whatever its value.
struct Switches {
    bool no_dma = false;            // MORIG_NO_DMA set: pre-split GEMMs stay on the tile engine                       (every call)
    bool no_edge_pc = false;        // MORIG_NO_EDGE_PC set: H = 128 / 256 EdgeConvs stay on the tile engine           (every call)
    bool tile_no_fast = false;      // MORIG_TILE_NO_FAST set: no guard-free FAST form of the dense store tile
    bool no_few_rows = false;       // MORIG_NO_FEW_ROWS set: no few-rows GEMM (vertex_ops.hip)
    int edge_kernel = 0;            // MORIG_EDGE_KERNEL=pp|pc: the older wide EdgeConv kernels (EK_PP / EK_PC)
    bool rl128 = true;              // MORIG_RL128=0: H = 128 on a 4-aligned CSR keeps the generic kernels, not edge_rl.hip
    bool edge_mix = true;           // MORIG_EDGE_MIX=0: a MIN4 CSR takes the generic kernels
    int edge_run = 8;               // MORIG_EDGE_RUN=<tiles>, 1 .. 4096: longest run of tiles that carries open segments
    bool edge_split_out = true;     // MORIG_EDGE_SPLIT_OUT=0: no EdgeConv stores split rows
    bool x3_tile = false;           // MORIG_X3_TILE=1: the 32-wide EdgeConvs stay on the tile engine
    int dma_tile = 256;             // MORIG_DMA_TILE=<n>: anything but 256 sends every LDS-DMA GEMM to the 128 x 128 kernel
    int dma_persist = 1;            // MORIG_DMA_PERSIST=0 never / anything else always (2); unset: the deep, wide launches only (1)
    int dma_small_tiles = 256;      // MORIG_DMA_SMALL_TILES=<n>: launches of at most n 256 x 256 tiles take the 128 x 128 kernel
    bool gemm_tr = true;            // MORIG_GEMM_TR=0: the 256 x 256 store kernel keeps the LDS-transposition epilogue
    int pool_run = 0;               // MORIG_POOL_RUN=<R>, 0 .. 256: forced run length of the pooled persistent GEMM (0 = automatic)
    int debug_flags = 0;            // MORIG_DEBUG_FLAGS: ablation switches for tools/microbench.py (0 in production)

    enum { EK_DEFAULT = 0, EK_PP = 1, EK_PC = 2 };

    static int to_int(const char* e) {          // atoi: blanks, a sign, digits
        while (*e == ' ' || (*e >= '\t' && *e <= '\r')) ++e;
        const bool neg = *e == '-';
        if (*e == '-' || *e == '+') ++e;
        long v = 0;
        for (; *e >= '0' && *e <= '9' && v < (1L << 40); ++e) v = v * 10 + (*e - '0');
        if (v > 0x7fffffffL) v = 0x7fffffffL;
        return (int)(neg ? -v : v);
    }
    static int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

    // get(name) -> value or nullptr, as getenv
    template <class Get> static Switches from(Get&& get) {
        Switches s;
        auto set = [&](const char* n) { return get(n) != nullptr; };
        auto is = [&](const char* n, char c) { const char* e = get(n); return e && e[0] == c; };
        auto num = [&](const char* n, int dflt) { const char* e = get(n); return e ? to_int(e) : dflt; };
        s.no_dma = set("MORIG_NO_DMA");
        s.no_edge_pc = set("MORIG_NO_EDGE_PC");
        s.tile_no_fast = set("MORIG_TILE_NO_FAST");
        s.no_few_rows = set("MORIG_NO_FEW_ROWS");
        if (const char* ek = get("MORIG_EDGE_KERNEL")) s.edge_kernel = ek[0] != 'p' ? EK_DEFAULT : (ek[1] == 'p' ? EK_PP : (ek[1] == 'c' ? EK_PC : EK_DEFAULT));
        s.rl128 = !is("MORIG_RL128", '0');
        s.edge_mix = !is("MORIG_EDGE_MIX", '0');
        s.edge_run = clamp(num("MORIG_EDGE_RUN", 8), 1, 4096);
        s.edge_split_out = !is("MORIG_EDGE_SPLIT_OUT", '0');
        s.x3_tile = is("MORIG_X3_TILE", '1');
        s.dma_tile = num("MORIG_DMA_TILE", 256);
        if (const char* e = get("MORIG_DMA_PERSIST")) s.dma_persist = e[0] == '0' ? 0 : 2;
        s.dma_small_tiles = num("MORIG_DMA_SMALL_TILES", 256);
        s.gemm_tr = !is("MORIG_GEMM_TR", '0');
        s.pool_run = clamp(num("MORIG_POOL_RUN", 0), 0, 256);
        s.debug_flags = num("MORIG_DEBUG_FLAGS", 0);
        return s;
    }
};

// ---- the tile engine's instantiations (tile_gemm.hip: tile_kernel<BN, KC, LOAD, MODE, PREC, FAST>) ------------------------------------
enum { PREC_F32 = 0, PREC_F16X3 = 1, PREC_BF16X3 = 2, PREC_BF16X6 = 3 };   // arithmetic (tile_gemm.hip describes each)
enum { LOAD_DENSE = 0, LOAD_EDGE = 1, LOAD_EDGE3 = 2 };                    // how the row operand is produced
enum { MODE_STORE = 0, MODE_POOL = 1, MODE_EDGEMAX = 2 };                  // how the accumulator tile is consumed

// THE list: every (BN, KC, LOAD, MODE, PREC) that is compiled. The launcher switches over it, the host check walks it. The FAST form
// exists for the entries tile_has_fast() names and is no row of its own.
#define MORIG_TILE_TABLE(X)                                                                                                    \
    /* dense stores (morig_gemm) */                                                                                            \
    X(128, 32, LOAD_DENSE, MODE_STORE, PREC_F32)     X(64, 32, LOAD_DENSE, MODE_STORE, PREC_F32)     X(32, 32, LOAD_DENSE, MODE_STORE, PREC_F32)     \
    X(128, 32, LOAD_DENSE, MODE_STORE, PREC_F16X3)   X(64, 32, LOAD_DENSE, MODE_STORE, PREC_F16X3)   X(32, 32, LOAD_DENSE, MODE_STORE, PREC_F16X3)   \
    X(128, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X3)  X(64, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X3)  X(32, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X3)  \
    X(128, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X6)  X(64, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X6)  X(32, 32, LOAD_DENSE, MODE_STORE, PREC_BF16X6)  \
    /* pooled (morig_gemm with pool) */                                                                                        \
    X(128, 32, LOAD_DENSE, MODE_POOL, PREC_F32)      X(128, 32, LOAD_DENSE, MODE_POOL, PREC_F16X3)   X(128, 32, LOAD_DENSE, MODE_POOL, PREC_BF16X6)  \
    /* segmented max over per-edge rows (morig_segmax_gemm) */                                                                 \
    X(32, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F32)    X(64, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F32)                             \
    X(128, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F32)   X(256, 16, LOAD_DENSE, MODE_EDGEMAX, PREC_F32)                            \
    X(32, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F16X3)  X(64, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F16X3)                           \
    X(128, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F16X3) X(256, 32, LOAD_DENSE, MODE_EDGEMAX, PREC_F16X3)                          \
    /* per-edge hidden rows (morig_edge_hidden) */                                                                             \
    X(32, 16, LOAD_EDGE, MODE_STORE, PREC_F32)       X(32, 32, LOAD_EDGE, MODE_STORE, PREC_F32)      X(64, 32, LOAD_EDGE, MODE_STORE, PREC_F32)      \
    X(128, 32, LOAD_EDGE, MODE_STORE, PREC_F32)      X(256, 16, LOAD_EDGE, MODE_STORE, PREC_F32)                               \
    X(32, 32, LOAD_EDGE, MODE_STORE, PREC_F16X3)     X(64, 32, LOAD_EDGE, MODE_STORE, PREC_F16X3)                              \
    X(128, 32, LOAD_EDGE, MODE_STORE, PREC_F16X3)    X(256, 32, LOAD_EDGE, MODE_STORE, PREC_F16X3)                             \
    X(32, 32, LOAD_EDGE, MODE_STORE, PREC_BF16X6)    X(64, 32, LOAD_EDGE, MODE_STORE, PREC_BF16X6)                             \
    X(128, 32, LOAD_EDGE, MODE_STORE, PREC_BF16X6)   X(256, 32, LOAD_EDGE, MODE_STORE, PREC_BF16X6)                            \
    /* fused EdgeConv (morig_edgeconv) */                                                                                      \
    X(32, 16, LOAD_EDGE, MODE_EDGEMAX, PREC_F32)     X(32, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F32)    X(64, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F32)    \
    X(128, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F32)    X(256, 16, LOAD_EDGE, MODE_EDGEMAX, PREC_F32)                             \
    X(32, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F16X3)   X(64, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F16X3)                            \
    X(128, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F16X3)  X(256, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_F16X3)                           \
    X(32, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_BF16X6)  X(64, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_BF16X6)                           \
    X(128, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_BF16X6) X(256, 32, LOAD_EDGE, MODE_EDGEMAX, PREC_BF16X6)                          \
    /* EdgeConv on 3-channel inputs (morig_edgeconv_x3) */                                                                     \
    X(32, 32, LOAD_EDGE3, MODE_EDGEMAX, PREC_F32)    X(32, 32, LOAD_EDGE3, MODE_EDGEMAX, PREC_F16X3)

struct TileInst { int BN, KC, LOAD, MODE, PREC; bool fast; };
constexpr int tile_key(int BN, int KC, int LOAD, int MODE, int PREC) { return BN | (KC << 10) | (LOAD << 17) | (MODE << 19) | (PREC << 21); }
constexpr int tile_key(const TileInst& t) { return tile_key(t.BN, t.KC, t.LOAD, t.MODE, t.PREC); }
// the guard-free FAST form (every row of every tile exists, K a multiple of KC, no debug switch): the 128-wide dense stores only
constexpr bool tile_has_fast(int BN, int KC, int LOAD, int MODE) { return BN == 128 && KC == 32 && LOAD == LOAD_DENSE && MODE == MODE_STORE; }
// row of the table, -1: no such instantiation
inline int tile_table_index(const TileInst& t) {
    int i = 0;
#define MORIG_TILE_ROW(BN, KC, LOAD, MODE, PREC) if (tile_key(t) == tile_key(BN, KC, LOAD, MODE, PREC)) return i; ++i;
    MORIG_TILE_TABLE(MORIG_TILE_ROW)
#undef MORIG_TILE_ROW
    return -1;
}
inline int tile_table_size() {
    int n = 0;
#define MORIG_TILE_ROW(BN, KC, LOAD, MODE, PREC) ++n;
    MORIG_TILE_TABLE(MORIG_TILE_ROW)
#undef MORIG_TILE_ROW
    return n;
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

namespace plan_detail {
inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool aligned16(const void* p) { return !misaligned(p, 15); }
// the width ladder, once: the tile instantiation for an output width that is already one of the library's (16 only in fp32, where the
// bf16 x 6 request falls back to it; 256 in fp32 on 16-deep chunks). false: no such width
inline bool tile_for_width(int width, int load, int mode, int prec, TileInst& t) {
    if (width == 16 && (prec == PREC_F32 || prec == PREC_BF16X6) && load == LOAD_EDGE) { t = TileInst{32, 16, load, mode, PREC_F32, false}; return true; }
    if (width != 32 && width != 64 && width != 128 && width != 256) return false;
    t = TileInst{width, (width == 256 && prec == PREC_F32) ? 16 : 32, load, mode, prec, false};
    return true;
}
}  // namespace plan_detail

// ---- morig_gemm --------------------------------------------------------------------------------------------------------------------
enum GemmEngine {
    GEMM_NONE = 0,        // M == 0, or a refusal: nothing is launched
    GEMM_FEW_ROWS,        // vertex_ops.hip few_rows_gemm_kernel: at most 128 rows, weights spread over the chip
    GEMM_TILE,            // tile_gemm.hip, plan.tile
    GEMM_DMA128,          // gemm_dma.hip gemm16_dma_kernel<128, 128, 2, 2, false>
    GEMM_DMA256,          // gemm_dma.hip gemm16_dma_kernel<256, 256, 4, 2, tr, tail>
    GEMM_DMAP,            // gemm_dmap.hip gemm16_dmap_kernel<pool>: persistent, 256 x 256 tiles
};
struct GemmPlan {
    int status;           // MORIG_OK, or what the call returns
    int engine;
    TileInst tile;        // GEMM_TILE
    bool tr, tail;        // GEMM_DMA256: register epilogue (else LDS transposition) / K tail from X_tail
    int tiles_n;          // column tiles of the engine's tile width
    int blocks;           // workgroups; GEMM_DMAP: tiles (its grid follows the device's CU count)
    int kind, retag;      // the ProfScope kind, and the kind the launch is re-labelled with (-1: none)
};

inline bool few_rows_takes(int M, int N, int K, int ldx, int ldw, const Switches& sw) {
    return !sw.no_few_rows && M <= 128 && N >= 128 && K >= 128 && K <= 1024 && (K & 3) == 0 && (ldx & 3) == 0 && (ldw & 3) == 0;
}

inline GemmPlan gemm_plan(const morig_gemm_args& a, const Switches& sw) {
    using namespace plan_detail;
    GemmPlan pl = {};
    pl.retag = -1;
    auto refuse = [&](int st) { pl.status = st; pl.engine = GEMM_NONE; return pl; };
    if (!a.X || !a.W) return refuse(MORIG_E_INVALID);
    if (a.M < 0 || a.N <= 0 || a.K <= 0) return refuse(MORIG_E_INVALID);
    if (a.M == 0) return pl;
    if ((a.ldx & 3) || (a.ldw & 3) || !aligned16(a.X) || !aligned16(a.W)) return refuse(MORIG_E_INVALID);
    const bool tail = a.X_tail != nullptr;
    // K tail: split chunks from X_tail[row % tail_rows] (include/morig_hip.h); everything about it is checked here, the kernel choice below
    if (tail && (!a.x_split || !a.W_split || a.tail_cols <= 0 || (a.tail_cols & 31) || (a.K & 31) || a.K <= a.tail_cols || a.tail_rows <= 0 ||
                 (a.ld_tail & 31) || a.ld_tail < a.tail_cols || misaligned(a.X_tail, 127) ||
                 (double)a.tail_rows * a.ld_tail * 4.0 >= 4.0e9)) return refuse(MORIG_E_INVALID);
    const int k_own = a.K - (tail ? a.tail_cols : 0);                  // columns X itself holds
    if (a.ldx < ((k_own + 3) & ~3) || a.ldw < ((a.K + 31) & ~31)) return refuse(MORIG_E_INVALID);
    const bool pool = a.pool != nullptr;
    if (tail && pool) return refuse(MORIG_E_UNSUPPORTED);
    if (!pool && !a.Y) return refuse(MORIG_E_INVALID);
    if (pool && a.Y) return refuse(MORIG_E_UNSUPPORTED);               // one consumer per launch
    if ((pool || a.rowbias) && !a.seg) return refuse(MORIG_E_INVALID);
    // MORIG_SPLIT_BF16X6 without an image: the exact path on three bf16 limbs per operand (split in the kernel)
    const bool x6 = a.W_split == nullptr && a.w_split_format == MORIG_SPLIT_BF16X6;
    if (x6 && (a.x_split || a.y_split)) return refuse(MORIG_E_INVALID);
    const bool f16 = a.W_split != nullptr;
    // the bf16 split is selected by w_split_format, never inferred from a missing overflow word: a caller that forgets the word on an
    // fp16 image gets MORIG_E_INVALID, not silently unguarded results
    if (f16 && a.w_split_format != MORIG_SPLIT_F16 && a.w_split_format != MORIG_SPLIT_BF16) return refuse(MORIG_E_INVALID);
    const bool bf16 = f16 && a.w_split_format == MORIG_SPLIT_BF16;
    if (f16 && !bf16 && a.overflow == nullptr) return refuse(MORIG_E_INVALID);
    if (f16 && !aligned16(a.W_split)) return refuse(MORIG_E_INVALID);
    if (bf16 && (pool || a.x_split || a.y_split)) return refuse(MORIG_E_UNSUPPORTED);
    if (a.x_split || a.y_split) {
        if (!f16) return refuse(MORIG_E_INVALID);                      // split activations only exist on the split-fp16 path
        if (a.x_split && ((a.ldx & 31) || a.ldx < ((k_own + 31) & ~31) || misaligned(a.X, 127))) return refuse(MORIG_E_INVALID);
        if (a.y_split && (pool || (a.ldy & 31) || misaligned(a.Y, 127))) return refuse(MORIG_E_INVALID);
    }
    if (pool && (a.n_seg <= 0 || a.ld_pool < a.N)) return refuse(MORIG_E_INVALID);

    const int tiles_m = cdiv(a.M, 128);
    if (f16 && a.x_split && a.N > 64 && !sw.no_dma) {
        // both operands pre-split: the LDS-DMA pipeline (gemm_dma.hip; a pooled launch needs `seg` sorted within the matrix)
        pl.kind = pool ? K_GEMM16_POOL : K_GEMM16_DMA;
        const bool by256 = sw.dma_tile == 256 && a.N % 256 == 0;
        if (tail && !by256) return refuse(MORIG_E_UNSUPPORTED);        // K tails: the 256 x 256 store kernel only
        const int tiles256 = by256 ? cdiv(a.M, 256) * (a.N / 256) : 0;
        // few rows (one to four meshes per launch): at most dma_small_tiles 256 x 256 tiles leave CUs idle -- the 128 x 128 kernel makes
        // four times as many workgroups of the launch, two per CU
        const bool few_tiles = !tail && a.N % 256 == 0 && (long)cdiv(a.M, 256) * (a.N / 256) <= sw.dma_small_tiles;
        // register epilogue: 16-byte vector stores to Y, 16-byte loads of rowbias
        const bool vec_ok = !pool && aligned16(a.Y) && (a.ldy & 3) == 0 && (!a.rowbias || (aligned16(a.rowbias) && (a.ld_rowbias & 3) == 0));
        // the persistent kernel takes the pooled launches and the deep, wide stores only (MORIG_DMA_PERSIST forces never / always);
        // its store form has only the register epilogue
        const bool deep_wide = pool || (a.K >= 768 && a.N >= 1024);
        if (by256 && !few_tiles && !tail && a.K > 32 && (pool || vec_ok) && (sw.dma_persist == 2 || (sw.dma_persist == 1 && deep_wide))) {
            pl.engine = GEMM_DMAP; pl.tr = !pool; pl.tiles_n = a.N / 256; pl.blocks = tiles256;
            if (!pool) pl.retag = K_GEMM16_DMAP;                       // the pooled kind already names this kernel
            return pl;
        }
        if (by256 && !few_tiles) {
            pl.engine = GEMM_DMA256; pl.tr = sw.gemm_tr && vec_ok; pl.tail = tail; pl.tiles_n = a.N / 256; pl.blocks = tiles256;
            if (tail && !pl.tr) return refuse(MORIG_E_UNSUPPORTED);
            return pl;
        }
        pl.engine = GEMM_DMA128; pl.tiles_n = cdiv(a.N, 128); pl.blocks = tiles_m * pl.tiles_n; pl.retag = K_GEMM16_DMA128;
        return pl;
    }
    if (tail) return refuse(MORIG_E_UNSUPPORTED);
    const int prec = bf16 ? PREC_BF16X3 : x6 ? PREC_BF16X6 : f16 ? PREC_F16X3 : PREC_F32;
    pl.engine = GEMM_TILE;
    if (pool) {
        pl.tile = TileInst{128, 32, LOAD_DENSE, MODE_POOL, prec, false};
        pl.tiles_n = cdiv(a.N, 128); pl.blocks = tiles_m * pl.tiles_n;
        pl.kind = f16 ? K_GEMM16_POOL : K_GEMM_POOL;
        return pl;
    }
    // a few rows (per-mesh vectors): weights spread over the chip, plain fp32 FMAs; W is the fp32 matrix on every path, so the fast
    // and the exact mode run the same kernel here
    if (!bf16 && !a.rowbias && !a.x_split && !a.y_split && few_rows_takes(a.M, a.N, a.K, a.ldx, a.ldw, sw)) {
        pl.engine = GEMM_FEW_ROWS; pl.kind = K_MISC; pl.tiles_n = cdiv(a.N, 4); pl.blocks = pl.tiles_n;
        return pl;
    }
    const int BN = a.N > 64 ? 128 : (a.N > 32 ? 64 : 32);
    pl.tile = TileInst{BN, 32, LOAD_DENSE, MODE_STORE, prec, false};
    // fp32 X on the split-fp16 path stays on 32-deep chunks: 3 workgroups per CU beat a 64-deep form at 2 per CU by ~20 % (measured)
    pl.tile.fast = BN == 128 && sw.debug_flags == 0 && !sw.tile_no_fast && a.M % 128 == 0 && a.K % 32 == 0;
    pl.tiles_n = BN == 128 ? cdiv(a.N, 128) : 1;
    pl.blocks = tiles_m * pl.tiles_n;
    pl.kind = bf16 ? K_MISC : (f16 ? K_GEMM16_BN128 : K_GEMM_BN128) + (BN == 128 ? 0 : BN == 64 ? 1 : 2);
    return pl;
}

// ---- morig_edgeconv, morig_edge_hidden, morig_segmax_gemm, morig_edgeconv_x3 ---------------------------------------------------------
enum EdgeEngine {
    EDGE_NONE = 0,        // a refusal
    EDGE_TILE,            // tile_gemm.hip, plan.tile
    EDGE_RL,              // edge_rl.hip: H = 128, 4-aligned CSR, W2 resident in LDS, 64-row tiles
    EDGE_WS,              // edge_ws.hip: H = 256, 4-aligned CSR, W2 resident in registers, 64-row tiles
    EDGE_WS_MIX,          // edge_ws.hip's mixed-quad form: H = 256, MIN4 CSR, split rows only
    EDGE_PP,              // edge_pp.hip: H = 128 / 256, persistent producer-consumer
    EDGE_PC,              // edge_pc.hip: H = 128 / 256, one tile per workgroup (any output alignment)
    EDGE_X3,              // edge_x3.hip: persistent 32-wide kernel (3-channel inputs, or gathered [A | B] rows)
};
struct EdgePlan {
    int status;           // MORIG_OK, or what the call returns
    bool late;            // morig_edgeconv: the refusal stands BEHIND the checks of an init_with partner, and does not count where the
                          // call is looked at as a partner itself (the order in which the codes have always been returned)
    int engine;
    TileInst tile;        // EDGE_TILE
    int tile_rows, run;   // rows of a tile; consecutive tiles that carry an open segment (only rows that straddle a run are shared)
    bool split_ok;        // morig_edgeconv: out_split would be honoured (morig_edgeconv_can_split_out)
    int blocks;           // workgroups (tile engine, PC) / tiles of tile_rows rows (the persistent kernels size their own grid)
    int kind, retag;      // as GemmPlan
};
inline bool edge_splits(const EdgePlan& pl) { return pl.engine == EDGE_RL || pl.engine == EDGE_WS || pl.engine == EDGE_WS_MIX; }

// the argument checks morig_edgeconv, morig_edge_hidden and morig_edgeconv_can_split_out share
inline int edge_args_status(const morig_edgeconv_args& a) {
    using namespace plan_detail;
    if (!a.A || !a.B || !a.rowptr || !a.src_sorted || !a.dst_sorted || !a.W2 || !a.out) return MORIG_E_INVALID;
    if ((a.s1 == nullptr) != (a.t1 == nullptr) || !a.b2 || !a.s2 || !a.t2) return MORIG_E_INVALID;
    if (a.n_nodes <= 0 || a.replicas <= 0 || a.edge_capacity <= 0) return MORIG_E_INVALID;
    if ((a.lda & 3) || (a.ldb & 3) || (a.ldw & 3) || !aligned16(a.A) || !aligned16(a.B) || !aligned16(a.W2) ||
        !aligned16(a.s1) || !aligned16(a.t1)) return MORIG_E_INVALID;
    if (a.ldo < a.H || a.lda < a.H || a.ldb < a.H || a.ldw < a.H) return MORIG_E_INVALID;
    if (a.W2_split && (!a.overflow || !aligned16(a.W2_split) || a.H < 32)) return MORIG_E_INVALID;
    return MORIG_OK;
}

// morig_edgeconv. H = 256 / 128 on the split-fp16 path with the hidden affine folded go to the specialised kernels: with a 4-aligned CSR
// the row-local one (H = 128) or the W2-stationary one (H = 256), whose tiles are 64 rows; MORIG_EDGE_KERNEL=pp|pc keeps the older ones.
// `args_only`: morig_edgeconv_can_split_out's view -- the shared argument checks, then the kernel choice; out_split is not looked at.
inline EdgePlan edge_plan(const morig_edgeconv_args& a, const Switches& sw, bool args_only = false) {
    using namespace plan_detail;
    EdgePlan pl = {};
    pl.retag = -1; pl.tile_rows = 128; pl.run = 1;
    // (a late refusal keeps the engine: the partner checks of a paired pass look at it, not at the partner's own flags)
    auto refuse = [&](int st, bool late) { pl.status = st; pl.late = late; if (!late) { pl.engine = EDGE_NONE; pl.split_ok = false; } return pl; };
    if (const int st = edge_args_status(a)) return refuse(st, false);
    if (!args_only && (a.in_rep_stride < 0 || (a.replicas > 1 && a.out_rep_stride < a.n_nodes))) return refuse(MORIG_E_INVALID, false);
    const bool f16 = a.W2_split != nullptr;
    const int tiles128 = cdiv(a.edge_capacity, 128) * a.replicas;
    const bool wide = f16 && (a.H == 256 || a.H == 128) && a.s1 == nullptr && !sw.no_edge_pc;
    // the persistent kernels store 16-byte result vectors and address gathered rows with 32-bit byte offsets
    const bool pp_ok = aligned16(a.out) && (a.ldo & 3) == 0 && (double)a.n_nodes * a.lda * 4.0 < 4.0e9 && (double)a.n_nodes * a.ldb * 4.0 < 4.0e9;
    const bool newer = wide && sw.edge_kernel == Switches::EK_DEFAULT && pp_ok;
    // H = 128 with a 4-aligned CSR: edge_rl.hip (MORIG_RL128=0: the producer-consumer kernel, which measured on par with / ahead of a
    // W2-stationary form at this width); H = 256: edge_ws.hip
    const bool quad_ok = newer && a.quad_aligned;
    // H = 256 on a MIN4 CSR (segments of >= 4 rows, NOT 4-aligned): the mixed-quad form of edge_ws.hip, which exists for split rows only
    const bool mix = newer && !a.quad_aligned && a.seg_min4 && a.H == 256 && sw.edge_mix;
    if (quad_ok && a.H == 128 && sw.rl128) pl.engine = EDGE_RL;
    else if (quad_ok && a.H == 256) pl.engine = EDGE_WS;
    else if (mix && a.out_split) pl.engine = EDGE_WS_MIX;
    else if (wide) pl.engine = (sw.edge_kernel == Switches::EK_PC || !pp_ok) ? EDGE_PC : EDGE_PP;
    if (edge_splits(pl)) {
        pl.tile_rows = 64;
        pl.blocks = cdiv(a.edge_capacity, 64) * a.replicas;
        // these kernels carry a segment that is still open at the end of a tile into the next tile of the same RUN of consecutive tiles
        // (edge_ws.hip in its split-rows form only). Measured (profiles/r05n_*): runs of 4 .. 8 tiles gain 0.5 % of the step over 1, 16
        // and more lose to the coarser work split -- so at most edge_run, and short enough that every wave (edge_rl.hip, 8 per CU) /
        // workgroup (edge_ws.hip) still gets >= 16 runs
        if (pl.engine == EDGE_RL || a.out_split) {
            const long units = pl.engine == EDGE_RL ? 2048 : 256;
            while (pl.run * 2 <= sw.edge_run && pl.blocks / (units * 16) >= pl.run * 2) pl.run *= 2;
        }
    }
    // split-fp16 results: the three kernels above, chunk-aligned output window
    pl.split_ok = (edge_splits(pl) || mix) && sw.edge_split_out && a.overflow != nullptr && (a.ldo & 31) == 0 && !misaligned(a.out, 127);
    if (args_only) return pl;
    if (a.out_split && !pl.split_ok) return refuse(MORIG_E_UNSUPPORTED, false);
    if (a.skip_init && a.init_with) return refuse(MORIG_E_INVALID, true);
    // only the split-rows kernels have a conversion pass to share
    if ((a.split_with || a.skip_split) && !(edge_splits(pl) && a.out_split && !(a.split_with && a.skip_split))) return refuse(MORIG_E_INVALID, true);
    if (wide) {
        pl.kind = a.H == 256 ? K_EDGE16_H256 : K_EDGE16_H128;
        if (pl.engine == EDGE_RL) pl.retag = K_EDGE16_H128_RL;
        else if (pl.engine == EDGE_PC) { pl.retag = K_EDGE16_PC; pl.blocks = tiles128; }
        else if (pl.engine == EDGE_PP) { if (a.H == 256) pl.retag = K_EDGE16_H256_PP; pl.blocks = tiles128; }
        return pl;
    }
    pl.blocks = tiles128;
    // H = 32 on the split-fp16 path with the hidden BatchNorm folded (packing.fold_hidden_affine: every pack of the networks): the
    // persistent 32-wide kernel with gathered [A | B] rows
    if (f16 && a.H == 32 && !a.s1 && !sw.x3_tile && (a.ldo & 3) == 0 && aligned16(a.out) && (a.lda & 3) == 0 && (a.ldb & 3) == 0 &&
        aligned16(a.b2) && a.ldw >= 32) {
        pl.engine = EDGE_X3; pl.kind = K_EDGE16_H32;
        return pl;
    }
    const int prec = f16 ? PREC_F16X3 : (a.exact_arith == 1 ? PREC_BF16X6 : PREC_F32);
    if (!tile_for_width(a.H, LOAD_EDGE, MODE_EDGEMAX, prec, pl.tile)) return refuse(MORIG_E_UNSUPPORTED, true);
    pl.engine = EDGE_TILE;
    const int rung = a.H == 16 ? 0 : a.H == 32 ? 1 : a.H == 64 ? 2 : a.H == 128 ? 3 : 4;
    pl.kind = f16 ? K_EDGE16_H32 + rung - 1 : K_EDGE_H16 + rung;
    return pl;
}

// morig_edge_hidden: the per-edge hidden rows of a PointConv, always on the tile engine
inline EdgePlan edge_hidden_plan(const morig_edgeconv_args& a, const Switches&) {
    using namespace plan_detail;
    EdgePlan pl = {};
    pl.retag = -1; pl.tile_rows = 128; pl.run = 1;
    auto refuse = [&](int st) { pl.status = st; return pl; };
    if (const int st = edge_args_status(a)) return refuse(st);
    if (a.replicas != 1 || a.out_split) return refuse(MORIG_E_UNSUPPORTED);
    const bool f16 = a.W2_split != nullptr;
    const int prec = f16 ? PREC_F16X3 : (a.exact_arith == 1 ? PREC_BF16X6 : PREC_F32);
    if (!tile_for_width(a.H, LOAD_EDGE, MODE_STORE, prec, pl.tile)) return refuse(MORIG_E_UNSUPPORTED);
    pl.engine = EDGE_TILE; pl.blocks = cdiv(a.edge_capacity, 128);
    pl.kind = f16 ? K_POINTCONV16 : K_POINTCONV;
    return pl;
}

// morig_segmax_gemm: a dense layer on per-edge rows with a segmented max, on the tile engine at the next width of the ladder
inline EdgePlan segmax_plan(const morig_segmax_args& a, const Switches&) {
    using namespace plan_detail;
    EdgePlan pl = {};
    pl.retag = -1; pl.tile_rows = 128; pl.run = 1;
    auto refuse = [&](int st) { pl.status = st; return pl; };
    if (!a.X || !a.W || !a.rowptr || !a.dst_sorted || !a.out) return refuse(MORIG_E_INVALID);
    if (a.N <= 0 || a.K <= 0 || a.n_nodes <= 0 || a.edge_capacity <= 0) return refuse(MORIG_E_INVALID);
    if ((a.ldx & 3) || (a.ldw & 3) || !aligned16(a.X) || !aligned16(a.W)) return refuse(MORIG_E_INVALID);
    if (a.ldx < ((a.K + 3) & ~3) || a.ldw < ((a.K + 31) & ~31) || a.ldo < a.N) return refuse(MORIG_E_INVALID);
    const bool f16 = a.W_split != nullptr;
    if (f16 && (!a.overflow || !aligned16(a.W_split))) return refuse(MORIG_E_INVALID);
    const int width = a.N <= 32 ? 32 : a.N <= 64 ? 64 : a.N <= 128 ? 128 : a.N <= 256 ? 256 : 0;
    if (!tile_for_width(width, LOAD_DENSE, MODE_EDGEMAX, f16 ? PREC_F16X3 : PREC_F32, pl.tile)) return refuse(MORIG_E_UNSUPPORTED);
    pl.engine = EDGE_TILE; pl.blocks = cdiv(a.edge_capacity, 128);
    pl.kind = f16 ? K_POINTCONV16 : K_POINTCONV;
    return pl;
}

// morig_edgeconv_x3: split-fp16 launches take the persistent kernel (MORIG_X3_TILE=1 keeps the one-tile-per-workgroup engine); the exact
// path (MORIG_PRECISION=f32, or the re-run after a range overflow) stays on the tile engine
inline EdgePlan edgeconv_x3_plan(const morig_edgeconv_x3_args& a, const Switches& sw) {
    using namespace plan_detail;
    EdgePlan pl = {};
    pl.retag = -1; pl.tile_rows = 128; pl.run = 1;
    auto refuse = [&](int st) { pl.status = st; return pl; };
    if (!a.X || !a.W1a || !a.W1b || !a.b1 || !a.rowptr || !a.src_sorted || !a.dst_sorted || !a.W2 || !a.out) return refuse(MORIG_E_INVALID);
    if (!a.b2 || !a.s2 || !a.t2) return refuse(MORIG_E_INVALID);
    if (a.H != 32) return refuse(MORIG_E_UNSUPPORTED);
    if (a.n_nodes <= 0 || a.replicas <= 0 || a.edge_capacity <= 0 || a.ldx < 4 || (a.ldx & 3) || !aligned16(a.X)) return refuse(MORIG_E_INVALID);
    if ((a.ldw & 3) || a.ldw < 32 || a.ldo < 32 || !aligned16(a.W2) || !aligned16(a.W1a) || !aligned16(a.W1b)) return refuse(MORIG_E_INVALID);
    if (a.in_rep_stride < 0 || (a.replicas > 1 && a.out_rep_stride < a.n_nodes)) return refuse(MORIG_E_INVALID);
    const bool f16 = a.W2_split != nullptr;
    if (f16 && (!a.overflow || !aligned16(a.W2_split))) return refuse(MORIG_E_INVALID);
    if (a.skip_init && a.init_with) return refuse(MORIG_E_INVALID);
    pl.blocks = cdiv(a.edge_capacity, 128) * a.replicas;
    pl.kind = f16 ? K_EDGE16_X3 : K_EDGE_X3;
    if (f16 && !sw.x3_tile && (a.ldo & 3) == 0 && aligned16(a.out)) { pl.engine = EDGE_X3; pl.retag = K_EDGE16_X3P; return pl; }
    pl.engine = EDGE_TILE;
    pl.tile = TileInst{32, 32, LOAD_EDGE3, MODE_EDGEMAX, f16 ? PREC_F16X3 : PREC_F32, false};
    return pl;
}

}  // namespace morig
