// The kernel choice of morig_gemm / morig_edgeconv / morig_edge_hidden / morig_segmax_gemm / morig_edgeconv_x3
// (morig_amd/csrc/dispatch_core.h) as a plain host program, so that the text the library compiles can be enumerated under the address
// and undefined-behaviour sanitizers: tests/test_dispatch_host.py builds it with -fsanitize=address,undefined and runs it as a
// program. Never loaded into Python, never run on a GPU machine. Pointers are made-up integers: nothing is dereferenced.
//
// Every case runs at default switches and with each switch alone at each of its non-default values. Checked:
//   (a) every MORIG_OK plan names a row of MORIG_TILE_TABLE or one of the special kernels listed in `Special`;
//   (b) every row of the table, every FAST form and every special kernel is reached by some case (a variant nothing reaches fails here);
//   (c) the rules include/morig_hip.h documents (K tails, tail + pool, pool + Y, the overflow word, split activations, split_ok,
//       H = 16, unknown widths);
//   (d) NativeOps.gemm_takes_tail (morig_amd/native.py), restated below, implies a tail-taking plan whenever the row bias is absent or
//       16-byte aligned;
//   (e) morig_edgeconv_can_split_out's answer (the plan of the arguments alone) equals the launch plan's split_ok;
//   (f) the paired passes: which refusals over init_with / skip_init / split_with / skip_split and an unknown H are `late`, that a late
//       refusal keeps the plan a partner check reads, and that the legal flag combinations leave the launch where it was.
// Prints "ok <cases checked>" or the first violation (exit status 1).
#include "../morig_amd/csrc/dispatch_core.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace morig;

template <class T> static T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }
static int up(int v, int m) { return (v + m - 1) / m * m; }

// ---- the switch settings ----
struct Setting { const char* name; const char* value; };
static const Setting kSettings[] = {
    {nullptr, nullptr},
    {"MORIG_NO_DMA", "1"}, {"MORIG_NO_EDGE_PC", "1"}, {"MORIG_TILE_NO_FAST", "1"}, {"MORIG_NO_FEW_ROWS", "1"},
    {"MORIG_EDGE_KERNEL", "pp"}, {"MORIG_EDGE_KERNEL", "pc"}, {"MORIG_RL128", "0"}, {"MORIG_EDGE_MIX", "0"}, {"MORIG_EDGE_RUN", "1"},
    {"MORIG_EDGE_SPLIT_OUT", "0"}, {"MORIG_X3_TILE", "1"}, {"MORIG_DMA_TILE", "128"}, {"MORIG_DMA_PERSIST", "0"}, {"MORIG_DMA_PERSIST", "1"},
    {"MORIG_DMA_SMALL_TILES", "0"}, {"MORIG_GEMM_TR", "0"}, {"MORIG_POOL_RUN", "4"}, {"MORIG_DEBUG_FLAGS", "1"},
};
constexpr int N_SETTINGS = sizeof(kSettings) / sizeof(kSettings[0]);
static Switches switches_of(const Setting& st) {
    return Switches::from([&](const char* n) -> const char* { return st.name && std::strcmp(n, st.name) == 0 ? st.value : nullptr; });
}

// ---- what was reached ----
enum Special { S_FEW_ROWS, S_DMA128, S_DMA256_LDS, S_DMA256_TR, S_DMA256_TAIL, S_DMAP_STORE, S_DMAP_POOL,
               S_EDGE_RL, S_EDGE_WS, S_EDGE_WS_SPLIT, S_EDGE_WS_MIX, S_EDGE_PP128, S_EDGE_PP256, S_EDGE_PC, S_EDGE_X3_GATHERED, S_EDGE_X3, S_COUNT };
static const char* kSpecialNames[S_COUNT] = {"few_rows_gemm_kernel", "gemm16_dma_kernel<128, 128, 2, 2, false>", "gemm16_dma_kernel<256, 256, 4, 2, false>",
    "gemm16_dma_kernel<256, 256, 4, 2, true>", "gemm16_dma_kernel<256, 256, 4, 2, true, true>", "gemm16_dmap_kernel<false>", "gemm16_dmap_kernel<true>",
    "edge_rl128_kernel", "edge_ws_kernel<256>", "edge_ws_kernel<256, true>", "edge_ws_kernel<256, true, true>", "edge_pp_kernel<128>", "edge_pp_kernel<256>",
    "edge_pc_kernel", "edge_x3_kernel<true>", "edge_x3_kernel<false>"};
static std::vector<int> g_row_hits, g_fast_hits;
static int g_special_hits[S_COUNT];
static long g_checked = 0;              // cases, one per check_* call

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

template <class Who> static int note_tile(const TileInst& t, Who&& who) {
    const int row = tile_table_index(t);
    if (row < 0) FAIL("%s: a plan names tile_kernel<%d, %d, %d, %d, %d>, which is no row of the table", who(), t.BN, t.KC, t.LOAD, t.MODE, t.PREC);
    if (t.fast && !tile_has_fast(t.BN, t.KC, t.LOAD, t.MODE)) FAIL("%s: FAST on a row that has no FAST form (%d)", who(), row);
    ++g_row_hits[row];
    if (t.fast) ++g_fast_hits[row];
    return 0;
}

// ---- morig_gemm ----
enum Image { IMG_NONE, IMG_F16, IMG_BF16, IMG_BF16X6, N_IMAGES };
enum Pool { POOL_NONE, POOL_ONLY, POOL_AND_Y, N_POOLS };
enum RowBias { RB_NONE, RB_ALIGNED, RB_MISALIGNED, N_ROWBIAS };
static const int kM[] = {0, 1, 127, 128, 129, 4096, 65536, 65792};
static const int kN[] = {16, 32, 33, 64, 65, 128, 256, 512, 1024};
static const int kK[] = {3, 32, 64, 96, 768, 832};
constexpr int N_M = 8, N_N = 9, N_K = 6;

struct GemmCase { int M, N, K, image, x_split, y_split, pool, rowbias, y_misaligned, tail; };
static morig_gemm_args gemm_args(const GemmCase& c) {
    morig_gemm_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.M = c.M; a.N = c.N; a.K = c.K;
    const int tail_cols = c.tail ? 32 : 0;
    a.X = fake<const float>(0x10000000); a.ldx = up(c.K - tail_cols > 0 ? c.K - tail_cols : 1, 32);
    a.W = fake<const float>(0x20000000); a.ldw = up(c.K, 32);
    a.relu = 1;
    if (c.image == IMG_F16 || c.image == IMG_BF16) a.W_split = fake<const void>(0x30000000);
    if (c.image == IMG_F16) a.overflow = fake<int32_t>(0x40000000);
    a.w_split_format = c.image == IMG_BF16 ? MORIG_SPLIT_BF16 : c.image == IMG_BF16X6 ? MORIG_SPLIT_BF16X6 : MORIG_SPLIT_F16;
    a.x_split = c.x_split; a.y_split = c.y_split;
    if (c.pool != POOL_ONLY) { a.Y = fake<float>(0x50000000 + (c.y_misaligned ? 4 : 0)); a.ldy = up(c.N, 32); }
    if (c.pool != POOL_NONE) { a.pool = fake<float>(0x60000000); a.ld_pool = up(c.N, 128); a.n_seg = 4; }
    if (c.rowbias != RB_NONE) { a.rowbias = fake<const float>(0x70000000 + (c.rowbias == RB_MISALIGNED ? 4 : 0)); a.ld_rowbias = up(c.N, 4); }
    if (c.pool != POOL_NONE || c.rowbias != RB_NONE) a.seg = fake<const int32_t>(0x78000000);
    if (c.tail) { a.X_tail = fake<const float>(0x80000000); a.ld_tail = 32; a.tail_rows = 64; a.tail_cols = 32; }
    return a;
}

static int check_gemm(const GemmCase& c, const Setting& st) {
    const Switches sw = switches_of(st);
    const morig_gemm_args a = gemm_args(c);
    const GemmPlan pl = gemm_plan(a, sw);
    ++g_checked;
    char text[200];
    auto who = [&]() -> const char* {                    // (only a violation pays for the text)
        std::snprintf(text, sizeof(text), "gemm M %d N %d K %d image %d x_split %d y_split %d pool %d rowbias %d y_misaligned %d tail %d [%s=%s]", c.M, c.N, c.K,
                      c.image, c.x_split, c.y_split, c.pool, c.rowbias, c.y_misaligned, c.tail, st.name ? st.name : "default", st.name ? st.value : "");
        return text;
    };
    if (pl.status != MORIG_OK && pl.status != MORIG_E_INVALID && pl.status != MORIG_E_UNSUPPORTED) FAIL("%s: status %d", who(), pl.status);
    if (pl.status != MORIG_OK && pl.engine != GEMM_NONE) FAIL("%s: a refusal names an engine", who());
    if (c.M == 0) { if (pl.status != MORIG_OK || pl.engine != GEMM_NONE) FAIL("%s: M = 0 is MORIG_OK and launches nothing", who()); return 0; }
    const bool split_acts = c.x_split || c.y_split;
    // (c) the documented rules. Every made-up argument is well formed, so where a rule refuses, it is the FIRST check that does
    const bool tail_well_formed = c.tail && c.x_split && (c.image == IMG_F16 || c.image == IMG_BF16) && c.K % 32 == 0 && c.K > 32;
    if (c.tail && !tail_well_formed && pl.status != MORIG_E_INVALID) FAIL("%s: a malformed tail is MORIG_E_INVALID, got %d", who(), pl.status);
    if (tail_well_formed && c.pool != POOL_NONE && pl.status != MORIG_E_UNSUPPORTED) FAIL("%s: tail + pool is MORIG_E_UNSUPPORTED, got %d", who(), pl.status);
    if (!c.tail && c.pool == POOL_AND_Y && pl.status != MORIG_E_UNSUPPORTED) FAIL("%s: pool + Y is MORIG_E_UNSUPPORTED, got %d", who(), pl.status);
    const bool consumers_ok = c.pool != POOL_AND_Y && !(c.tail && (c.pool != POOL_NONE || !tail_well_formed));
    if (consumers_ok && split_acts && (c.image == IMG_NONE || c.image == IMG_BF16X6) && pl.status != MORIG_E_INVALID)
        FAIL("%s: split activations without an f16 image are MORIG_E_INVALID, got %d", who(), pl.status);
    if (consumers_ok && c.image == IMG_BF16 && (split_acts || c.pool != POOL_NONE) && pl.status != MORIG_E_UNSUPPORTED)
        FAIL("%s: the bf16 image takes plain stores only (MORIG_E_UNSUPPORTED), got %d", who(), pl.status);
    if (c.image == IMG_F16) {
        morig_gemm_args b = a;
        b.overflow = nullptr;
        const GemmPlan q = gemm_plan(b, sw);
        if (q.status == MORIG_OK || (pl.status == MORIG_OK && q.status != MORIG_E_INVALID)) FAIL("%s: an f16 image without an overflow word is MORIG_E_INVALID, got %d", who(), q.status);
    }
    if (c.tail && pl.status == MORIG_OK && !(pl.engine == GEMM_DMA256 && pl.tr && pl.tail))
        FAIL("%s: a K tail is taken by the 256 x 256 register-epilogue tail kernel only (engine %d)", who(), pl.engine);
    if (c.tail && pl.status != MORIG_OK && tail_well_formed && c.pool == POOL_NONE && !(c.y_split && c.y_misaligned) && pl.status != MORIG_E_UNSUPPORTED)
        FAIL("%s: a well-formed tail that no kernel takes is MORIG_E_UNSUPPORTED, got %d", who(), pl.status);
    if (!c.tail && pl.tail) FAIL("%s: tail form without a tail", who());
    // (d) gemm_takes_tail: self.fast (an f16 image with split activations), no MORIG_NO_DMA, N % 256 == 0, K % 32 == 0, tail_cols % 32 == 0,
    // K > tail_cols, Y 16-byte aligned with ld % 4 == 0, MORIG_GEMM_TR not "0", MORIG_DMA_TILE "256"
    const bool python_says = c.image == IMG_F16 && !sw.no_dma && c.N % 256 == 0 && c.K % 32 == 0 && c.K > 32 && !c.y_misaligned && sw.gemm_tr && sw.dma_tile == 256;
    if (c.tail && c.x_split && c.pool == POOL_NONE && python_says && c.rowbias != RB_MISALIGNED && !(pl.status == MORIG_OK && pl.tail))
        FAIL("%s: gemm_takes_tail says yes, the plan refuses (%d)", who(), pl.status);
    if (pl.status != MORIG_OK) return 0;
    // (a)
    if (pl.blocks <= 0 || pl.tiles_n <= 0) FAIL("%s: an empty launch (%d blocks, %d column tiles)", who(), pl.blocks, pl.tiles_n);
    if (pl.kind < 0 || pl.kind >= K_COUNT || pl.retag < -1 || pl.retag >= K_COUNT) FAIL("%s: kinds %d / %d", who(), pl.kind, pl.retag);
    switch (pl.engine) {
        case GEMM_TILE:
            if (pl.tile.LOAD != LOAD_DENSE || pl.tile.MODE != (c.pool != POOL_NONE ? MODE_POOL : MODE_STORE)) FAIL("%s: tile mode", who());
            if (pl.tile.fast && (c.M % 128 || c.K % pl.tile.KC || sw.debug_flags || sw.tile_no_fast)) FAIL("%s: FAST with guards needed", who());
            if ((long)pl.tiles_n * pl.tile.BN < c.N) FAIL("%s: the column tiles do not cover N", who());
            return note_tile(pl.tile, who);
        case GEMM_FEW_ROWS: if (c.M > 128 || split_acts || c.rowbias != RB_NONE || c.pool != POOL_NONE) FAIL("%s: few-rows", who()); ++g_special_hits[S_FEW_ROWS]; return 0;
        case GEMM_DMA128: case GEMM_DMA256: case GEMM_DMAP: {
            if (!(c.image == IMG_F16 && c.x_split && c.N > 64) || sw.no_dma) FAIL("%s: an LDS-DMA engine without pre-split operands", who());
            const int tile = pl.engine == GEMM_DMA128 ? 128 : 256;
            if ((long)pl.tiles_n * tile < c.N || (pl.engine != GEMM_DMA128 && c.N % 256)) FAIL("%s: the column tiles do not cover N", who());
            if (pl.engine != GEMM_DMA128 && pl.tr && (c.y_misaligned || c.rowbias == RB_MISALIGNED || c.pool != POOL_NONE)) FAIL("%s: register epilogue on misaligned rows", who());
            if (pl.engine == GEMM_DMAP && !pl.tr && c.pool == POOL_NONE) FAIL("%s: the persistent store kernel has the register epilogue only", who());
            const int sp = pl.engine == GEMM_DMA128 ? S_DMA128 : pl.engine == GEMM_DMAP ? (c.pool != POOL_NONE ? S_DMAP_POOL : S_DMAP_STORE)
                         : pl.tail ? S_DMA256_TAIL : pl.tr ? S_DMA256_TR : S_DMA256_LDS;
            ++g_special_hits[sp];
            return 0;
        }
        default: FAIL("%s: MORIG_OK without an engine", who());
    }
}

// ---- the EdgeConv family ----
static const int kH[] = {16, 32, 64, 128, 256, 48};
constexpr int N_H = 6;
enum Csr { CSR_PLAIN, CSR_PAD4, CSR_MIN4, N_CSRS };
constexpr int kEdgeRows = 700000;            // enough 64-row tiles that the split-rows kernels form runs
struct EdgeCase { int H, csr, image, affine, out_split, out_misaligned, replicas, exact_arith; };
static morig_edgeconv_args edge_args(const EdgeCase& c) {
    morig_edgeconv_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.H = c.H; a.n_nodes = 64; a.replicas = c.replicas; a.in_rep_stride = 64; a.out_rep_stride = 64;
    const int ld = up(c.H, 32);
    a.A = fake<const float>(0x10000000); a.lda = ld; a.B = fake<const float>(0x11000000); a.ldb = ld;
    a.rowptr = fake<const int32_t>(0x12000000); a.src_sorted = fake<const int32_t>(0x13000000); a.dst_sorted = fake<const int32_t>(0x14000000);
    a.edge_capacity = kEdgeRows;
    if (c.affine) { a.s1 = fake<const float>(0x15000000); a.t1 = fake<const float>(0x15100000); }
    a.W2 = fake<const float>(0x20000000); a.ldw = ld;
    a.b2 = fake<const float>(0x21000000); a.s2 = fake<const float>(0x22000000); a.t2 = fake<const float>(0x23000000);
    a.out = fake<float>(0x50000000 + (c.out_misaligned ? 4 : 0)); a.ldo = ld;
    if (c.image) { a.W2_split = fake<const void>(0x30000000); a.overflow = fake<int32_t>(0x40000000); }
    a.quad_aligned = c.csr == CSR_PAD4; a.seg_min4 = c.csr == CSR_MIN4;
    a.out_split = c.out_split; a.exact_arith = c.exact_arith;
    return a;
}
static bool known_width(int H) { return H == 16 || H == 32 || H == 64 || H == 128 || H == 256; }

template <class Who> static int check_edge_tile(const EdgePlan& pl, int width, int load, int mode, bool image, Who&& who) {
    if (pl.tile.LOAD != load || pl.tile.MODE != mode || pl.tile.fast) FAIL("%s: tile loader / mode", who());
    if (width == 16 ? !(pl.tile.BN == 32 && pl.tile.KC == 16 && pl.tile.PREC == PREC_F32) : pl.tile.BN != width) FAIL("%s: tile width %d for H %d", who(), pl.tile.BN, width);
    if (image != (pl.tile.PREC == PREC_F16X3)) FAIL("%s: arithmetic %d", who(), pl.tile.PREC);
    return note_tile(pl.tile, who);
}

static int check_edge(const EdgeCase& c, const Setting& st) {
    const Switches sw = switches_of(st);
    const morig_edgeconv_args a = edge_args(c);
    char text[200];
    auto who = [&]() -> const char* {
        std::snprintf(text, sizeof(text), "edge H %d csr %d image %d affine %d out_split %d out_misaligned %d replicas %d exact %d [%s=%s]", c.H, c.csr, c.image,
                      c.affine, c.out_split, c.out_misaligned, c.replicas, c.exact_arith, st.name ? st.name : "default", st.name ? st.value : "");
        return text;
    };
    // morig_edgeconv
    const EdgePlan pl = edge_plan(a, sw);
    ++g_checked;
    if (pl.status != MORIG_OK && pl.status != MORIG_E_INVALID && pl.status != MORIG_E_UNSUPPORTED) FAIL("%s: status %d", who(), pl.status);
    if (pl.kind < 0 || pl.kind >= K_COUNT || pl.retag < -1 || pl.retag >= K_COUNT) FAIL("%s: kinds %d / %d", who(), pl.kind, pl.retag);
    // (e) what morig_edgeconv_can_split_out answers: the plan of the arguments alone
    const bool can_split = edge_plan(a, sw, true).split_ok;
    if ((pl.status == MORIG_OK || pl.late) && can_split != pl.split_ok) FAIL("%s: can_split_out %d, plan %d", who(), (int)can_split, (int)pl.split_ok);
    if (c.out_split && !can_split && pl.status != (c.H == 16 && c.image ? MORIG_E_INVALID : MORIG_E_UNSUPPORTED)) FAIL("%s: out_split where it cannot be honoured is MORIG_E_UNSUPPORTED, got %d", who(), pl.status);
    // (c) split_ok only on RL / WS / WS-mix: asked with out_split, the launch takes one of them
    if (can_split) {
        morig_edgeconv_args b = a;
        b.out_split = 1;
        const EdgePlan q = edge_plan(b, sw);
        if (q.status != MORIG_OK || !edge_splits(q)) FAIL("%s: split_ok, but out_split gets status %d on engine %d", who(), q.status, q.engine);
    }
    if (c.H == 16 && c.image && pl.status != MORIG_E_INVALID) FAIL("%s: H = 16 has no split image (MORIG_E_INVALID), got %d", who(), pl.status);
    if (!known_width(c.H) && pl.status != MORIG_E_UNSUPPORTED) FAIL("%s: an H the library does not have is MORIG_E_UNSUPPORTED, got %d", who(), pl.status);
    if (known_width(c.H) && !(c.H == 16 && c.image) && !c.out_split && pl.status != MORIG_OK) FAIL("%s: a plain launch is refused (%d)", who(), pl.status);
    if (pl.status == MORIG_OK) {
        if (c.out_split && !edge_splits(pl)) FAIL("%s: out_split on engine %d", who(), pl.engine);
        if (pl.blocks != (kEdgeRows + pl.tile_rows - 1) / pl.tile_rows * c.replicas) FAIL("%s: %d blocks of %d rows", who(), pl.blocks, pl.tile_rows);
        if (pl.run < 1 || (pl.run & (pl.run - 1)) || pl.run > sw.edge_run || (pl.run > 1 && !edge_splits(pl))) FAIL("%s: run %d", who(), pl.run);
        if ((pl.tile_rows == 64) != edge_splits(pl)) FAIL("%s: tile rows %d on engine %d", who(), pl.tile_rows, pl.engine);
        switch (pl.engine) {
            case EDGE_TILE: if (check_edge_tile(pl, c.H, LOAD_EDGE, MODE_EDGEMAX, c.image, who)) return 1; break;
            case EDGE_RL: if (!(c.H == 128 && c.image && c.csr == CSR_PAD4 && !c.affine)) FAIL("%s: RL", who()); ++g_special_hits[S_EDGE_RL]; break;
            case EDGE_WS: if (!(c.H == 256 && c.image && c.csr == CSR_PAD4 && !c.affine)) FAIL("%s: WS", who()); ++g_special_hits[c.out_split ? S_EDGE_WS_SPLIT : S_EDGE_WS]; break;
            case EDGE_WS_MIX: if (!(c.H == 256 && c.image && c.csr == CSR_MIN4 && !c.affine && c.out_split)) FAIL("%s: WS-mix", who()); ++g_special_hits[S_EDGE_WS_MIX]; break;
            case EDGE_PP: if (!((c.H == 128 || c.H == 256) && c.image && !c.affine && !c.out_misaligned)) FAIL("%s: PP", who()); ++g_special_hits[c.H == 128 ? S_EDGE_PP128 : S_EDGE_PP256]; break;
            case EDGE_PC: if (!((c.H == 128 || c.H == 256) && c.image && !c.affine)) FAIL("%s: PC", who()); ++g_special_hits[S_EDGE_PC]; break;
            case EDGE_X3: if (!(c.H == 32 && c.image && !c.affine && !c.out_misaligned)) FAIL("%s: X3", who()); ++g_special_hits[S_EDGE_X3_GATHERED]; break;
            default: FAIL("%s: MORIG_OK without an engine", who());
        }
        if (c.H == 16 && pl.engine != EDGE_TILE) FAIL("%s: H = 16 runs on the fp32 tile only", who());
    }
    // morig_edge_hidden
    const EdgePlan ph = edge_hidden_plan(a, sw);
    const int want = (c.H == 16 && c.image) ? MORIG_E_INVALID : (c.replicas != 1 || c.out_split || !known_width(c.H)) ? MORIG_E_UNSUPPORTED : MORIG_OK;
    if (ph.status != want) FAIL("%s: edge_hidden status %d, expected %d", who(), ph.status, want);
    if (ph.status == MORIG_OK && (ph.engine != EDGE_TILE || ph.blocks != (kEdgeRows + 127) / 128 || check_edge_tile(ph, c.H, LOAD_EDGE, MODE_STORE, c.image, who))) FAIL("%s: edge_hidden plan", who());
    return 0;
}

// The paired passes of morig_edgeconv (init_with / skip_init / split_with / skip_split): a refusal over these flags, and the one over an
// unknown H, stand BEHIND the checks of an init_with partner in the order of the codes -- the plan marks them `late` and keeps the
// engine, and a call that is looked at as a partner passes with them (tile_gemm.hip: qp.late ? MORIG_OK : qp.status). Refusals over
// the arguments themselves are never late.
enum PairFlags { PF_SKIP_INIT_AND_INIT_WITH, PF_SPLIT_WITH_NO_SPLIT, PF_SKIP_SPLIT_NO_SPLIT, PF_SPLIT_WITH_AND_SKIP_SPLIT, PF_SKIP_SPLIT, PF_SPLIT_WITH,
                 PF_INIT_WITH, PF_UNKNOWN_H, PF_UNKNOWN_H_AND_FLAGS, PF_BAD_ARGS_AND_FLAGS, PF_SPLIT_REFUSED_AND_FLAGS, N_PAIR_FLAGS };
static const int kPairH[] = {32, 64, 128, 256};
constexpr int N_PAIR_H = 4;
static int check_pair_flags(int H, int csr, int flags, const Setting& st) {
    const Switches sw = switches_of(st);
    const morig_edgeconv_args* other = fake<const morig_edgeconv_args>(0x90000000);       // never dereferenced by a plan
    const bool wants_split = flags == PF_SPLIT_WITH_AND_SKIP_SPLIT || flags == PF_SKIP_SPLIT || flags == PF_SPLIT_WITH;
    EdgeCase c{H, csr, 1, 0, wants_split ? 1 : 0, 0, 2, 0};
    if (flags == PF_UNKNOWN_H || flags == PF_UNKNOWN_H_AND_FLAGS) c.H = 48;
    if (flags == PF_SPLIT_REFUSED_AND_FLAGS) { c.out_split = 1; c.out_misaligned = 1; }
    const morig_edgeconv_args plain = edge_args(c);
    morig_edgeconv_args a = plain;
    switch (flags) {
        case PF_SKIP_INIT_AND_INIT_WITH: a.skip_init = 1; a.init_with = other; break;
        case PF_SPLIT_WITH_NO_SPLIT: a.split_with = other; break;
        case PF_SKIP_SPLIT_NO_SPLIT: a.skip_split = 1; break;
        case PF_SPLIT_WITH_AND_SKIP_SPLIT: a.split_with = other; a.skip_split = 1; break;
        case PF_SKIP_SPLIT: a.skip_split = 1; a.init_with = other; break;              // the first launch of a pair
        case PF_SPLIT_WITH: a.split_with = other; a.skip_init = 1; break;              // the second
        case PF_INIT_WITH: a.init_with = other; break;
        case PF_UNKNOWN_H_AND_FLAGS: a.skip_init = 1; a.init_with = other; break;
        case PF_BAD_ARGS_AND_FLAGS: a.b2 = nullptr; a.skip_init = 1; a.init_with = other; break;
        case PF_SPLIT_REFUSED_AND_FLAGS: a.skip_split = 1; break;
        default: break;
    }
    const EdgePlan base = edge_plan(plain, sw), pl = edge_plan(a, sw);
    ++g_checked;
    char text[160];
    std::snprintf(text, sizeof(text), "pair flags %d H %d csr %d [%s=%s]", flags, H, csr, st.name ? st.name : "default", st.name ? st.value : "");
    auto who = [&]() -> const char* { return text; };
    int want = MORIG_OK;
    bool late = false;
    switch (flags) {
        case PF_SKIP_INIT_AND_INIT_WITH: case PF_SPLIT_WITH_NO_SPLIT: case PF_SKIP_SPLIT_NO_SPLIT: want = MORIG_E_INVALID; late = true; break;
        case PF_SPLIT_WITH_AND_SKIP_SPLIT: case PF_SKIP_SPLIT: case PF_SPLIT_WITH:
            // without split rows the launch is refused for out_split itself, early; with them only the two flags together are illegal
            if (base.status != MORIG_OK) want = MORIG_E_UNSUPPORTED;
            else if (flags == PF_SPLIT_WITH_AND_SKIP_SPLIT) { want = MORIG_E_INVALID; late = true; }
            break;
        case PF_UNKNOWN_H: want = MORIG_E_UNSUPPORTED; late = true; break;
        case PF_UNKNOWN_H_AND_FLAGS: want = MORIG_E_INVALID; late = true; break;           // the flags are looked at in front of the width
        case PF_BAD_ARGS_AND_FLAGS: want = MORIG_E_INVALID; break;
        case PF_SPLIT_REFUSED_AND_FLAGS: want = MORIG_E_UNSUPPORTED; break;
        default: break;
    }
    if (pl.status != want || pl.late != late) FAIL("%s: status %d late %d, expected %d late %d", who(), pl.status, (int)pl.late, want, (int)late);
    if (pl.status != MORIG_OK && !pl.late && (pl.engine != EDGE_NONE || pl.split_ok)) FAIL("%s: an early refusal names an engine", who());
    // a late refusal keeps what the partner checks of the other launch look at: the engine of a wide launch, the tile rows, the run,
    // split_ok (the tile engine and the 32-wide kernel are named behind the flags: a partner reads nothing of them but 128-row tiles)
    const bool wide = edge_splits(base) || base.engine == EDGE_PP || base.engine == EDGE_PC;
    if (pl.late && c.H != 48 && (pl.engine != (wide ? base.engine : (int)EDGE_NONE) || pl.tile_rows != base.tile_rows || pl.run != base.run || pl.split_ok != base.split_ok))
        FAIL("%s: a late refusal changed the plan (engine %d, was %d)", who(), pl.engine, base.engine);
    if (pl.status == MORIG_OK && (pl.engine != base.engine || pl.run != base.run || pl.blocks != base.blocks)) FAIL("%s: the pair flags moved the launch", who());
    return 0;
}

static const int kSegN[] = {16, 32, 33, 64, 65, 128, 256, 512};
constexpr int N_SEGN = 8;
static int check_segmax(int N, int image, const Setting& st) {
    morig_segmax_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.N = N; a.K = 64; a.X = fake<const float>(0x10000000); a.ldx = 64; a.W = fake<const float>(0x20000000); a.ldw = 64;
    a.rowptr = fake<const int32_t>(0x12000000); a.dst_sorted = fake<const int32_t>(0x14000000); a.n_nodes = 64; a.edge_capacity = 200;
    a.out = fake<float>(0x50000000); a.ldo = up(N, 4);
    if (image) { a.W_split = fake<const void>(0x30000000); a.overflow = fake<int32_t>(0x40000000); }
    const EdgePlan pl = segmax_plan(a, switches_of(st));
    ++g_checked;
    char text[100];
    auto who = [&]() -> const char* { return text; };
    std::snprintf(text, sizeof(text), "segmax N %d image %d [%s]", N, image, st.name ? st.name : "default");
    if (pl.status != (N <= 256 ? MORIG_OK : MORIG_E_UNSUPPORTED)) FAIL("%s: status %d", who(), pl.status);
    if (pl.status != MORIG_OK) return 0;
    if (pl.engine != EDGE_TILE || pl.blocks != 2 || pl.tile.BN < N || (pl.tile.BN > 32 && pl.tile.BN / 2 >= N)) FAIL("%s: plan (BN %d)", who(), pl.tile.BN);
    return check_edge_tile(pl, pl.tile.BN, LOAD_DENSE, MODE_EDGEMAX, image, who);
}

static int check_x3(int H, int image, int out_misaligned, const Setting& st) {
    morig_edgeconv_x3_args a;
    std::memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.H = H; a.n_nodes = 64; a.replicas = 2; a.in_rep_stride = 64; a.out_rep_stride = 64;
    a.X = fake<const float>(0x10000000); a.ldx = 4;
    a.W1a = fake<const float>(0x11000000); a.W1b = fake<const float>(0x11100000); a.b1 = fake<const float>(0x11200000);
    a.rowptr = fake<const int32_t>(0x12000000); a.src_sorted = fake<const int32_t>(0x13000000); a.dst_sorted = fake<const int32_t>(0x14000000);
    a.edge_capacity = 200;
    a.W2 = fake<const float>(0x20000000); a.ldw = 32;
    a.b2 = fake<const float>(0x21000000); a.s2 = fake<const float>(0x22000000); a.t2 = fake<const float>(0x23000000);
    a.out = fake<float>(0x50000000 + (out_misaligned ? 4 : 0)); a.ldo = 32;
    if (image) { a.W2_split = fake<const void>(0x30000000); a.overflow = fake<int32_t>(0x40000000); }
    const Switches sw = switches_of(st);
    const EdgePlan pl = edgeconv_x3_plan(a, sw);
    ++g_checked;
    char text[100];
    auto who = [&]() -> const char* { return text; };
    std::snprintf(text, sizeof(text), "edgeconv_x3 H %d image %d out_misaligned %d [%s]", H, image, out_misaligned, st.name ? st.name : "default");
    if (pl.status != (H == 32 ? MORIG_OK : MORIG_E_UNSUPPORTED)) FAIL("%s: status %d", who(), pl.status);
    if (pl.status != MORIG_OK) return 0;
    if (pl.blocks != 4) FAIL("%s: %d blocks", who(), pl.blocks);
    if (pl.engine == EDGE_X3) {
        if (!image || out_misaligned || sw.x3_tile || pl.retag != K_EDGE16_X3P) FAIL("%s: the persistent kernel", who());
        ++g_special_hits[S_EDGE_X3];
        return 0;
    }
    if (pl.engine != EDGE_TILE) FAIL("%s: engine %d", who(), pl.engine);
    return check_edge_tile(pl, 32, LOAD_EDGE3, MODE_EDGEMAX, image, who);
}

int main() {
    g_row_hits.assign(tile_table_size(), 0);
    g_fast_hits.assign(tile_table_size(), 0);
    for (int s = 0; s < N_SETTINGS; ++s) {
        const Setting& st = kSettings[s];
        for (int im = 0; im < N_M; ++im) for (int in = 0; in < N_N; ++in) for (int ik = 0; ik < N_K; ++ik)
            for (int image = 0; image < N_IMAGES; ++image) for (int xs = 0; xs < 2; ++xs) for (int ys = 0; ys < 2; ++ys)
                for (int pool = 0; pool < N_POOLS; ++pool) for (int rb = 0; rb < N_ROWBIAS; ++rb) for (int ym = 0; ym < 2; ++ym) for (int tail = 0; tail < 2; ++tail)
                    if (check_gemm(GemmCase{kM[im], kN[in], kK[ik], image, xs, ys, pool, rb, ym, tail}, st)) return 1;
        for (int ih = 0; ih < N_H; ++ih) for (int csr = 0; csr < N_CSRS; ++csr) for (int image = 0; image < 2; ++image) for (int aff = 0; aff < 2; ++aff)
            for (int os = 0; os < 2; ++os) for (int om = 0; om < 2; ++om) for (int rep = 1; rep <= 2; ++rep) for (int ex = 0; ex < 2; ++ex)
                if (check_edge(EdgeCase{kH[ih], csr, image, aff, os, om, rep, ex}, st)) return 1;
        for (int ih = 0; ih < N_PAIR_H; ++ih) for (int csr = 0; csr < N_CSRS; ++csr) for (int f = 0; f < N_PAIR_FLAGS; ++f)
            if (check_pair_flags(kPairH[ih], csr, f, st)) return 1;
        for (int in = 0; in < N_SEGN; ++in) for (int image = 0; image < 2; ++image) if (check_segmax(kSegN[in], image, st)) return 1;
        for (int H = 32; H <= 64; H += 32) for (int image = 0; image < 2; ++image) for (int om = 0; om < 2; ++om) if (check_x3(H, image, om, st)) return 1;
    }
    // (b) nothing in the table, and no special kernel, is out of reach
    int row = 0;
#define MORIG_TILE_ROW(BN, KC, LOAD, MODE, PREC)                                                                                                \
    if (g_row_hits[row] == 0) FAIL("no case reaches tile_kernel<%d, %d, %d, %d, %d>", BN, KC, LOAD, MODE, PREC);                               \
    if (tile_has_fast(BN, KC, LOAD, MODE) && (g_fast_hits[row] == 0 || g_fast_hits[row] == g_row_hits[row]))                                    \
        FAIL("tile_kernel<%d, %d, %d, %d, %d>: one of the FAST and the guarded form is never reached", BN, KC, LOAD, MODE, PREC);              \
    ++row;
    MORIG_TILE_TABLE(MORIG_TILE_ROW)
#undef MORIG_TILE_ROW
    for (int k = 0; k < S_COUNT; ++k)
        if (g_special_hits[k] == 0) FAIL("no case reaches %s", kSpecialNames[k]);
    // the parse rules of the switches
    const Switches d = switches_of(kSettings[0]);
    if (d.no_dma || d.no_edge_pc || d.tile_no_fast || d.no_few_rows || d.edge_kernel != Switches::EK_DEFAULT || !d.rl128 || !d.edge_mix || d.edge_run != 8 ||
        !d.edge_split_out || d.x3_tile || d.dma_tile != 256 || d.dma_persist != 1 || d.dma_small_tiles != 256 || !d.gemm_tr || d.pool_run != 0 || d.debug_flags)
        FAIL("the defaults of the switches");
    if (switches_of({"MORIG_EDGE_RUN", "0"}).edge_run != 1 || switches_of({"MORIG_EDGE_RUN", "99999"}).edge_run != 4096 || switches_of({"MORIG_POOL_RUN", "-3"}).pool_run != 0 ||
        switches_of({"MORIG_POOL_RUN", "999"}).pool_run != 256 || switches_of({"MORIG_DMA_PERSIST", "yes"}).dma_persist != 2 || switches_of({"MORIG_X3_TILE", "0"}).x3_tile ||
        switches_of({"MORIG_RL128", "1"}).rl128 != true || switches_of({"MORIG_EDGE_KERNEL", "px"}).edge_kernel != Switches::EK_DEFAULT || Switches::to_int(" \t-12x") != -12)
        FAIL("the parse rules of the switches");
    std::printf("ok %ld\n", g_checked);
    return 0;
}
