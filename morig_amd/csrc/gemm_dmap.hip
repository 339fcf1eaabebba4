// PERSISTENT variant of the LDS-DMA split-fp16 GEMM (gemm_dma.hip), 256 x 256 tiles, 8 waves of 64 x 128.
//
// gemm_dma.hip launches one workgroup per tile: every tile pays a cold start (~2.5 us until its first K-chunk has landed in
// LDS and the first fragments are read: 3-7 % of a launch) with nothing to hide it, because the 128 KB ring and 512 threads at
// 256 registers leave room for ONE workgroup per CU. Here one workgroup per CU walks a static list of tiles (contiguous per
// XCD, as the EdgeConv kernels do) and treats the K-chunks of consecutive tiles as ONE stream through the 2-stage ring:
//   * chunk 0 of tile j+1 is fetched in the DMA slot of tile j's second-to-last chunk -- the stage it goes to was freed by
//     that chunk's hand-over barrier -- so it lands under tile j's last chunk and store epilogue;
//   * the store epilogue transposes through the stage of tile j's LAST chunk only (16-row slabs, 8 KB per wave = one stage),
//     never through the stage that is receiving the next tile's chunk 0;
//   * chunk 1 of tile j+1 is fetched when the epilogue is over (the usual prologue slot).
// vmcnt counts stores as well, so the wait for chunk 0' sits BEFORE the epilogue's stores (it was issued a chunk earlier).
// The swizzled ring image, fragment loads, MFMA groups and DMA pieces are dma_ring.h's, shared with gemm_dma.hip; counted waits,
// DMA instructions spread between MFMA groups and the epilogues follow gemm_dma.hip. Reference op: the vertex MLP layers, models/basic_modules.py:31-36.
#include "common.h"
#include "dma_ring.h"
#include "epilogue_store.h"
#include "pool_epilogue.h"
#include "pool_runs.h"
#include <stdlib.h>
#include <type_traits>

namespace morig {

// The parameter block stays in the kernarg segment: the persistent loop reads its fields through a pointer the compiler cannot see
// through (re-made opaque at the top of every tile and of every epilogue), so they are s_load-ed from the scalar cache where
// they are used instead of being hoisted out of the tile loop -- hoisted, they cost 59 spilled SGPRs and, through the spill lanes,
// 26 spilled VGPRs in a kernel that needs 250 for accumulators and fragments.
struct GemmDmaHot { int M, K, ldx, ldw, tiles_n; const float* X; const float* W; const int* seg; };
typedef __attribute__((address_space(4))) const GemmDmaParams* kernarg_params_t;
// POOL = true : pooled launches (column max per mesh): accumulators in the usual layout (a lane owns a column). The tile list is
//               cut into RUNS of consecutive row tiles of one column block (pool_runs.h) and the epilogue of a tile only merges the
//               raw max / min over the rows of its wave tile into a running pair per lane and column (pool_epilogue.h; the pair
//               lives in 16 KB of LDS behind the ring: 2 ds_read_b128 + 2 ds_write_b128 per wave and tile, no register across the K
//               loop). The pair is FLUSHED -- column constants loaded, transform applied once per column, one atomic per column --
//               when the wave's mesh id changes and at the end of a run: once or twice per mesh instead of once per tile.
// POOL = false: store launches: the MFMAs run with the operands swapped (A = W fragment, B = X fragment), the result tile is D^T
//               (a lane owns an output ROW and groups of 4 adjacent columns) and leaves through the register epilogue
//               (epilogue_store.h: store_tile_regs): no LDS scratch, no barrier in front of the epilogue; bias (+ the row bias of
//               a one-mesh tile) = initial accumulator value, taken from a double-buffered LDS panel that is loaded for tile
//               j + 1 BEFORE tile j's stores are issued (vmcnt retires in order).
template <bool POOL>
__global__ __launch_bounds__(512) void gemm16_dmap_kernel(const GemmDmaParams) {
#if defined(__HIP_DEVICE_COMPILE__)              // (the host pass only needs the symbol: the body reads the kernarg segment directly)
    kernarg_params_t q = (kernarg_params_t)__builtin_amdgcn_kernarg_segment_ptr();   // the one by-value argument
    asm volatile("" : "+s"(q));
    const GemmDmaHot p = {q->M, q->K, q->ldx, q->ldw, q->tiles_n, q->X, q->W, q->seg};        // what the main loop reads
    constexpr int BM = 256, BN = 256, NT = 4, MT = 2;
    constexpr int WNW = BN / (32 * NT);          // 2 waves along N
    constexpr int NW = (BM / 64) * WNW;          // 8 waves
    constexpr int STAGE = (BM + BN) * 128;       // 64 KB: X tile + W tile of one 32-column chunk
    constexpr int XJ = BM / 8 / NW, WJ = BN / 8 / NW;     // 4 + 4 one-KiB DMA instructions per wave and chunk
    constexpr int PANEL = 3 * BN;                // floats: [bias (+ row bias) | scale | shift] of a tile's columns
    constexpr int PAIR = 2 * NT * 64;            // floats per wave: the running (max, min) of its lanes' NT columns over a pooled run
    // (ONE __shared__ object on purpose: a second one beside a ring that LDS-DMA writes can cost a vmcnt(0) in front of every ds_read)
    __shared__ __attribute__((aligned(128))) char smem[2 * STAGE + (POOL ? NW * PAIR * 4 : 2 * PANEL * 4)];
    float* pan = reinterpret_cast<float*>(smem + 2 * STAGE);          // POOL = false: two panels (tile parity)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wm = wave / WNW, wn = wave % WNW;

    // ---- this workgroup's tile list (tile_list.h) of linear tile ids (row tile major, so the N-tiles of one row tile run at the
    // same time on one XCD and share its L2); POOL: of runs (pool_runs.h: run = up to q->run consecutive row tiles of one column
    // block; run length 1 = the same list) ----
    const int tiles_m = (p.M + BM - 1) / BM;
    const int T = tiles_m * p.tiles_n;
    const int xcd = blockIdx.x & 7, bi = blockIdx.x >> 3, nbx = gridDim.x >> 3;
    TileList tl = {};                            // store launches: the list of tiles
    int run_u = 0, run_left = 0;                 // POOL: the current run and the tiles of it that follow the current tile
    int n_my;
    if constexpr (POOL) {
        int u_end, u_stride;
        n_my = pool_wg_tiles(tiles_m, p.tiles_n, q->run, (int)gridDim.x, (int)blockIdx.x);
        pool_wg_runs(pool_run_units(tiles_m, p.tiles_n, q->run), (int)gridDim.x, (int)blockIdx.x, run_u, u_end, u_stride);
    } else {
        tl = tile_list(T, xcd, bi, nbx);
        n_my = tile_list_count(tl);
    }
    if (n_my <= 0) return;                       // block-uniform

    const int nchunk = (p.K + 31) / 32;          // >= 2 (the launcher sends shallower products to gemm_dma.hip)
    const int rsub = lane >> 3, pslot = lane & 7;
    unsigned ow[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int r = (wave * WJ + j) * 8 + rsub;
        ow[j] = dma_piece_offset(r, r, p.ldw, pslot);
    }
    // X source offsets of a tile whose first row is row0 (dma_ring.h)
    auto x_offset = [&](int j, int row0) __attribute__((always_inline)) {
        return dma_x_offset((wave * XJ + j) * 8 + rsub, row0, p.M, p.ldx, pslot);
    };
    // Measurement builds (tools/gpu_gemm_ablate.sh; results wrong by construction): DMAP_ABL_HOT = every LDS-DMA re-reads chunk 0 of
    // tile 0 (cache-hot: what the instructions cost without the memory behind them), DMAP_ABL_NODMA = none issued in the steady
    // state, DMAP_ABL_NOWAIT = nobody waits for them to land, DMAP_ABL_NOFRAG = no fragment reads in the steady state
    auto dma_x = [&](const char* xb, unsigned o, int c, int stage, int j) __attribute__((always_inline)) {
#ifdef DMAP_ABL_HOT
        xb = reinterpret_cast<const char*>(p.X); c = 0;
#endif
        dma_piece(xb, c, o, smem + stage * STAGE, wave * XJ + j);
    };
    auto dma_w = [&](const char* wb, int c, int stage, int j) __attribute__((always_inline)) {
#ifdef DMAP_ABL_HOT
        wb = reinterpret_cast<const char*>(p.W); c = 0;
#endif
        dma_piece(wb, c, ow[j], smem + stage * STAGE + BM * 128, wave * WJ + j);
    };

    const int x7 = (l31 >> 1) & 7;
    const int aoff = (wm * 64 + l31) * 128, boff = BM * 128 + (wn * NT * 32 + l31) * 128;
    // fragments and MFMAs: dma_ring.h; the store variant swaps the operand roles (D^T = W X^T)
    typedef SplitFrag<MT, NT> Frag;
    auto load_frag = [&](Frag& f, int stage, int s2) __attribute__((always_inline)) {
        load_split_frag(f, smem + stage * STAGE, aoff, boff, s2, hi, x7);
    };
    f32x16 acc[MT][NT];
    auto mma = [&](const Frag& f) __attribute__((always_inline)) { split_mma<!POOL>(f, acc); };
    auto mma_pair = [&](const Frag& f, int mt, int nt0) __attribute__((always_inline)) { split_mma_pair<!POOL>(f, acc, mt, nt0); };
    // ---- store variant: the column constants of one tile. Threads 0..255 fetch bias (+ the row bias when all rows of the tile lie
    // in one mesh), threads 256..511 scale and shift; `slow` (block-uniform) = the tile spans several meshes, the row bias is added
    // per row in the epilogue instead. Parameters come from the kernarg segment (scalar loads). ----
    float pv0 = 0.f, pv1 = 0.f;
    auto panel_fetch = [&](int plin, bool& slow) __attribute__((always_inline)) {
        asm volatile("" : "+s"(q));
        const float* bias = q->bias; const float* scale = q->scale; const float* shift = q->shift;
        const float* rowbias = q->rowbias; const int* seg = q->seg;
        const int col = (plin % p.tiles_n) * BN + (tid & (BN - 1));
        slow = false;
        pv0 = 0.f; pv1 = 0.f;
        if (tid < BN) {
            if (bias) pv0 = bias[col];
        } else if (scale) { pv0 = scale[col]; pv1 = shift[col]; }
        if (rowbias != nullptr) {
            const int prow0 = (plin / p.tiles_n) * BM;
            const int s0 = seg[prow0], s1 = seg[min(prow0 + BM, p.M) - 1];       // `seg` is sorted: one mesh iff the ends agree
            slow = s0 != s1;
            if (!slow && tid < BN) pv1 = rowbias[(size_t)s0 * q->ld_rowbias + col];
        }
    };
    auto panel_write = [&](int par) __attribute__((always_inline)) {
        float* pn = pan + par * PANEL;
        if (tid < BN) pn[tid] = pv0 + pv1;
        else { pn[BN + (tid - BN)] = pv0; pn[2 * BN + (tid - BN)] = pv1; }
    };

    // one K-chunk of the stream. `more`: a chunk of this tile follows (hand-over barrier in the middle); `go`: this chunk's DMA slot
    // is used -- for stream chunk g + c + 2, which goes to the stage chunk c is leaving -- with the given bases / chunk index
    unsigned ox[XJ];
    Frag f0, f1;
    auto chunk_iter = [&](int st, auto morec, auto goc, const char* xb, const char* wb, int cc, bool reclamp, int nrow0)
                          __attribute__((always_inline)) {
#ifdef DMAP_ABL_NODMA
        constexpr bool more = decltype(morec)::value != 0, go = false;
#else
        constexpr bool more = decltype(morec)::value != 0, go = decltype(goc)::value != 0;
#endif
#ifdef DMAP_ABL_NOFRAG
        asm volatile("" : "+v"(f1.ah[0]), "+v"(f1.al[0]), "+v"(f1.ah[1]), "+v"(f1.al[1]));
        asm volatile("" : "+v"(f1.bh[0]), "+v"(f1.bl[0]), "+v"(f1.bh[1]), "+v"(f1.bl[1]), "+v"(f1.bh[2]), "+v"(f1.bl[2]), "+v"(f1.bh[3]), "+v"(f1.bl[3]));
#else
        load_frag(f1, st, 1);
#endif
        mma(f0);
        if constexpr (more) {
#ifndef DMAP_ABL_NOWAIT
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // chunk c+1 landed for this wave (the only DMA in flight)
#endif
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // my own reads of chunk c have returned ...
            __builtin_amdgcn_s_barrier();                          // ... and everyone's: stage `st` is free
#ifdef DMAP_ABL_NOFRAG
            asm volatile("" : "+v"(f0.ah[0]), "+v"(f0.al[0]), "+v"(f0.ah[1]), "+v"(f0.al[1]));
            asm volatile("" : "+v"(f0.bh[0]), "+v"(f0.bl[0]), "+v"(f0.bh[1]), "+v"(f0.bl[1]), "+v"(f0.bh[2]), "+v"(f0.bl[2]), "+v"(f0.bh[3]), "+v"(f0.bl[3]));
#else
            load_frag(f0, st ^ 1, 0);
#endif
        }
        unsigned o0 = ox[0], o1 = ox[1], o2 = ox[2], o3 = ox[3];
        if (go && reclamp) { o0 = x_offset(0, nrow0); o1 = x_offset(1, nrow0); o2 = x_offset(2, nrow0); o3 = x_offset(3, nrow0); }
        mma_pair(f1, 0, 0); __builtin_amdgcn_sched_barrier(0);
        if constexpr (go) { dma_x(xb, o0, cc, st, 0); dma_x(xb, o1, cc, st, 1); }
        __builtin_amdgcn_sched_barrier(0);
        mma_pair(f1, 0, 2); __builtin_amdgcn_sched_barrier(0);
        if constexpr (go) { dma_x(xb, o2, cc, st, 2); dma_x(xb, o3, cc, st, 3); }
        __builtin_amdgcn_sched_barrier(0);
        mma_pair(f1, 1, 0); __builtin_amdgcn_sched_barrier(0);
        if constexpr (go) { dma_w(wb, cc, st, 0); dma_w(wb, cc, st, 1); }
        __builtin_amdgcn_sched_barrier(0);
        mma_pair(f1, 1, 2); __builtin_amdgcn_sched_barrier(0);
        if constexpr (go) { dma_w(wb, cc, st, 2); dma_w(wb, cc, st, 3); }
        __builtin_amdgcn_sched_barrier(0);
    };
    typedef std::integral_constant<int, 1> Yes;
    typedef std::integral_constant<int, 0> No;

    // ---- first tile: chunk 0 in flight ----
    int lin = tl.first;
    if constexpr (POOL) {
        lin = pool_run_first_tile(run_u, p.tiles_n, q->run);
        run_left = pool_run_count(run_u, tiles_m, p.tiles_n, q->run) - 1;
    }
    // POOL: the running (max, min) pair of every thread, in LDS ([max | min][thread][NT]: a thread's NT values are one 16-byte
    // access, its address one shift of the thread id -- nothing of it is kept in a register over the K loop); `rseg`: the mesh the
    // wave's pair belongs to, -1 = the pair is empty (wave-uniform); `drained`: this wave has waited for all its DMAs so far
    static_assert(NT == 4 && PAIR == 2 * 4 * 64, "the pair is kept as two 16-byte vectors per thread");
    auto pair_ptr = [&](int t) __attribute__((always_inline)) { return reinterpret_cast<f32x4*>(smem + 2 * STAGE) + t; };   // max; min: + 512
    int rseg = -1;
    bool drained = true;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    if constexpr (POOL) {
        pair_ptr(tid)[0] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        pair_ptr(tid)[512] = f32x4{INFINITY, INFINITY, INFINITY, INFINITY};
    }
    int g = 0;                                  // stream position of the current tile's chunk 0: chunk c lives in stage (g + c) & 1
    {
        const int row0 = (lin / p.tiles_n) * BM;
        const char* xbase = reinterpret_cast<const char*>(p.X + (size_t)row0 * p.ldx);
        const char* wbase = reinterpret_cast<const char*>(p.W + (size_t)((lin % p.tiles_n) * BN) * p.ldw);
#pragma unroll
        for (int j = 0; j < XJ; ++j) dma_x(xbase, x_offset(j, row0), 0, 0, j);
#pragma unroll
        for (int j = 0; j < WJ; ++j) dma_w(wbase, 0, 0, j);
    }
    bool slow_cur = false, slow_next = false;    // POOL = false: does the current / next tile span several meshes (row bias per row)?
    if constexpr (!POOL) { panel_fetch(lin, slow_cur); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (!POOL) { panel_write(0); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

#pragma unroll 1
    for (int jt = 0; jt < n_my; ++jt) {
        const int tn = lin % p.tiles_n, row0 = (lin / p.tiles_n) * BM;
        const char* xbase = reinterpret_cast<const char*>(p.X + (size_t)row0 * p.ldx);
        const char* wbase = reinterpret_cast<const char*>(p.W + (size_t)(tn * BN) * p.ldw);
#pragma unroll
        for (int j = 0; j < XJ; ++j) ox[j] = x_offset(j, row0);
        bool run_end = true;                     // POOL: this is the last tile of its run

        if constexpr (POOL) {
            // Which wait covers which DMA: this tile's chunk 0 was issued in the previous tile's second-to-last chunk and is the
            // only DMA of this wave that can still be in flight here (that tile's own chunks were waited for inside its K loop). A
            // tile whose epilogue flushed or took the per-element path has waited for it already, IN FRONT of its atomics (vmcnt
            // retires in order: behind them the wait would cover the atomics too); the common tile issues no global access at all
            // in its epilogue and waits here. The barrier then makes "my chunk 0 pieces landed" true of every wave.
            if (!drained) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            drained = false;
        }
        __builtin_amdgcn_s_barrier();            // chunk 0 landed for everyone; this tile's panel is visible
#pragma unroll
        for (int j = 0; j < XJ; ++j) dma_x(xbase, ox[j], 1, (g + 1) & 1, j);          // chunk 1: the usual prologue slot
#pragma unroll
        for (int j = 0; j < WJ; ++j) dma_w(wbase, 1, (g + 1) & 1, j);
        if constexpr (POOL) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = acc_zero();
        } else {
            // accumulators start at bias (+ row bias): register r of tile nt is column 32 nt + (r & 3) + 8 (r >> 2) + 4 hi
            const float* pn = pan + (jt & 1) * PANEL + wn * NT * 32 + 4 * hi;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const f32x16 v = acc_from_panel(pn, nt);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = v;
            }
        }
        load_frag(f0, g & 1, 0);

#pragma unroll 1
        for (int c = 0; c + 2 < nchunk; ++c) chunk_iter((g + c) & 1, Yes{}, Yes{}, xbase, wbase, c + 2, false, 0);
        {
            // the second-to-last chunk's slot fetches chunk 0 of the NEXT tile of the list (at the end of the list this tile's
            // own chunk 0 once more: never read); rows past M are clamped
            int nlin = jt + 1 < n_my ? lin + nbx : lin;
            if constexpr (POOL) {
                // the next row tile of the run, or the first tile of the workgroup's next run
                run_end = run_left == 0;
                if (!run_end) { nlin = lin + p.tiles_n; --run_left; }
                else if (jt + 1 < n_my) {
                    asm volatile("" : "+s"(q));
                    const int R = q->run;
                    run_u += nbx;
                    nlin = pool_run_first_tile(run_u, p.tiles_n, R);
                    run_left = pool_run_count(run_u, tiles_m, p.tiles_n, R) - 1;
                }
            }
            const int nrow0 = (nlin / p.tiles_n) * BM;
            const char* nxbase = reinterpret_cast<const char*>(p.X + (size_t)nrow0 * p.ldx);
            const char* nwbase = reinterpret_cast<const char*>(p.W + (size_t)((nlin % p.tiles_n) * BN) * p.ldw);
            // the next tile's column constants: requested two chunks ahead of the epilogue's stores (vmcnt retires in order, so
            // a load issued behind the stores could only be waited for together with them)
            if constexpr (!POOL) panel_fetch(nlin, slow_next);
            chunk_iter((g + nchunk - 2) & 1, Yes{}, Yes{}, nxbase, nwbase, 0, true, nrow0);
            chunk_iter((g + nchunk - 1) & 1, No{}, No{}, nxbase, nwbase, 0, false, 0);
            lin = nlin;
        }

        // ---- tile done. Store launches: chunk 0 of the next tile must have landed BEFORE the epilogue issues stores (vmcnt is in
        // order). Pooled launches: only in front of a flush or a per-element tile (`drain`); see the top of the tile loop ----
        if constexpr (!POOL) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const int colw0 = tn * BN + wn * NT * 32;
        if constexpr (POOL) {
            // thread ids of the epilogue: the lane from mbcnt, the wave from a scalar, so that none of them is one more vector register
            // kept (or spilled: a scratch reload is waited for with vmcnt(0)) over the K loop; first row / column are scalars
            const int elane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), ewave = wave_s;
            const int te = ewave * 64 + elane;
            const int ecolw0 = tn * BN + (ewave % WNW) * NT * 32;
            const int rfirst = row0 + (ewave / WNW) * 64;                            // (wave-uniform: the mesh ids are scalar loads)
            f32x4* const pair_mx = pair_ptr(te);
            f32x4* const pair_mn = pair_mx + 512;
            auto drain = [&]() __attribute__((always_inline)) {
                if (!drained) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); drained = true; }
            };
            auto load_pe = [&](GemmDmaParams& pe) __attribute__((always_inline)) {
                asm volatile("" : "+s"(q));      // field by field: scalar loads from the kernarg segment (a memcpy becomes VMEM loads)
                pe.M = q->M; pe.N = q->N; pe.bias = q->bias; pe.scale = q->scale; pe.shift = q->shift; pe.relu = q->relu; pe.seg = q->seg;
                pe.pool = q->pool; pe.ld_pool = q->ld_pool;
            };
            // the running pair leaves: half-wave exchange, column constants, transform, one atomic per column (pool_epilogue.h)
            auto flush = [&]() __attribute__((always_inline)) {
                drain();
                GemmDmaParams pe;
                load_pe(pe);
                const f32x4 vx = *pair_mx, vn = *pair_mn;
                const float mx[NT] = {vx[0], vx[1], vx[2], vx[3]}, mn[NT] = {vn[0], vn[1], vn[2], vn[3]};
                pool_flush<NT>(pe, rseg, ecolw0, elane, mx, mn);
                *pair_mx = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                *pair_mn = f32x4{INFINITY, INFINITY, INFINITY, INFINITY};
                rseg = -1;
            };
            int s0 = -1;
            const bool whole = pool_slab_is_uniform(p, rfirst, s0);                  // all 64 rows < M and in one mesh
            if (rseg >= 0 && !(whole && s0 == rseg)) flush();                        // the mesh in front of this slab is complete
            if (whole) {
                const f32x4 vx = *pair_mx, vn = *pair_mn;
                float mx[NT] = {vx[0], vx[1], vx[2], vx[3]}, mn[NT] = {vn[0], vn[1], vn[2], vn[3]};
                pool_reduce_rows<MT, NT>(acc, mx, mn);
                *pair_mx = f32x4{mx[0], mx[1], mx[2], mx[3]};
                *pair_mn = f32x4{mn[0], mn[1], mn[2], mn[3]};
                rseg = s0;
            } else if (rfirst < p.M) {
                // a slab that holds rows of several meshes, or row M: the per-element path (the pair is empty here)
                drain();
                GemmDmaParams pe;
                load_pe(pe);
                pool_tile_per_element<MT, NT>(pe, acc, rfirst, ecolw0, elane);
            }
            if (run_end && rseg >= 0) flush();
        } else {
            panel_write((jt + 1) & 1);           // the next tile's panel (its loads returned with the vmcnt(0) above); published by the
                                                 // barrier at the top of the next tile. This tile's panel: parity jt & 1
            asm volatile("" : "+s"(q));
            GemmDmaParams pe;
            pe.M = q->M; pe.N = q->N; pe.scale = q->scale; pe.relu = q->relu;
            pe.rowbias = q->rowbias; pe.ld_rowbias = q->ld_rowbias; pe.seg = q->seg;
            pe.Y = q->Y; pe.ldy = q->ldy; pe.y16 = q->y16; pe.ovf = q->ovf; pe.dbg = q->dbg;
            const float* pn = pan + (jt & 1) * PANEL;
            if (!(pe.dbg & 1))
                store_tile_regs<MT, NT>(pe, acc, pe.scale ? pn + BN : nullptr, pn + 2 * BN, wm * 64, row0, pe.M, colw0, wn * NT * 32, lane,
                                        slow_cur);
            slow_cur = slow_next;
        }
        g += nchunk;                             // the next tile's chunk 0 sits in stage (g + nchunk) & 1
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no LDS-DMA may outlive the workgroup
#endif
}

int launch_gemm16_dmap(const GemmDmaParams& p0, hipStream_t s) {
    GemmDmaParams p = p0;
    p.dbg = debug_flags();
    p.tiles_n = p.N / 256;
    const int T = cdiv(p.M, 256) * p.tiles_n;
    const int grid = persistent_grid(T);
    // pooled launches: runs of 16 (= the row tiles of a 4096-vertex mesh) consecutive row tiles of one column block, halved until every
    // workgroup gets at least two runs. MORIG_POOL_RUN=<R> FORCES the run length instead (rounded down to a power of two, at most 256,
    // not halved: short launches then leave workgroups without a run); 1 = a run is a tile, the list of the store launches
    const int run_env = switches().pool_run;
    if (!p.pool) p.run = 1;
    else if (run_env > 0) p.run = pool_run_length(cdiv(p.M, 256), p.tiles_n, 0, run_env);
    else p.run = pool_run_length(cdiv(p.M, 256), p.tiles_n, grid, 16);
    if (p.pool) hipLaunchKernelGGL(gemm16_dmap_kernel<true>, dim3(grid), dim3(512), 0, s, p);
    else        hipLaunchKernelGGL(gemm16_dmap_kernel<false>, dim3(grid), dim3(512), 0, s, p);
    MORIG_LAUNCH_CHECK();
    return MORIG_OK;
}

}  // namespace morig
