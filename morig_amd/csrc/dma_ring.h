// The split-fp16 LDS-DMA GEMM core shared by gemm_dma.hip (one workgroup per tile) and gemm_dmap.hip (persistent): the pieces that
// must agree between the two for the ring image to mean the same thing. The kernels keep their schedules (prologue, chunk loop,
// where the DMA pieces sit between the MFMA groups, epilogues).
//
// LDS image of a stage: [BM rows][128 B] for X then [BN rows][128 B] for W, a row = [32 hi | 32 lo] halves of one 32-column chunk
// = 8 slots of 16 B. DMA writes are lane-linear (wave base + lane * 16), so the bank-conflict fix is an XOR swizzle applied on the
// SOURCE side (cdna_hip_programming.md rule 21): LDS slot p of row r holds logical slot p ^ ((r >> 1) & 7); fragment reads apply
// the same involution. A 16-lane read group (16 distinct rows mod 16) then hits 16 distinct slots.
#pragma once
#include "mfma_types.h"

namespace morig {

// the operand fragments of one 16-k step of a wave tile of MT x NT 32 x 32 blocks: hi and lo halves of X (a) and of W (b)
template <int MT, int NT> struct SplitFrag { f16x8 ah[MT], al[MT], bh[NT], bl[NT]; };

// 16-k step s2 (0, 1) of the chunk in stage `st`. aoff / boff: byte offsets of this lane's first X / W row in the stage;
// hi = lane >> 5; x7 = ((lane & 31) >> 1) & 7, the swizzle of the lane's rows (rows 32 apart share it)
template <int MT, int NT>
__device__ __forceinline__ void load_split_frag(SplitFrag<MT, NT>& f, const char* st, int aoff, int boff, int s2, int hi, int x7) {
    const int sh = ((2 * s2 + hi) ^ x7) * 16, sl = ((4 + 2 * s2 + hi) ^ x7) * 16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        f.ah[mt] = *reinterpret_cast<const f16x8*>(st + aoff + mt * 32 * 128 + sh);
        f.al[mt] = *reinterpret_cast<const f16x8*>(st + aoff + mt * 32 * 128 + sl);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        f.bh[nt] = *reinterpret_cast<const f16x8*>(st + boff + nt * 32 * 128 + sh);
        f.bl[nt] = *reinterpret_cast<const f16x8*>(st + boff + nt * 32 * 128 + sl);
    }
}

// one split product term: x (a fragment of X) times w (a fragment of W); SWAP exchanges the operand roles (D^T = W X^T: a lane then
// owns an output ROW and groups of 4 adjacent columns -- the register epilogue, epilogue_store.h: store_tile_regs)
template <bool SWAP>
__device__ __forceinline__ void split_mm(const f16x8& x, const f16x8& w, f32x16& c) {
    if constexpr (SWAP) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, x, c, 0, 0, 0);
    else                c = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, w, c, 0, 0, 0);
}
// all MT x NT blocks of one 16-k step: lo * hi, hi * lo, hi * hi (LOHI = false drops x_hi * w_lo: a measurement form)
template <bool SWAP, bool LOHI = true, int MT, int NT>
__device__ __forceinline__ void split_mma(const SplitFrag<MT, NT>& f, f32x16 (&acc)[MT][NT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            split_mm<SWAP>(f.al[mt], f.bh[nt], acc[mt][nt]);
            if constexpr (LOHI) split_mm<SWAP>(f.ah[mt], f.bl[nt], acc[mt][nt]);
            split_mm<SWAP>(f.ah[mt], f.bh[nt], acc[mt][nt]);
        }
}
// one (mt, nt0 .. nt0 + 1) pair of accumulators = 6 MFMAs with the dependent ones two slots apart
template <bool SWAP, bool LOHI = true, int MT, int NT>
__device__ __forceinline__ void split_mma_pair(const SplitFrag<MT, NT>& f, f32x16 (&acc)[MT][NT], int mt, int nt0) {
    split_mm<SWAP>(f.al[mt], f.bh[nt0],     acc[mt][nt0]);
    split_mm<SWAP>(f.al[mt], f.bh[nt0 + 1], acc[mt][nt0 + 1]);
    if constexpr (LOHI) {
        split_mm<SWAP>(f.ah[mt], f.bl[nt0],     acc[mt][nt0]);
        split_mm<SWAP>(f.ah[mt], f.bl[nt0 + 1], acc[mt][nt0 + 1]);
    }
    split_mm<SWAP>(f.ah[mt], f.bh[nt0],     acc[mt][nt0]);
    split_mm<SWAP>(f.ah[mt], f.bh[nt0 + 1], acc[mt][nt0 + 1]);
}

// Byte offset, from the operand's tile base, of the 16-byte piece this lane (physical slot pslot = lane & 7) fetches for tile row r:
// row `src_row` of the source (leading dimension ld floats), logical slot pslot ^ ((r >> 1) & 7). 32 bits: with a block-uniform base
// in SGPRs this is half the address VGPRs of a pointer
__device__ __forceinline__ unsigned dma_piece_offset(int r, int src_row, int ld, int pslot) {
    return ((unsigned)src_row * (unsigned)ld + 4u * (pslot ^ ((r >> 1) & 7))) * 4u;
}
// X pieces of a tile whose first row is row0: rows past M are clamped to the last one (they are never stored)
__device__ __forceinline__ unsigned dma_x_offset(int r, int row0, int M, int ldx, int pslot) {
    const int lslot = pslot ^ ((r >> 1) & 7);
    int xr = r; if (row0 + xr >= M) xr = M - 1 - row0;
    return ((unsigned)xr * (unsigned)ldx + 4u * lslot) * 4u;
}
// one LDS-DMA instruction: 64 lanes x 16 B = 8 rows x 128 B = 1 KiB of 32-column chunk c of the operand whose tile starts at `base`,
// from lane offset o, to lane-linear piece `piece` of the operand's part `st` of a stage
__device__ __forceinline__ void dma_piece(const char* base, int c, unsigned o, char* st, int piece) {
    asm volatile("" : "+v"(o));                  // keep (scalar base + lane offset) addressing
    __builtin_amdgcn_global_load_lds((glb_void_t*)(base + c * 128 + o), (lds_void_t*)(st + piece * 1024), 16, 0, 0);
}

__device__ __forceinline__ f32x16 acc_zero() {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.f;
    return v;
}
// SWAP form: the accumulators start at the bias panel (bias + the row bias of a one-mesh tile): the initial value of the blocks of
// 32-column block nt. pn: the panel entry of the wave's first column + 4 hi; register r is column 32 nt + (r & 3) + 8 (r >> 2) + 4 hi
__device__ __forceinline__ f32x16 acc_from_panel(const float* pn, int nt) {
    f32x16 v;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(pn + nt * 32 + 8 * g4);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[4 * g4 + q] = b4[q];
    }
    return v;
}

}  // namespace morig
