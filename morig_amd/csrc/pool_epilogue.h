// Pooled epilogue shared by the LDS-DMA GEMMs (gemm_dmap.hip POOL launches, gemm_dma.hip `!TR && pool`): column max per mesh of
// f(a) = relu(a + bias) * scale + shift over the rows of a wave's MT x NT accumulator tiles (a lane owns a COLUMN; layout as in
// epilogue_store.h), combined across waves and workgroups by atomic_max_f32.
//
// f is monotone in a -- non-decreasing where the column's scale is >= 0, non-increasing where it is < 0 -- and so is every
// rounded step it is made of (add, max with 0, multiply-add by a constant). So max_rows f(a) == f(max_rows a) for scale >= 0 and
// f(min_rows a) for scale < 0, BIT FOR BIT: the rows are reduced RAW, one v_max3_f32 and one v_min3_f32 per two elements, into a
// (max, min) pair per lane and column; the pair can keep running over any number of tiles of the same mesh (pool_runs.h); a FLUSH
// joins the two half-waves, reads the column constants (the only global loads), applies f once per column and issues the atomic.
// (NaN accumulators -- which the guarded inputs exclude -- are the one case where the two orders differ: the raw max drops them.)
// What the argument does not cover takes the per-element path, which is the code both kernels had before: a 64-row slab that
// holds rows of several meshes, or rows >= M (their accumulators come from clamped DMA sources).
#pragma once
#include "common.h"

namespace morig {

__device__ __forceinline__ float pool_transform(float a, float b, float sc, float shf, int relu) {
    float v = a + b;
    if (relu) v = v > 0.f ? v : 0.f;
    v = v * sc + shf;
    return v;
}

template <int NT> __device__ __forceinline__ void pool_pair_identity(float (&mx)[NT], float (&mn)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { mx[nt] = -INFINITY; mn[nt] = INFINITY; }
}

// merge the raw max / min over all 32 MT rows this lane holds of each of its NT columns into the running pair
template <int MT, int NT>
__device__ __forceinline__ void pool_reduce_rows(const f32x16 (&acc)[MT][NT], float (&mx)[NT], float (&mn)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        float a = mx[nt], i = mn[nt];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float x = acc[mt][nt][r], y = acc[mt][nt][r + 1];
                asm("v_max3_f32 %0, %1, %2, %0" : "+v"(a) : "v"(x), "v"(y));
                asm("v_min3_f32 %0, %1, %2, %0" : "+v"(i) : "v"(x), "v"(y));
            }
        mx[nt] = a; mn[nt] = i;
    }
}

// P: N, bias, scale, shift, relu, pool, ld_pool. All rows behind the pair belong to mesh `sg`; colw0: first column of the wave tile.
// The two half-waves hold different rows of the same columns: one exchange, then lanes 0..31 issue the atomics.
template <int NT, class P>
__device__ __forceinline__ void pool_flush(const P& p, int sg, int colw0, int lane, const float (&mx)[NT], const float (&mn)[NT]) {
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = colw0 + nt * 32 + l31;
        const bool cok = col < p.N;
        const float b = (p.bias && cok) ? p.bias[col] : 0.f;
        const float sc = (p.scale && cok) ? p.scale[col] : 1.f;
        const float shf = (p.shift && cok) ? p.shift[col] : 0.f;
        const float a = fmaxf(mx[nt], __shfl_xor(mx[nt], 32, 64));
        const float i = fminf(mn[nt], __shfl_xor(mn[nt], 32, 64));
        const float m = pool_transform(sc < 0.f ? i : a, b, sc, shf, p.relu);
        if (hi == 0 && cok && m > -INFINITY) atomic_max_f32(p.pool + (size_t)sg * p.ld_pool + col, m);
    }
}

// The per-element path. P: the above + M, seg. rfirst < M: global row of the wave tile's first row.
template <int MT, int NT, class P>
__device__ __forceinline__ void pool_tile_per_element(const P& p, const f32x16 (&acc)[MT][NT], int rfirst, int colw0, int lane) {
    const int l31 = lane & 31, hi = lane >> 5;
    const int rlast = min(rfirst + 63, p.M - 1);
    const int s0 = p.seg[rfirst];
    const bool uni = s0 == p.seg[rlast];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = colw0 + nt * 32 + l31;
        const bool cok = col < p.N;
        const float b = (p.bias && cok) ? p.bias[col] : 0.f;
        const float sc = (p.scale && cok) ? p.scale[col] : 1.f;
        const float shf = (p.shift && cok) ? p.shift[col] : 0.f;
        float m = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rfirst + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const float v = pool_transform(acc[mt][nt][r], b, sc, shf, p.relu);
                if (row < p.M) {
                    if (uni) m = fmaxf(m, v);
                    else if (cok) atomic_max_f32(p.pool + (size_t)p.seg[row] * p.ld_pool + col, v);
                }
            }
        if (uni) {
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            if (hi == 0 && cok && m > -INFINITY) atomic_max_f32(p.pool + (size_t)s0 * p.ld_pool + col, m);
        }
    }
}

// does the raw reduction cover the wave tile that starts at row rfirst? (all 64 rows < M and in one mesh: `seg` is sorted)
// `seg` is read through the constant address space -- nothing writes it while the kernel runs --, so that a wave-uniform rfirst
// makes these scalar loads: a vector load here would be waited for with vmcnt(0), together with every LDS-DMA in flight.
template <class P> __device__ __forceinline__ bool pool_slab_is_uniform(const P& p, int rfirst, int& sg) {
    typedef __attribute__((address_space(4))) const int* const_int_ptr;
    if (rfirst + 63 >= p.M) return false;
    const_int_ptr seg = (const_int_ptr)p.seg;
    sg = seg[rfirst];
    return sg == seg[rfirst + 63];
}

// one wave tile that is pooled on its own (gemm_dma.hip: one tile per workgroup)
template <int MT, int NT, class P>
__device__ __forceinline__ void pool_tile(const P& p, const f32x16 (&acc)[MT][NT], int rfirst, int colw0, int lane) {
    int sg = 0;
    if (pool_slab_is_uniform(p, rfirst, sg)) {
        float mx[NT], mn[NT];
        pool_pair_identity<NT>(mx, mn);
        pool_reduce_rows<MT, NT>(acc, mx, mn);
        pool_flush<NT>(p, sg, colw0, lane, mx, mn);
    } else {
        pool_tile_per_element<MT, NT>(p, acc, rfirst, colw0, lane);
    }
}

}  // namespace morig
