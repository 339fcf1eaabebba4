// The segment lookup and the workgroup layout of a ragged batch: rows of B segments are concatenated and delimited by a prefix sum
// ptr[B + 1] that ascends from 0; segment b owns the rows [ptr[b], ptr[b + 1]), so an empty segment owns no row. Plain C++ without a
// HIP construct, so that the kernels and tools/ragged_host_check.cpp (built with the host sanitizers, run by tests/test_ragged.py)
// compile the SAME text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORIG_RAGGED_HD __host__ __device__ __forceinline__
#else
#define MORIG_RAGGED_HD inline
#endif

namespace morig {

// The last b in [0, n) with ptr[b] <= i; 0 when n <= 1 or no such b exists. Reads ptr[1 .. n - 1] only, never ptr[n]. P is int32_t or
// int64_t, I is int or a 64-bit integer: the comparison is made in 64 bits, nothing narrows. For an ascending ptr and ptr[0] <= i < ptr[n]
// the result is THE segment that owns row i. Where a bad ptr or an i outside the batch is possible, the caller checks
// ptr[b] <= i < ptr[b + 1] on the result: the search itself ends after at most log2(n) steps on any input.
template <class P, class I> MORIG_RAGGED_HD int segment_of(const P* ptr, int n, I i) {
    static_assert((P)-1 < (P)0 && (I)-1 < (I)0, "segment_of: signed tables and indices (cast blockIdx / threadIdx at the call)");
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)ptr[mid] <= (int64_t)i) lo = mid; else hi = mid;
    }
    return lo;
}

// Where a thread of a kernel whose workgroups are laid out over the segments by blk_ptr stands (morig_amd/ragged.py blocks() makes the
// table: segment b has ceil(rows(b) / width) workgroups of width rows, blk_ptr is their prefix sum). row is local to seg and computed in
// 64 bits; the caller's liveness test is 0 <= row < rows(seg), which also refuses a workgroup that a bad blk_ptr puts in front of its
// segment (row < 0). Reads blk_ptr[1 .. n_segs - 1] and blk_ptr[seg].
struct BlockRow { int seg; long long row; };
template <class P> MORIG_RAGGED_HD BlockRow block_row(const P* blk_ptr, int n_segs, int block, int thread, int width) {
    const int seg = segment_of(blk_ptr, n_segs, block);
    return {seg, ((long long)block - (long long)blk_ptr[seg]) * width + thread};
}

}  // namespace morig
