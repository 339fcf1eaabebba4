// Tile list of the pooled persistent GEMM (gemm_dmap.hip, POOL launches): RUNS of consecutive row tiles of one column block.
//
// A launch has tiles_m row tiles (256 rows) x tiles_n column blocks (256 columns). Rows are cut into groups of R consecutive row
// tiles (the last group may be shorter); a RUN is one group x one column block, numbered u = group * tiles_n + column block, so
// the tiles_n runs over the same rows are neighbours. The U runs are dealt to the workgroups as tile_list.h deals any items (a
// contiguous slice per XCD, strided inside it): adjacent workgroups of an XCD work on the same rows at the same time and share X in
// that XCD's L2. Inside a run a workgroup walks row tiles first .. first + count - 1 of its column block and keeps the running column
// maximum across them (pool_epilogue.h). R = 1: a run is a tile, u is the row-major linear tile id -- the list the store launches
// use. Plain C++ on purpose (host and device): tests/test_gpu_pooled_runs.py compiles it into a stand-alone checker.
#pragma once
#include "tile_list.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MORIG_POOL_HD __host__ __device__ inline
#else
#define MORIG_POOL_HD inline
#endif

namespace morig {

MORIG_POOL_HD int pool_run_units(int tiles_m, int tiles_n, int R) { return ((tiles_m + R - 1) / R) * tiles_n; }

// the runs of workgroup `block` of a grid of `grid` (a multiple of 8): first, first + stride, ... below end
MORIG_POOL_HD void pool_wg_runs(int units, int grid, int block, int& first, int& end, int& stride) {
    const int xcd = block & 7, bi = block >> 3;
    stride = grid >> 3;
    first = xcd_slice_lo(units, xcd) + bi;
    end = xcd_slice_lo(units, xcd + 1);
}

MORIG_POOL_HD int pool_run_col_block(int u, int tiles_n) { return u % tiles_n; }
MORIG_POOL_HD int pool_run_first_row_tile(int u, int tiles_n, int R) { return (u / tiles_n) * R; }
MORIG_POOL_HD int pool_run_count(int u, int tiles_m, int tiles_n, int R) {
    const int left = tiles_m - pool_run_first_row_tile(u, tiles_n, R);
    return left < R ? left : R;
}
// row-major linear id (row tile * tiles_n + column block) of a run's first tile; the next tile of the run is + tiles_n
MORIG_POOL_HD int pool_run_first_tile(int u, int tiles_n, int R) {
    return pool_run_first_row_tile(u, tiles_n, R) * tiles_n + pool_run_col_block(u, tiles_n);
}

// all tiles of a workgroup's runs
MORIG_POOL_HD int pool_wg_tiles(int tiles_m, int tiles_n, int R, int grid, int block) {
    int first, end, stride, n = 0;
    pool_wg_runs(pool_run_units(tiles_m, tiles_n, R), grid, block, first, end, stride);
    if (R == 1) return first < end ? (end - first + stride - 1) / stride : 0;
    for (int u = first; u < end; u += stride) n += pool_run_count(u, tiles_m, tiles_n, R);
    return n;
}

// run length of a launch: the largest power of two <= r_max at which every workgroup still gets at least two runs (a workgroup
// with one long run would leave the end of the launch to the slowest XCD); 1 when there are too few tiles for that.
// grid = 0: the largest power of two <= r_max, whatever the launch (a forced run length)
MORIG_POOL_HD int pool_run_length(int tiles_m, int tiles_n, int grid, int r_max) {
    int R = 1;
    while (R * 2 <= r_max) R *= 2;
    const int nbx = grid >> 3;
    if (nbx <= 0) return R;
    while (R > 1 && (pool_run_units(tiles_m, tiles_n, R) / 8) / nbx < 2) R >>= 1;
    return R;
}

}  // namespace morig
