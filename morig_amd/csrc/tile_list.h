// Static work lists of the persistent kernels (edge_pp.hip, edge_ws.hip, edge_rl.hip, gemm_dmap.hip; pool_runs.h builds on it).
//
// n items (tiles, or runs of tiles) are dealt to 8 XCDs x the owners of each XCD -- an owner is a workgroup (block >> 3 of grid >> 3;
// XCD = block & 7 under round-robin dispatch) or, in edge_rl.hip, one of its 8 waves. XCD x owns the contiguous slice
// [n x / 8, n (x + 1) / 8); owner i of it takes items lo + i, lo + i + owners, ...: neighbours work on neighbouring items at the same
// time and share that XCD's L2. RUN form: T tiles are cut into runs of R = 2^lg consecutive tiles (the last may be shorter), the runs
// are the items dealt and an owner walks its runs tile by tile.
// Plain C++ on purpose (host and device): tools/tile_list_host_check.cpp enumerates every list on the host. The expressions are
// spelled, and ordered, as the kernels had them inline: the kernels sit at their register limits and compile to the same
// instructions as before only with these forms, so a rewrite here needs the assembly comparison again.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MORIG_TILE_HD __host__ __device__ __forceinline__
#else
#define MORIG_TILE_HD inline
#endif

namespace morig {

struct TileList { int first, end, stride; };             // items first, first + stride, ... below end

// the slice of XCD x: [xcd_slice_lo(n, x), xcd_slice_lo(n, x + 1))
MORIG_TILE_HD int xcd_slice_lo(int n, int xcd) { return (int)((long long)n * xcd / 8); }
// workgroup `bi` of the XCD's nbx (nsub = 1), or wave `sub` of that workgroup's nsub waves
MORIG_TILE_HD TileList tile_list(int n, int xcd, int bi, int nbx, int sub = 0, int nsub = 1) {
    const int lo = xcd_slice_lo(n, xcd), hi = xcd_slice_lo(n, xcd + 1);
    const int owner = bi * nsub + sub, nown = nbx * nsub;
    return TileList{lo + owner, hi, nown};
}
MORIG_TILE_HD int tile_list_count(const TileList& l) { return (l.stride - 1 + l.end - l.first) / l.stride; }   // <= 0: none
// item j of an owner with `count` > 0 items; j >= count repeats the last one (the kernels prefetch past the end of their list)
MORIG_TILE_HD int tile_list_item(const TileList& l, int count, int j) { return l.first + (j < count ? j : count - 1) * l.stride; }

// RUN form: T tiles cut into runs of R = 2^lg (run lengths are powers of two, anything else is rounded down); the NR runs are the
// items that tile_list() deals
struct RunCut { int lg, R, NR; };
MORIG_TILE_HD int tile_min(int a, int b) { return a < b ? a : b; }
MORIG_TILE_HD RunCut run_cut(int T, int run) {
    RunCut c;
    c.lg = 31 - __builtin_clz(run > 0 ? run : 1);
    c.R = 1 << c.lg;
    c.NR = (T + c.R - 1) >> c.lg;
    return c;
}
// tiles of an owner with nruns > 0 runs: whole runs, the last one cut at T
MORIG_TILE_HD int run_tiles(const RunCut& c, const TileList& runs, int nruns, int T) {
    return ((nruns - 1) << c.lg) + tile_min(c.R, T - ((runs.first + (nruns - 1) * runs.stride) << c.lg));
}
// tile j of the owner's n_my; j >= n_my repeats the last one
MORIG_TILE_HD int run_tile(const RunCut& c, const TileList& runs, int n_my, int j) {
    const int jj = j < n_my ? j : n_my - 1;
    return ((runs.first + (jj >> c.lg) * runs.stride) << c.lg) + (jj & (c.R - 1));
}

}  // namespace morig
