// The work lists of the persistent kernels (morig_amd/csrc/tile_list.h) as a plain host program, so that the text the kernels compile
// can be enumerated under the address and undefined-behaviour sanitizers: tests/test_tile_list.py builds it with
// -fsanitize=address,undefined and runs it as a program. Never loaded into Python, never run on a GPU machine.
//
// The four lists, walked exactly as their kernels walk them:
//   pp    edge_pp.hip (and edge_ws.hip's WS_OLD_MAP build): tiles dealt to workgroups, tile_of(j) = tile_list_item
//   dmap  gemm_dmap.hip store launches: tiles dealt to workgroups, walked as lin = first, lin += stride
//   ws    edge_ws.hip: runs of 2^lg tiles dealt to workgroups, tile_of(j) = run_tile
//   rl    edge_rl.hip: runs dealt to the 8 waves of every workgroup
// For every tile count 0..300, grid 8..64 (multiples of 8) and, where the list has runs, run length 1, 2, 4, 8: every tile is visited
// exactly once; tile_of(j >= n_my) repeats the last tile; the tiles of a run are consecutive and stay with one owner.
// Prints "ok <combinations>" or the first violation (exit status 1).
#include "../morig_amd/csrc/tile_list.h"
#include "../morig_amd/csrc/pool_runs.h"
#include <cstdio>
#include <vector>

using namespace morig;

static int fail(const char* list, int T, int grid, int R, const char* what, int a, int b) {
    std::printf("%s T %d grid %d run %d: %s (%d, %d)\n", list, T, grid, R, what, a, b);
    return 1;
}

static int every_tile_once(const char* list, int T, int grid, int R, const std::vector<int>& seen) {
    for (int t = 0; t < T; ++t)
        if (seen[t] != 1) return fail(list, T, grid, R, "tile visited other than once", t, seen[t]);
    return 0;
}

// tiles dealt to workgroups: the clamped tile_of of edge_pp.hip, and gemm_dmap.hip's walk by stride
static int check_tiles(int T, int grid) {
    std::vector<int> seen_pp(T, 0), seen_dmap(T, 0);
    for (int block = 0; block < grid; ++block) {
        const TileList tl = tile_list(T, block & 7, block >> 3, grid >> 3);
        const int n_my = tile_list_count(tl);
        if (n_my <= 0) continue;                                               // the kernels return here
        int lin = tl.first;
        for (int j = 0; j < n_my; ++j, lin += tl.stride) {
            const int t = tile_list_item(tl, n_my, j);
            if (t < 0 || t >= T) return fail("pp", T, grid, 1, "tile outside the launch", block, t);
            if (t != lin) return fail("dmap", T, grid, 1, "the walk by stride leaves the list", block, lin);
            ++seen_pp[t]; ++seen_dmap[lin];
        }
        const int last = tile_list_item(tl, n_my, n_my - 1);
        for (int j = n_my; j < n_my + 9; ++j)
            if (tile_list_item(tl, n_my, j) != last) return fail("pp", T, grid, 1, "tile_of past the end is not the last tile", block, j);
        // the pooled GEMM's run list at run length 1 is this list
        int first, end, stride;
        pool_wg_runs(T, grid, block, first, end, stride);
        if (first != tl.first || end != tl.end || stride != tl.stride) return fail("dmap", T, grid, 1, "pool_wg_runs disagrees", block, first);
    }
    if (every_tile_once("pp", T, grid, 1, seen_pp)) return 1;
    return every_tile_once("dmap", T, grid, 1, seen_dmap);
}

// runs dealt to workgroups (nsub = 1, edge_ws.hip) or to their waves (nsub = 8, edge_rl.hip)
static int check_runs(const char* list, int T, int grid, int run, int nsub) {
    const RunCut rc = run_cut(T, run);
    if (rc.R != run || (1 << rc.lg) != rc.R || rc.NR != (T + run - 1) / run) return fail(list, T, grid, run, "run_cut", rc.R, rc.NR);
    std::vector<int> seen(T, 0), run_owner(rc.NR, -1);
    for (int block = 0; block < grid; ++block)
        for (int sub = 0; sub < nsub; ++sub) {
            const int owner = block * nsub + sub;
            const TileList rl = tile_list(rc.NR, block & 7, block >> 3, grid >> 3, sub, nsub);
            const int nruns = tile_list_count(rl);
            if (nruns <= 0) continue;                                          // the kernels return here
            const int n_my = run_tiles(rc, rl, nruns, T);
            if (n_my <= 0 || n_my > nruns * rc.R) return fail(list, T, grid, run, "n_my", owner, n_my);
            int prev = -1;
            for (int j = 0; j < n_my; ++j) {
                const int t = run_tile(rc, rl, n_my, j);
                if (t < 0 || t >= T) return fail(list, T, grid, run, "tile outside the launch", owner, t);
                const int u = t >> rc.lg;
                if (run_owner[u] >= 0 && run_owner[u] != owner) return fail(list, T, grid, run, "a run is shared by two owners", u, owner);
                run_owner[u] = owner;
                if ((j & (rc.R - 1)) != 0 && (t != prev + 1 || (prev >> rc.lg) != u))
                    return fail(list, T, grid, run, "the tiles of a run are not consecutive", owner, j);
                if ((j & (rc.R - 1)) == 0 && (t & (rc.R - 1)) != 0) return fail(list, T, grid, run, "a run does not start at its first tile", owner, j);
                ++seen[t]; prev = t;
            }
            for (int j = n_my; j < n_my + 9; ++j)
                if (run_tile(rc, rl, n_my, j) != prev) return fail(list, T, grid, run, "tile_of past the end is not the last tile", owner, j);
        }
    return every_tile_once(list, T, grid, run, seen);
}

int main() {
    long checked = 0;
    for (int T = 0; T <= 300; ++T)
        for (int grid = 8; grid <= 64; grid += 8) {
            if (check_tiles(T, grid)) return 1;
            ++checked;
            for (int run = 1; run <= 8; run *= 2) {
                if (check_runs("ws", T, grid, run, 1) || check_runs("rl", T, grid, run, 8)) return 1;
                checked += 2;
            }
        }
    // a run length that is no power of two is rounded down, none means 1
    if (run_cut(100, 3).R != 2 || run_cut(100, 0).R != 1 || run_cut(100, -5).R != 1 || run_cut(100, 9).R != 8) return fail("cut", 100, 0, 3, "rounding", 0, 0);
    std::printf("ok %ld\n", checked);
    return 0;
}
