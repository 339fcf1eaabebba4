// The sequential logic of the joint matching (csrc/metrics.hip): shortest augmenting paths with dual potentials on a rectangular cost
// matrix, the algorithm behind scipy.optimize.linear_sum_assignment (D. F. Crouse, "On implementing 2D rectangular assignment
// algorithms", IEEE Trans. Aerospace and Electronic Systems 52(4), 2016). Plain C++ without a HIP construct, so that the kernel and
// tools/assign_host_check.cpp (built with the host sanitizers, run by tests/test_metrics_host.py) compile the SAME text.
//
// The work of one problem is shared by `Lanes`: lane l owns the columns j = l, l + count, ... -- their shortest[], path[] and in_SC[]
// entries are written by the owner only, so the scan loop of an augmentation needs no barrier, just Lanes::min. The kernel's Lanes is one
// wave of 64; the host program's is a single lane with an empty sync.
//
// Orientation: the solver wants rows <= columns. A caller's n_rows x n_cols matrix with more rows than columns is solved transposed
// (solver_index says where an entry goes); emit() returns pairs in the caller's orientation, rows ascending, as scipy does.
//
// Ties: among columns of equal reduced cost an unassigned one wins, then the lowest index. scipy walks its `remaining` list instead, so on a
// matrix with several optima the two may return different -- equally optimal -- matchings.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MORIG_ASSIGN_HD __host__ __device__ inline
#else
#define MORIG_ASSIGN_HD inline
#endif

namespace morig_assign {

constexpr int MAX_SMALL = 128;            // MORIG_ASSIGN_MAX_SMALL: the smaller side
constexpr int MAX_LARGE = 256;            // MORIG_ASSIGN_MAX_LARGE: the larger side

MORIG_ASSIGN_HD bool transposed(int n_rows, int n_cols) { return n_cols < n_rows; }
MORIG_ASSIGN_HD bool supported(int n_rows, int n_cols) {
    const int small = n_rows < n_cols ? n_rows : n_cols, large = n_rows < n_cols ? n_cols : n_rows;
    return small >= 0 && small <= MAX_SMALL && large <= MAX_LARGE;
}
// entry (r, c) of the caller's matrix in the solver's row-major matrix
MORIG_ASSIGN_HD long solver_index(int r, int c, int n_rows, int n_cols) {
    return transposed(n_rows, n_cols) ? (long)c * n_rows + r : (long)r * n_cols + c;
}

struct State {
    double* u;                  // [nr] row potentials
    double* v;                  // [nc] column potentials
    double* shortest;           // [nc] shortest path to column j in the current augmentation
    int* path;                  // [nc] the row that path arrives from
    int* col4row;               // [nr] -1: unassigned
    int* row4col;               // [nc]
    unsigned char* in_SR;       // [nr] rows scanned in the current augmentation
    unsigned char* in_SC;       // [nc] columns scanned
};

struct Best { double val; int key; };         // key = (column is assigned) << 16 | column; the smaller (val, key) wins
MORIG_ASSIGN_HD bool better(const Best& a, const Best& b) { return a.val < b.val || (a.val == b.val && a.key < b.key); }

struct OneLane {
    int lane() const { return 0; }
    int count() const { return 1; }
    void sync() const {}
    Best min(Best b) const { return b; }
};

// cost: nr x nc row-major, nr <= nc. Returns false when no complete assignment of finite cost exists (an infinite or NaN entry in the way).
template <class Lanes> MORIG_ASSIGN_HD bool solve(const double* cost, int nr, int nc, State s, Lanes& L) {
    const double inf = __builtin_huge_val();
    const int lane = L.lane(), W = L.count();
    for (int i = lane; i < nr; i += W) { s.u[i] = 0.0; s.col4row[i] = -1; }
    for (int j = lane; j < nc; j += W) { s.v[j] = 0.0; s.row4col[j] = -1; }
    for (int cur = 0; cur < nr; ++cur) {
        for (int i = lane; i < nr; i += W) s.in_SR[i] = 0;
        for (int j = lane; j < nc; j += W) { s.shortest[j] = inf; s.in_SC[j] = 0; }
        L.sync();
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {                                   // every pass moves one column into SC: at most nc passes
            if (lane == 0) s.in_SR[i] = 1;
            const double ui = s.u[i];
            const double* row = cost + (long)i * nc;
            Best best = {inf, 0x7fffffff};
            for (int j = lane; j < nc; j += W) {
                if (s.in_SC[j]) continue;
                const double r = ((min_val + row[j]) - ui) - s.v[j];
                if (r < s.shortest[j]) { s.path[j] = i; s.shortest[j] = r; }
                const Best mine = {s.shortest[j], (s.row4col[j] >= 0 ? 1 << 16 : 0) | j};
                if (better(mine, best)) best = mine;
            }
            best = L.min(best);
            if (!(best.val < inf)) return false;
            min_val = best.val;
            const int j = best.key & 0xffff;
            if (j % W == lane) s.in_SC[j] = 1;
            if (s.row4col[j] < 0) sink = j; else i = s.row4col[j];
        }
        L.sync();
        // dual update
        for (int r = lane; r < nr; r += W)
            if (s.in_SR[r]) s.u[r] += r == cur ? min_val : min_val - s.shortest[s.col4row[r]];
        for (int j = lane; j < nc; j += W)
            if (s.in_SC[j]) s.v[j] -= min_val - s.shortest[j];
        L.sync();
        // augment along the path that ends in the sink
        if (lane == 0) {
            int j = sink;
            for (int guard = 0; guard <= nr; ++guard) {
                const int r = s.path[j];
                s.row4col[j] = r;
                const int prev = s.col4row[r];
                s.col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        L.sync();
    }
    return true;
}

// the pairs in the caller's orientation: min(n_rows, n_cols) of them, row_ind ascending
template <class Lanes> MORIG_ASSIGN_HD void emit(const State& s, int n_rows, int n_cols, int* row_ind, int* col_ind, Lanes& L) {
    if (!transposed(n_rows, n_cols)) {
        for (int i = L.lane(); i < n_rows; i += L.count()) { row_ind[i] = i; col_ind[i] = s.col4row[i]; }
    } else if (L.lane() == 0) {                              // the solver's columns are the caller's rows
        int k = 0;
        for (int j = 0; j < n_rows && k < n_cols; ++j)
            if (s.row4col[j] >= 0) { row_ind[k] = j; col_ind[k] = s.row4col[j]; ++k; }
    }
    L.sync();
}

}  // namespace morig_assign
