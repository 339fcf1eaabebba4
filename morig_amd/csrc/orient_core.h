// The arithmetic of csrc/meshfix.hip that can go wrong on its own, shared with the host program
// tools/meshfix_host_check.cpp so that it can be checked without a device and under the host sanitizers: the edge record, the shape of a
// run of sorted records, the edge of the double cover, the signed-volume term with its exact negation, and the decision which parity
// class of a component flips. Plain C++ without a HIP construct; float64 in the written order, contraction off (topo_core.h switches it
// off for clang, a host compiler takes -ffp-contract=off). The fold of the lane sums is topo_core.h's fold_lanes.
#pragma once
#include "topo_core.h"

namespace morig_orient {

constexpr long long KEY_NONE = 0x7fffffffffffffffLL;
enum RootInfo : int { ROOT_ORIENTABLE = 1, ROOT_NONORIENTABLE = 2, ROOT_CLOSED = 4, ROOT_INVERTED = 8 };

// The record of the directed face edge a -> b (a != b, rows below 2^31): the key is the UNDIRECTED edge lo << 32 | hi, the direction
// travels in the value face << 1 | dir, dir = 1 where the face runs low -> high.
MORIG_TOPO_HD long long record_key(long long a, long long b) { return a < b ? ((a << 32) | b) : ((b << 32) | a); }
MORIG_TOPO_HD int record_val(int face, long long a, long long b) { return (face << 1) | (a < b ? 1 : 0); }

// The run of equal SORTED keys that holds position i (0 <= i < n): -> its length, capped at 3; *pos: the records of the run in front of
// i, capped at 2. At most four neighbours are read, whatever the length of the run and wherever it lies: a 200-face fan edge costs its
// records what a manifold edge costs.
MORIG_TOPO_HD int run_shape(const long long* keys, long long i, long long n, int* pos) {
    const long long k = keys[i];
    int before = 0, after = 0;
    if (i > 0 && keys[i - 1] == k) before = (i > 1 && keys[i - 2] == k) ? 2 : 1;
    if (i + 1 < n && keys[i + 1] == k) after = (i + 2 < n && keys[i + 2] == k) ? 2 : 1;
    *pos = before;
    const int count = 1 + before + after;
    return count > 3 ? 3 : count;
}

// The link of faces f < g with relative parity p (1: both traverse the edge the same way, an orientation conflict) as the cover edge of
// sign s: node 2f + s -- node 2g + (s ^ p), in morig_meshcheck_cc_round's layout lo << 32 | hi << 1 (2f + 1 < 2g: lo is f's node).
MORIG_TOPO_HD long long cover_key(long long f, long long g, int p, int s) { return ((2 * f + s) << 32) | ((2 * g + (s ^ p)) << 1); }

// The cover edge that sorted record i emits: KEY_NONE unless its run is a link (exactly two records, of faces f < g below n_faces); the
// first record of the link emits the edge of sign 0, the second that of sign 1. *count: the run's length as run_shape gives it.
MORIG_TOPO_HD long long link_cover(const long long* keys, const int* vals, long long i, long long n, long long n_faces, int* count) {
    int pos;
    *count = run_shape(keys, i, n, &pos);
    if (*count != 2) return KEY_NONE;
    const int val = vals[i], other = vals[pos == 0 ? i + 1 : i - 1];
    const int first = pos == 0 ? val : other, second = pos == 0 ? other : val;
    const long long f = first >> 1, g = second >> 1;
    if (first < 0 || second < 0 || f >= g || g >= n_faces) return KEY_NONE;
    return cover_key(f, g, (first & 1) == (second & 1) ? 1 : 0, pos);
}

// Six times the signed volume of the tetrahedron (0, A, B, C). Exchanging B and C negates every difference exactly (x - y = -(y - x) in
// IEEE arithmetic; a difference of equal numbers stays +0), so t(A, C, B) == -t(A, B, C) as numbers, NaNs apart: the sum of a repaired
// component is the sum that decided it.
MORIG_TOPO_HD double signed_term(const double* a, const double* b, const double* c) {
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// Which parity class of a component flips: -1 none (not orientable). A closed component with a volume sum s > 0 flips parity 1, with
// s < 0 parity 0 (*by_volume = true); an open one, or s == 0 or NaN, flips the class with fewer faces, parity 1 on a tie.
MORIG_TOPO_HD int flip_class(bool nonorientable, bool open, double s, long long n_faces, long long n_par1, bool* by_volume) {
    *by_volume = false;
    if (nonorientable) return -1;
    if (!open && s > 0.0) { *by_volume = true; return 1; }
    if (!open && s < 0.0) { *by_volume = true; return 0; }
    return n_par1 <= n_faces - n_par1 ? 1 : 0;
}

// the report bits of a component from the same inputs
MORIG_TOPO_HD int root_info(bool nonorientable, bool open, double s, long long n_faces, long long n_par1) {
    bool by_volume;
    const int cls = flip_class(nonorientable, open, s, n_faces, n_par1, &by_volume);
    if (cls < 0) return ROOT_NONORIENTABLE;
    int info = ROOT_ORIENTABLE | (open ? 0 : ROOT_CLOSED);
    if (by_volume && (cls == 1 ? n_par1 : n_faces - n_par1) == n_faces) info |= ROOT_INVERTED;
    return info;
}

}  // namespace morig_orient
