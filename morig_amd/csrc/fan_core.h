// The arithmetic of csrc/meshsplit.hip that can go wrong on its own, shared with the host program
// tools/manifold_host_check.cpp so that it can be checked without a device and under the host sanitizers: the corner of a face edge
// record at the low and at the high end of its edge, and the corner link that a sorted record emits. Plain C++ without a HIP construct,
// integers only. The record, its key and the shape of a run are orient_core.h's.
#pragma once
#include "orient_core.h"

namespace morig_fan {

using morig_orient::KEY_NONE;

// Record r = 3 f + c is the edge from corner c to corner c + 1 of face f; dir = 1 where the face runs low -> high. The NODE of a corner
// is 3 f + corner.
MORIG_TOPO_HD long long node_at_lo(long long r, int dir) { return dir ? r : (r - r % 3) + (r % 3 + 1) % 3; }
MORIG_TOPO_HD long long node_at_hi(long long r, int dir) { return dir ? (r - r % 3) + (r % 3 + 1) % 3 : r; }

// two corners a < b of one vertex as an edge key of morig_meshcheck_cc_round: lo << 32 | hi << 1
MORIG_TOPO_HD long long link_key(long long a, long long b) { return (a << 32) | (b << 1); }

// The corner link that sorted record i emits (order[i]: the record at sorted position i): KEY_NONE unless its run is exactly two
// records, of faces f < g below n_faces whose records are theirs; the first record of the run carries the link of the two corners at
// the LOW end of the edge, the second that of the corners at the HIGH end. The traversal directions only say which corner is which.
// *count: the run's length, capped at 3; *pos: the records of the run in front of i, capped at 2.
MORIG_TOPO_HD long long fan_link(const long long* keys, const int* vals, const long long* order, long long i, long long n, long long n_faces,
                                 int* count, int* pos) {
    *count = morig_orient::run_shape(keys, i, n, pos);
    if (*count != 2) return KEY_NONE;
    const long long i0 = *pos == 0 ? i : i - 1, i1 = i0 + 1;
    const int first = vals[i0], second = vals[i1];
    const long long f = first >> 1, g = second >> 1, rf = order[i0], rg = order[i1];
    if (first < 0 || second < 0 || f >= g || g >= n_faces || rf < 0 || rg < 0 || rf / 3 != f || rg / 3 != g) return KEY_NONE;
    if (*pos == 0) return link_key(node_at_lo(rf, first & 1), node_at_lo(rg, second & 1));
    return link_key(node_at_hi(rf, first & 1), node_at_hi(rg, second & 1));
}

}  // namespace morig_fan
