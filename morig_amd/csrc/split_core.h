// The arithmetic of csrc/refine.hip that can go wrong on its own, shared with the host program
// tools/refine_host_check.cpp so that it can be checked without a device and under the host sanitizers: the squared length of an edge and
// its order-preserving integer image, the midpoint, the mask of a face's marked edges, the rotation that puts a pattern into its
// canonical frame, the choice of the quad's diagonal and the table of children. Plain C++ without a HIP construct; float64 in the written
// order, contraction off (topo_core.h switches it off for clang, a host compiler takes -ffp-contract=off).
#pragma once
#include "topo_core.h"

namespace morig_split {

constexpr long long KEY_NONE = 0x7fffffffffffffffLL;

// The undirected edge {a, b}, a != b, rows below 2^31: lo << 32 | hi (the layout of orient_core.h record_key).
MORIG_TOPO_HD long long split_key(long long a, long long b) { return a < b ? ((a << 32) | b) : ((b << 32) | a); }

// (d0 d0 + d1 d1) + d2 d2 with d = p - q: exchanging p and q negates every d exactly, so the value does not depend on the direction.
MORIG_TOPO_HD double len2(const double* p, const double* q) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// The image of a squared length under which integer order is numeric order: the bit pattern of a finite value (never negative: a sum
// of squares; -0.0 cannot occur), -1 for an infinity or a NaN, which take part in no maximum and in no mark.
MORIG_TOPO_HD long long len2_image(double x) { return morig_topo::finite(x) ? morig_topo::bits_of(x) : -1; }

MORIG_TOPO_HD double image_len2(long long image) {
    double x;
    memcpy(&x, &image, 8);
    return x;
}

MORIG_TOPO_HD void midpoint(const double* a, const double* b, double* m) {
    for (int d = 0; d < 3; ++d) m[d] = 0.5 * (a[d] + b[d]);
}

// Edge c of the face (v0, v1, v2) runs from corner c to corner c + 1; mid[c] is its new vertex, negative where it is not marked.
MORIG_TOPO_HD int mask_of(const int* mid) { return (mid[0] >= 0 ? 1 : 0) | (mid[1] >= 0 ? 2 : 0) | (mid[2] >= 0 ? 4 : 0); }
MORIG_TOPO_HD int marked_edges(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }
MORIG_TOPO_HD int child_count(int mask) { return 1 + marked_edges(mask); }

// The corner the canonical frame (a, b, c) = (v[r], v[r + 1], v[r + 2]) begins with. One marked edge: it is a -> b. Two: a is their
// apex, so the unmarked edge is b -> c. None or three: the face as it is listed.
MORIG_TOPO_HD int rotation(int mask) {
    switch (mask) {
        case 1: return 0;
        case 2: return 1;
        case 4: return 2;
        case 3: return 1;      // edges 0 and 1 meet in corner 1
        case 6: return 2;
        case 5: return 0;
        default: return 0;
    }
}

// Two marked edges, frame (a, b, c) with the new vertices ab and ca: the quad (ab, b, c, ca) is cut along ab -- c (-> 0) or along
// b -- ca (-> 1), whichever is shorter; a tie goes to the diagonal with the lowest vertex index, and the two old vertices b and c lie
// below every new one.
MORIG_TOPO_HD int pick_diagonal(double l2_ab_c, double l2_b_ca, long long b, long long c) {
    if (l2_ab_c < l2_b_ca) return 0;
    if (l2_b_ca < l2_ab_c) return 1;
    return c < b ? 0 : 1;
}

// The diagonal of a face with two marked edges from the positions of its frame's corners: the new vertices as they are emitted
// (a + b is b + a, so the direction of an edge does not matter).
MORIG_TOPO_HD int frame_diagonal(const double* pa, const double* pb, const double* pc, long long b, long long c) {
    double ab[3], ca[3];
    midpoint(pa, pb, ab);
    midpoint(pc, pa, ca);
    return pick_diagonal(len2(ab, pc), len2(pb, ca), b, c);
}

// The children of the face v with the new vertices mid under ``mask`` (= mask_of(mid)) and, where two edges are marked, the diagonal
// ``diag`` -> their number; winding is kept. out[k] is child k.
MORIG_TOPO_HD int children(const long long* v, const long long* mid, int mask, int diag, long long out[4][3]) {
    const int r = rotation(mask);
    const long long a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3];
    const long long ab = mid[r], bc = mid[(r + 1) % 3], ca = mid[(r + 2) % 3];
    auto put = [&](int k, long long x, long long y, long long z) { out[k][0] = x; out[k][1] = y; out[k][2] = z; };
    switch (marked_edges(mask)) {
        case 0:
            put(0, a, b, c);
            return 1;
        case 1:                                    // the median ab -- c
            put(0, a, ab, c);
            put(1, ab, b, c);
            return 2;
        case 2:                                    // the corner at the apex, then the quad
            put(0, a, ab, ca);
            if (diag == 0) { put(1, ab, b, c); put(2, ab, c, ca); }
            else { put(1, ab, b, ca); put(2, b, c, ca); }
            return 3;
        default:                                   // the three corners in corner order, then the centre
            put(0, a, ab, ca);
            put(1, b, bc, ab);
            put(2, c, ca, bc);
            put(3, ab, bc, ca);
            return 4;
    }
}

}  // namespace morig_split
