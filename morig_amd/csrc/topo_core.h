// The arithmetic of csrc/meshcheck.hip that can go wrong on its own, shared with the host program
// tools/topo_host_check.cpp so that it can be checked without a device and under the host sanitizers: the coordinate key of the weld, the
// directed edge key and the classification of a run of them, the triangle area and the fold of 64 lane sums. Plain C++ without a HIP
// construct. All float64 in the written order: contraction is switched off here for clang, from this point to the end of the including
// file (with a fused multiply-add the normal of a zero-area face is its rounding error, not zero); a host compiler takes
// -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define MORIG_TOPO_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define MORIG_TOPO_HD inline
#endif

namespace morig_topo {

constexpr long long KEY_SENTINEL = 0x7fffffffffffffffLL;
enum EdgeClass : int { EDGE_NONE = 0, EDGE_MANIFOLD = 1, EDGE_BOUNDARY = 2, EDGE_NONMANIFOLD = 3, EDGE_CONFLICT = 4 };

MORIG_TOPO_HD long long bits_of(double x) {
    long long b;
    memcpy(&b, &x, 8);
    return b;
}

// finite: neither an infinity nor a NaN (the exponent field is not all ones)
MORIG_TOPO_HD bool finite(double x) { return ((bits_of(x) >> 52) & 0x7ff) != 0x7ff; }

// A signed 64-bit key with key(a) < key(b) exactly when a < b, and key(a) == key(b) exactly when a == b as numbers: -0.0 takes the key of
// +0.0 (0). A non-negative double keeps its bit pattern; a negative one has its 63 magnitude bits flipped, so that a larger magnitude is
// a smaller key. (A NaN gets some key too; the weld never compares the keys of a row with a non-finite coordinate.)
MORIG_TOPO_HD long long coord_key(double x) {
    if (x == 0.0) return 0;
    const long long b = bits_of(x);
    return b >= 0 ? b : (b ^ 0x7fffffffffffffffLL);
}

// The undirected edge {a, b}, a != b, rows below 2^31, as one key: lo << 32 | hi << 1 | dir, dir = 1 where the face traverses the edge
// low -> high (a < b for the directed pair a -> b of its cyclic order).
MORIG_TOPO_HD long long edge_key(long long a, long long b) {
    return a < b ? ((a << 32) | (b << 1) | 1LL) : ((b << 32) | (a << 1));
}
MORIG_TOPO_HD long long edge_lo(long long key) { return key >> 32; }
MORIG_TOPO_HD long long edge_hi(long long key) { return (key & 0xffffffffLL) >> 1; }

// The class of the run of SORTED keys that begins at i (0 <= i < n): EDGE_NONE where i does not begin a run (its predecessor is the same
// edge) or holds the sentinel; else by n_inc = the keys of the run and fwd = those with dir = 1: one key a boundary edge, three or more a
// non-manifold edge, two an orientation conflict unless exactly one runs low -> high. The walk is sequential, so a run may be of any
// length and lie anywhere in the array.
MORIG_TOPO_HD int classify_run(const long long* keys, long long i, long long n, long long* n_inc) {
    const long long k = keys[i];
    *n_inc = 0;
    if (k == KEY_SENTINEL || (i > 0 && (keys[i - 1] >> 1) == (k >> 1))) return EDGE_NONE;
    long long count = 0, fwd = 0;
    for (long long j = i; j < n && (keys[j] >> 1) == (k >> 1); ++j) {
        ++count;
        fwd += keys[j] & 1;
    }
    *n_inc = count;
    if (count == 1) return EDGE_BOUNDARY;
    if (count >= 3) return EDGE_NONMANIFOLD;
    return fwd == 1 ? EDGE_MANIFOLD : EDGE_CONFLICT;
}

// n = (B - A) x (C - A); the area 0.5 sqrt((nx^2 + ny^2) + nz^2); *zero: n is exactly (0, 0, 0)
MORIG_TOPO_HD double tri_area(const double* a, const double* b, const double* c, bool* zero) {
    double e1[3], e2[3];
    for (int d = 0; d < 3; ++d) { e1[d] = b[d] - a[d]; e2[d] = c[d] - a[d]; }
    const double nx = e1[1] * e2[2] - e1[2] * e2[1];
    const double ny = e1[2] * e2[0] - e1[0] * e2[2];
    const double nz = e1[0] * e2[1] - e1[1] * e2[0];
    *zero = nx == 0.0 && ny == 0.0 && nz == 0.0;
    return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// The sum of 64 lane sums: lane l takes lane l + h for h = 32, 16, 8, 4, 2, 1; the result is s[0]. s is overwritten.
MORIG_TOPO_HD double fold_lanes(double* s) {
    for (int h = 32; h > 0; h >>= 1)
        for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
    return s[0];
}

}  // namespace morig_topo
