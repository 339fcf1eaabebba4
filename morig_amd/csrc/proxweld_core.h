// The arithmetic of csrc/proxweld.hip that can go wrong on its own, shared with the host program
// tools/proxweld_host_check.cpp so that it can be checked without a device and under the host sanitizers: the inverse of the weld's
// coordinate key, the side of a grid cell, the cell of a coordinate, the packed cell key and the link test. Plain C++ without a HIP
// construct; float64 in the written order, contraction off (topo_core.h switches it off for clang, a host compiler takes
// -ffp-contract=off).
//
// The grid is an accelerator only: the links are DEFINED by the test `linked` over all pairs of nodes, and the walk over the 3 x 3 x 3
// neighbourhood must find exactly those. A link needs eps2 = fl(eps eps) to be a NORMAL double (EPS2_MIN = 2^-1022; below it nothing
// links): a subnormal eps2, and the squares next to it, are rounded to multiples of 2^-1074, which lets a link reach eps (1 + 2e-4) and
// more, past any fixed padding of the cell. With eps2 normal every square and sum near it is rounded to 2^-53 relative (a term in the
// subnormal range carries an absolute error of 2^-1075 <= 2^-53 eps2), so a link means y - x <= eps (1 + 2^-50) for two coordinates
// x <= y of one axis. With h >= eps (1 + 2^-20) and h >= extent / 2^20 the quotient q = fl(fl(x - lo) / h) is below
// 2^20 (1 + 2^-51) and carries an absolute error below 2^20 * 2^-51 = 2^-31 (eps >= 2^-511, so h and the quotient are normal), so
// q(y) - q(x) <= (1 + 2^-50) / (1 + 2^-20) + 2^-30 < 1 - 2^-21: the floors differ by at most one. Floor and clamp are monotone, so
// they keep the property.
#pragma once
#include "split_core.h"

namespace morig_prox {

constexpr int CELL_BITS = 21;
constexpr long long CELL_MASK = (1LL << CELL_BITS) - 1;
constexpr long long CELL_TOP = (1LL << CELL_BITS) - 2;         // the highest cell of an axis: three of them are not the sentinel key
constexpr long long KEY_NONE = 0x7fffffffffffffffLL;          // a row that is no node: it sorts behind every cell
constexpr double EPS2_MIN = 0x1p-1022;                         // the smallest normal double: a squared tolerance below it links nothing

// The coordinate of a morig_topo::coord_key (its inverse but for the sign of zero).
MORIG_TOPO_HD double key_coord(long long k) {
    const long long b = k >= 0 ? k : (k ^ 0x7fffffffffffffffLL);
    double x;
    memcpy(&x, &b, 8);
    return x;
}

// max(eps (1 + 2^-20), extent / 2^20), 1 where that is 0 (or a NaN). An infinite side (extent overflowed) is allowed: every
// coordinate then lands in cell 0.
MORIG_TOPO_HD double cell_side(double eps, double extent) {
    const double a = eps * (1.0 + 0x1p-20), b = extent * 0x1p-20;
    const double h = a > b ? a : b;
    return h > 0.0 ? h : 1.0;
}

// floor((x - lo) / h), clamped to [0, CELL_TOP]; a NaN quotient (inf / inf) goes to 0.
MORIG_TOPO_HD long long cell_coord(double x, double lo, double h) {
    const double q = (x - lo) / h;
    if (!(q >= 1.0)) return 0;
    if (q >= (double)CELL_TOP) return CELL_TOP;
    return (long long)q;                                       // q >= 1: truncation is the floor
}

MORIG_TOPO_HD long long cell_key(long long cx, long long cy, long long cz) { return (cx << (2 * CELL_BITS)) | (cy << CELL_BITS) | cz; }
MORIG_TOPO_HD long long key_x(long long key) { return key >> (2 * CELL_BITS); }
MORIG_TOPO_HD long long key_y(long long key) { return (key >> CELL_BITS) & CELL_MASK; }
MORIG_TOPO_HD long long key_z(long long key) { return key & CELL_MASK; }

// Two nodes are linked when (d0 d0 + d1 d1) + d2 d2 <= eps2, not strict, and eps2 is a normal double. eps2 < EPS2_MIN -- a tolerance of
// 0, or one below 2^-511 (1.5e-154), whose square is 0 or subnormal -- links nothing: the nodes are distinct points, a squared distance
// that underflows to 0 is not a distance of 0, and in the subnormal range the comparison has no precision left.
MORIG_TOPO_HD bool linked(const double* p, const double* q, double eps2) { return eps2 >= EPS2_MIN && morig_split::len2(p, q) <= eps2; }

// The first position in [lo, hi) of the ascending keys with keys[position] >= key (hi where there is none).
MORIG_TOPO_HD long long lower_bound(const long long* keys, long long lo, long long hi, long long key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The walk of node i (a sorted position of a mesh whose positions are [lo, hi)): the nine key ranges of its 3 x 3 x 3 neighbourhood in
// the order x, then y, every range in ascending position; `take(row)` is called for every partner with a higher input row inside the
// tolerance. Every position read lies in [lo, hi); a row outside [0, n_rows) is skipped.
template <class F>
MORIG_TOPO_HD void walk_links(const long long* keys, const long long* order, const double* pos, long long n_rows, long long i, long long lo,
                              long long hi, double eps2, F&& take) {
    const long long key = keys[i], row = order[i];
    if (key == KEY_NONE || key < 0 || row < 0 || row >= n_rows || !(eps2 >= EPS2_MIN)) return;
    const long long cx = key_x(key), cy = key_y(key), cz = key_z(key);
    const double p[3] = {pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
    const long long z0 = cz > 0 ? cz - 1 : 0, z1 = cz < CELL_TOP ? cz + 1 : CELL_TOP;
    for (long long nx = cx - 1; nx <= cx + 1; ++nx) {
        if (nx < 0 || nx > CELL_TOP) continue;
        for (long long ny = cy - 1; ny <= cy + 1; ++ny) {
            if (ny < 0 || ny > CELL_TOP) continue;
            const long long last = cell_key(nx, ny, z1);
            for (long long j = lower_bound(keys, lo, hi, cell_key(nx, ny, z0)); j < hi && keys[j] <= last; ++j) {
                const long long other = order[j];
                if (other > row && other < n_rows && linked(p, pos + j * 3, eps2)) take(other);
            }
        }
    }
}

}  // namespace morig_prox
