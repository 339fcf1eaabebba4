// Stand-alone check of csrc/bvh_core.h together with the per-face rules it guards (csrc/raytri_core.h, csrc/pointtri_core.h), for the CPU
// suite (tests/test_spatial_host.py builds it with -ffp-contract=off and the address and undefined-behaviour sanitizers). On seeded
// meshes, on a coarse binary grid and generic:
//   1. whenever the ray rule accepts a ray on a face at t, the face's box and every box of the tree above it is ENTERED for every best >= t;
//   2. whenever the point rule gives a face a squared distance below +inf, its boxes are not skipped for any best >= that distance;
//   3. the serial form of the three traversals of csrc/bvh.hip (near-first, re-checked when taken up, lexicographic best; the segment
//      query ends with its first hit) returns what the serial brute force returns: value, face, and for points the barycentrics, bit
//      for bit; blocked or not for segments, with and without a vertex to leave out and a t_max exactly at a hit.
// Prints one line per mesh and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../morig_amd/csrc/bvh_core.h"
#include "../morig_amd/csrc/pointtri_core.h"
#include "../morig_amd/csrc/raytri_core.h"

namespace bvh = morig_bvh;

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Mesh {
    std::vector<double> tri;                       // [F][9]
    std::vector<int> order;                        // sorted position -> face
    std::vector<std::vector<double>> levels;       // levels[k][n][6]
    int faces() const { return (int)(tri.size() / 9); }
};

void build(Mesh& m) {
    const int F = m.faces();
    double bbox[6];
    bvh::empty_box(bbox);
    for (int f = 0; f < F; ++f)
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) {
                const double x = m.tri[(size_t)f * 9 + c * 3 + k];
                if (x < bbox[k]) bbox[k] = x;
                if (x > bbox[3 + k]) bbox[3 + k] = x;
            }
    std::vector<long long> key(F);
    for (int f = 0; f < F; ++f) key[f] = bvh::face_key(0, bvh::morton30(&m.tri[(size_t)f * 9], &m.tri[(size_t)f * 9 + 3], &m.tri[(size_t)f * 9 + 6], bbox));
    m.order.resize(F);
    for (int f = 0; f < F; ++f) m.order[f] = f;
    std::stable_sort(m.order.begin(), m.order.end(), [&](int a, int b) { return key[a] < key[b]; });
    long long count[bvh::MAX_LEVELS];
    const int L = bvh::level_counts(F, count);
    m.levels.assign(L > 0 ? L : 0, {});
    for (int k = 0; k < L; ++k) {
        m.levels[k].resize((size_t)count[k] * 6);
        const long long below = k == 0 ? F : count[k - 1];
        for (long long n = 0; n < count[k]; ++n) {
            double* box = &m.levels[k][(size_t)n * 6];
            bvh::empty_box(box);
            for (long long c = n * bvh::WIDTH; c < std::min(below, (n + 1) * bvh::WIDTH); ++c) {
                double child[6];
                if (k == 0) {
                    const double* t = &m.tri[(size_t)m.order[c] * 9];
                    bvh::face_box(t, t + 3, t + 6, child);
                } else {
                    memcpy(child, &m.levels[k - 1][(size_t)c * 6], sizeof child);
                }
                bvh::grow_box(box, child);
            }
        }
    }
}

struct RayQ {
    double o[3], d[3], scale, best; int face;
    bool skips(const double* box, double& bound) const { return bvh::ray_skips(o, d, box, scale, best, bound); }
    bool wanted(double bound) const { return bvh::ray_wanted(bound, best); }
    bool done() const { return false; }
    bool value(const double* t, double& v) const {
        const morig_raytri::Num n = morig_raytri::numerators(o, d, t, t + 3, t + 6);
        return morig_raytri::hit(n, 0.0, v) && v < bvh::inf();
    }
};

// a face "names" the vertex `skip` when one of its corners has exactly that position's index: here every face owns three vertices, 3 f + k
struct SegQ {
    double o[3], d[3], scale, best, t_max; int face, skip; const double* tri;
    bool skips(const double* box, double& bound) const { return bvh::ray_skips(o, d, box, scale, t_max, bound); }
    bool wanted(double bound) const { return bvh::ray_wanted(bound, t_max); }
    bool done() const { return face != 0x7fffffff; }
    bool value(const double* t, double& v) const {
        if (skip >= 0 && (t - tri) / 9 == skip / 3) return false;
        const morig_raytri::Num n = morig_raytri::numerators(o, d, t, t + 3, t + 6);
        return morig_raytri::hit(n, 0.0, v) && v < t_max;
    }
};

struct PointQ {
    double p[3], slack, best; int face;
    bool skips(const double* box, double& bound) const { return bvh::point_skips(p, box, slack, best, bound); }
    bool wanted(double bound) const { return bvh::point_wanted(bound, slack, best); }
    bool done() const { return false; }
    bool value(const double* t, double& v) const {
        double bary[3];
        morig_pointtri::closest_bary(p, t, t + 3, t + 6, bary);
        v = morig_pointtri::bary_dist2(p, t, t + 3, t + 6, bary);
        return v < bvh::inf();
    }
};

// node `node` of level `level` (1-based) has been entered
template <class Q> void enter(const Mesh& m, Q& q, int level, long long node, long long& visits) {
    const long long first = node * bvh::WIDTH;
    if (level == 1) {
        const long long last = std::min<long long>(m.faces(), first + bvh::WIDTH);
        for (long long c = first; c < last; ++c) {
            double v;
            ++visits;
            const int f = m.order[c];
            if (!q.value(&m.tri[(size_t)f * 9], v)) continue;
            if (v < q.best || (v == q.best && f < q.face)) { q.best = v; q.face = f; }
        }
        return;
    }
    const std::vector<double>& boxes = m.levels[level - 2];
    const long long last = std::min<long long>((long long)(boxes.size() / 6), first + bvh::WIDTH);
    std::vector<std::pair<double, long long>> pending;
    for (long long c = first; c < last; ++c) {
        double bound;
        ++visits;
        if (!q.skips(&boxes[(size_t)c * 6], bound)) pending.push_back({bound, c});
    }
    std::sort(pending.begin(), pending.end());
    for (const auto& pc : pending) {
        if (q.done() || !q.wanted(pc.first)) break;
        enter(m, q, level - 1, pc.second, visits);
    }
}

template <class Q> long long walk(const Mesh& m, Q& q) {
    long long visits = 0;
    const int L = (int)m.levels.size();
    if (L == 0) return 0;
    double bound;
    ++visits;
    if (!q.skips(&m.levels[L - 1][0], bound)) enter(m, q, L, 0, visits);
    return visits;
}

int failures = 0;
void fail(const char* what, int mesh, int query) {
    if (++failures <= 20) fprintf(stdout, "FAILED %s: mesh %d query %d\n", what, mesh, query);
}

// every box above sorted position `at`, the face's own box first; returns false when `skips` refuses one
template <class Q> bool chain_entered(const Mesh& m, const Q& q, int f) {
    double box[6], bound;
    const double* t = &m.tri[(size_t)f * 9];
    bvh::face_box(t, t + 3, t + 6, box);
    if (q.skips(box, bound)) return false;
    long long at = std::find(m.order.begin(), m.order.end(), f) - m.order.begin();
    for (size_t k = 0; k < m.levels.size(); ++k) {
        at /= bvh::WIDTH;
        if (q.skips(&m.levels[k][(size_t)at * 6], bound)) return false;
    }
    return true;
}

double coordinate(Rng& rng, bool grid, double span) { return grid ? (double)rng.below(33) / 8.0 : span * (rng.unit() - 0.5); }

void check_mesh(int id, int F, int Q, bool grid, uint64_t seed) {
    Rng rng{seed};
    Mesh m;
    m.tri.resize((size_t)F * 9);
    for (int f = 0; f < F; ++f) {
        double c[3];
        for (int k = 0; k < 3; ++k) c[k] = coordinate(rng, grid, 4.0);
        for (int j = 0; j < 9; ++j) m.tri[(size_t)f * 9 + j] = grid ? coordinate(rng, true, 0.0) : c[j % 3] + 0.3 * (rng.unit() - 0.5);
        if (grid && f % 7 == 3) memcpy(&m.tri[(size_t)f * 9], &m.tri[(size_t)(f - 1) * 9], 9 * sizeof(double));      // a twin: an exact tie
        if (f % 41 == 17) memcpy(&m.tri[(size_t)f * 9 + 3], &m.tri[(size_t)f * 9], 3 * sizeof(double));              // zero area
        if (f % 97 == 29) m.tri[(size_t)f * 9 + 4] = NAN;
    }
    build(m);
    const double* root = m.levels.empty() ? nullptr : &m.levels.back()[0];
    long long ray_visits = 0, point_visits = 0, accepted = 0;
    for (int r = 0; r < Q; ++r) {
        RayQ q;
        for (int k = 0; k < 3; ++k) { q.o[k] = coordinate(rng, grid, 6.0); q.d[k] = grid ? (double)(rng.below(5) - 2) / 2.0 : rng.unit() - 0.5; }
        if (!grid && F > 0 && r % 3 != 0) {                                             // aimed at a point of a face
            const double* t = &m.tri[(size_t)rng.below(F) * 9];
            const double u = 0.5 * rng.unit(), v = 0.5 * rng.unit();
            for (int k = 0; k < 3; ++k) q.d[k] = (t[k] + u * (t[3 + k] - t[k]) + v * (t[6 + k] - t[k])) - q.o[k];
        }
        if (r % 11 == 5) q.d[rng.below(3)] = 0.0;
        if (r % 53 == 7) q.o[rng.below(3)] = NAN;
        q.scale = root ? bvh::query_scale(q.o, root) : 0.0;
        int bf = -1;
        double bt = bvh::inf();
        for (int f = 0; f < F; ++f) {                                                   // the serial brute force, and property 1 on the way
            double t;
            q.best = bvh::inf();
            if (!q.value(&m.tri[(size_t)f * 9], t)) continue;
            ++accepted;
            const double bests[3] = {t, t * 1.5, bvh::inf()};
            for (double best : bests) {
                q.best = best;
                if (!chain_entered(m, q, f)) fail("a box above an accepted hit is skipped", id, r);
            }
            if (t < bt) { bt = t; bf = f; }
        }
        q.best = bvh::inf(); q.face = 0x7fffffff;
        ray_visits += walk(m, q);
        const int got = q.face == 0x7fffffff ? -1 : q.face;
        if (got != bf || (bf >= 0 && memcmp(&q.best, &bt, sizeof bt) != 0)) fail("the ray walk differs from brute force", id, r);
        for (int variant = 0; variant < 3; ++variant) {                                 // the segment from o to o + d, o + d / 2 ...
            SegQ s;
            memcpy(s.o, q.o, sizeof s.o); memcpy(s.d, q.d, sizeof s.d);
            s.scale = q.scale; s.tri = m.tri.data();
            s.skip = variant >= 1 && bf >= 0 ? 3 * bf + 1 : -1;                         // leave out the nearest face
            s.t_max = variant == 2 && bf >= 0 ? bt : 1.0;                               // the nearest hit exactly at t_max
            bool want = false;
            for (int f = 0; f < F && !want; ++f) { double t; want = s.value(&m.tri[(size_t)f * 9], t); }
            s.best = s.t_max; s.face = 0x7fffffff;
            walk(m, s);
            if (s.done() != want) fail("the segment walk differs from brute force", id, r);
        }
    }
    for (int i = 0; i < Q; ++i) {
        PointQ q;
        for (int k = 0; k < 3; ++k) q.p[k] = coordinate(rng, grid, i % 5 == 0 ? 40.0 : 5.0);
        if (F > 0 && i % 3 == 1) memcpy(q.p, &m.tri[(size_t)rng.below(F) * 9 + 3 * rng.below(3)], sizeof q.p);      // on the surface
        if (i % 59 == 9) q.p[rng.below(3)] = NAN;
        q.slack = root ? bvh::point_slack(bvh::query_scale(q.p, root)) : 0.0;
        for (int f = 0; f < F; ++f) {                                                   // property 2
            double d2;
            q.best = bvh::inf();
            if (!q.value(&m.tri[(size_t)f * 9], d2)) continue;
            const double bests[3] = {d2, d2 * 2.0 + 1.0, bvh::inf()};
            for (double best : bests) {
                q.best = best;
                if (!chain_entered(m, q, f)) fail("a box above a face at this distance is skipped", id, i);
            }
        }
        double bary[3] = {0, 0, 0}, d2 = 0.0;
        int region = -1;
        const int bf = morig_pointtri::closest_face_serial(q.p, m.tri.data(), F, bary, &d2, &region);
        q.best = bvh::inf(); q.face = 0x7fffffff;
        point_visits += walk(m, q);
        const int got = q.face == 0x7fffffff ? -1 : q.face;
        bool same = got == bf;
        if (same && bf >= 0) {
            double mine[3];
            const double* t = &m.tri[(size_t)bf * 9];
            morig_pointtri::closest_bary(q.p, t, t + 3, t + 6, mine);
            same = memcmp(&q.best, &d2, sizeof d2) == 0 && memcmp(mine, bary, sizeof mine) == 0;
        }
        if (!same) fail("the point walk differs from brute force", id, i);
    }
    printf("mesh %d: %d faces (%s), %d queries, %lld accepted hits, tests per query: rays %.1f points %.1f\n", id, F, grid ? "grid" : "generic", Q,
           accepted, Q ? (double)ray_visits / Q : 0.0, Q ? (double)point_visits / Q : 0.0);
}

}  // namespace

int main() {
    long long count[bvh::MAX_LEVELS];
    const long long sizes[] = {0, 1, 64, 65, 4096, 4097, 262144, 262145, bvh::MAX_FACES, bvh::MAX_FACES + 1};
    const int levels[] = {0, 1, 1, 2, 2, 3, 3, 4, 4, -1};
    for (int i = 0; i < 10; ++i)
        if (bvh::level_counts(sizes[i], count) != levels[i]) fail("level_counts", i, 0);
    const int faces[] = {0, 1, 63, 64, 65, 300, 4097};
    int id = 0;
    for (int F : faces)
        for (int grid = 0; grid < 2; ++grid, ++id) check_mesh(id, F, F > 1000 ? 60 : 120, grid != 0, 0x5eed0000ull + (uint64_t)id);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
