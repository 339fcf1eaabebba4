// Stand-alone check of the two visibility rules on the mesh BVH without a device: csrc/bonevis_core.h, the padded
// entering rule of csrc/bvh_core.h and the scan rule of csrc/scan.hip on csrc/raytri_core.h. tests/test_visibility_oracle.py builds it
// with -ffp-contract=off and the address and undefined-behaviour sanitizers and runs it as a program. On seeded meshes, generic and on a
// coarse binary grid:
//   1. ray_skips with the pad SLACK is the existing six-argument ray_skips, bit for bit; a larger pad never skips more;
//   2. whenever the bone rule accepts a face at t, the face's box and every box above it is ENTERED under the pad BONE_SLACK for every
//      best >= t; whenever the scan rule accepts a face (0 < t < 1), its boxes are entered under the pad SLACK with the bound 1;
//   3. the serial form of the two walks (the nearest hit on t ended by a hit that decides; any hit with the bound 1) gives the visibility
//      the serial brute force gives, where the brute force takes the minimum over h as bone_visibility_kernel does;
//   4. h(t) does not decrease with t on the accepted hits, and a hit that decides is followed by an invisible ray.
// Prints one line per mesh and returns 0, or says what failed and returns 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../morig_amd/csrc/bonevis_core.h"
#include "../morig_amd/csrc/bvh_core.h"
#include "../morig_amd/csrc/raytri_core.h"

namespace bvh = morig_bvh;
namespace bone = morig_bonevis;

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
    const double* face(int f) const { return &tri[(size_t)f * 9]; }
};

// the order from the triangles `pose` (another pose of the same faces), the boxes from the mesh's own: a view tree
void build(Mesh& m, const std::vector<double>& pose) {
    const int F = m.faces();
    double bbox[6];
    bvh::empty_box(bbox);
    for (size_t i = 0; i < pose.size(); ++i) {
        const int k = (int)(i % 3);
        if (pose[i] < bbox[k]) bbox[k] = pose[i];
        if (pose[i] > bbox[3 + k]) bbox[3 + k] = pose[i];
    }
    std::vector<long long> key(F);
    for (int f = 0; f < F; ++f) key[f] = bvh::face_key(0, bvh::morton30(&pose[(size_t)f * 9], &pose[(size_t)f * 9 + 3], &pose[(size_t)f * 9 + 6], bbox));
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
                if (k == 0) bvh::face_box(m.face(m.order[c]), m.face(m.order[c]) + 3, m.face(m.order[c]) + 6, child);
                else memcpy(child, &m.levels[k - 1][(size_t)c * 6], sizeof child);
                bvh::grow_box(box, child);
            }
        }
    }
}

int failures = 0;
void fail(const char* what, int a, int b) {
    if (++failures <= 20) printf("FAILED %s (%d, %d)\n", what, a, b);
}

// whether the box of the sorted position `at` and every box above it is entered
template <class Skips> bool entered(const Mesh& m, int at, const Skips& skips) {
    long long n = at;
    for (size_t k = 0; k < m.levels.size(); ++k) {
        n /= bvh::WIDTH;
        double bound;
        if (skips(&m.levels[k][(size_t)n * 6], bound)) return false;
    }
    return true;
}

struct BoneQ {
    bone::Ray ray; double scale, best; int face;
    bool skips(const double* box, double& bound) const { return bvh::ray_skips(ray.o, ray.d, box, scale, best, bound, bvh::BONE_SLACK); }
    bool wanted(double bound) const { return bvh::ray_wanted(bound, best); }
    bool done() const { return face >= 0 && bone::decides(bone::hit_distance(ray, best), ray.len); }
    bool value(const double* t, int, double& v) const { return bone::hit(ray, t, t + 3, t + 6, v) && v < bvh::inf(); }
};

struct ScanQ {
    double o[3], d[3], scale, best, len, eps; int face;
    bool skips(const double* box, double& bound) const { return bvh::ray_skips(o, d, box, scale, 1.0, bound); }
    bool wanted(double bound) const { return bvh::ray_wanted(bound, 1.0); }
    bool done() const { return face >= 0; }
    bool value(const double* t, int, double& v) const {
        const morig_raytri::Num n = morig_raytri::numerators(o, d, t, t + 3, t + 6);
        if (!morig_raytri::inside(n)) return false;
        v = n.tn / n.det;
        return v > 0.0 && v < 1.0 && v * len < len - eps;
    }
};

// the serial walk of csrc/bvh.hip: the pending children by (bound, child), re-checked when taken up
template <class Q> void enter(const Mesh& m, Q& q, int level, long long node) {
    const long long first = node * bvh::WIDTH;
    if (level == 0) {
        const long long last = std::min<long long>(m.faces(), first + bvh::WIDTH);
        for (long long c = first; c < last; ++c) {
            double v;
            const int f = m.order[c];
            if (q.value(m.face(f), f, v) && (v < q.best || (v == q.best && q.face >= 0 && f < q.face))) { q.best = v; q.face = f; }
        }
        return;
    }
    const std::vector<double>& boxes = m.levels[level - 1];
    const long long last = std::min<long long>((long long)(boxes.size() / 6), first + bvh::WIDTH);
    std::vector<std::pair<double, long long>> pending;
    for (long long c = first; c < last; ++c) {
        double bound;
        if (!q.skips(&boxes[(size_t)c * 6], bound)) pending.push_back({bound, c});
    }
    std::sort(pending.begin(), pending.end());
    for (const auto& p : pending) {
        if (q.done() || !q.wanted(p.first)) break;
        enter(m, q, level - 1, p.second);
    }
}

template <class Q> void walk(const Mesh& m, Q& q) {
    if (m.levels.empty()) return;
    enter(m, q, (int)m.levels.size(), 0);
}

void noisy_torus(Rng& r, int nu, int nv, double bend, std::vector<double>& tri) {
    auto at = [&](int i, int j, double* p) {
        const double u = 6.283185307179586 * (i % nu) / nu, v = 6.283185307179586 * (j % nv) / nv;
        Rng n{(uint64_t)((i % nu) * 4099 + (j % nv)) * 77 + 5};
        double x = (0.5 + 0.2 * cos(v)) * cos(u) + 1e-3 * n.unit(), y = 0.2 * sin(v) + 1e-3 * n.unit(), z = (0.5 + 0.2 * cos(v)) * sin(u) + 1e-3 * n.unit();
        const double a = bend * std::min(std::max(x / 0.3, 0.0), 1.0);
        p[0] = cos(a) * x - sin(a) * y; p[1] = sin(a) * x + cos(a) * y; p[2] = z;
    };
    (void)r;
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nv; ++j) {
            double q[4][3];
            at(i, j, q[0]); at(i + 1, j, q[1]); at(i + 1, j + 1, q[2]); at(i, j + 1, q[3]);
            const int ids[2][3] = {{0, 1, 2}, {0, 2, 3}};
            for (auto& t : ids)
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < 3; ++k) tri.push_back(q[t[c]][k]);
        }
}

void grid_soup(Rng& r, int n, std::vector<double>& tri) {                               // triangles on the grid of eighths, some degenerate
    for (int f = 0; f < n; ++f) {
        const double cx = r.below(17) * 0.125, cy = r.below(17) * 0.125, cz = r.below(17) * 0.125;
        for (int c = 0; c < 3; ++c) { tri.push_back(cx + r.below(5) * 0.125); tri.push_back(cy + r.below(5) * 0.125); tri.push_back(cz + r.below(5) * 0.125); }
    }
}

void check_bone(const Mesh& m, Rng& r, int n_rays, bool on_grid, int id) {
    const int F = m.faces();
    int hits = 0, invisible = 0;
    for (int q = 0; q < n_rays; ++q) {
        double p[3], bn[6];
        for (int k = 0; k < 3; ++k) {
            if (on_grid) { p[k] = r.below(33) * 0.125 - 1.0; bn[k] = r.below(33) * 0.125 - 1.0; bn[3 + k] = q % 5 ? r.below(33) * 0.125 - 1.0 : bn[k]; }
            else { p[k] = 1.6 * r.unit() - 0.8; bn[k] = 0.5 * r.unit() - 0.25; bn[3 + k] = q % 7 ? 0.5 * r.unit() - 0.25 : bn[k]; }
        }
        if (F && q % 3 == 0) {                                                          // end on a corner of the occluder, or on an edge
            const double* t = m.face(r.below(F));
            for (int k = 0; k < 3; ++k) p[k] = q % 2 ? t[k] : 0.5 * (t[k] + t[3 + k]);
        }
        if (q % 11 == 0) for (int k = 0; k < 3; ++k) p[k] = bn[k];                       // a ray of length zero
        BoneQ bq;
        bq.ray = bone::ray_of(p, bn);
        bq.best = bvh::inf(); bq.face = -1; bq.scale = 0.0;
        if (!m.levels.empty()) bq.scale = bvh::query_scale(bq.ray.o, &m.levels.back()[0]);
        double min_hit = bvh::inf(), min_t = bvh::inf();
        bool decided = false;
        for (int at = 0; at < F; ++at) {
            double t;
            const double* T = m.face(m.order[at]);
            if (!bone::hit(bq.ray, T, T + 3, T + 6, t)) continue;
            ++hits;
            const double h = bone::hit_distance(bq.ray, t);
            if (h < min_hit) min_hit = h;
            if (t < min_t) min_t = t;
            decided = decided || bone::decides(h, bq.ray.len);
            const double bests[3] = {t, t * 1.5, bvh::inf()};
            for (double best : bests)
                if (!entered(m, at, [&](const double* box, double& bound) { return bvh::ray_skips(bq.ray.o, bq.ray.d, box, bq.scale, best, bound, bvh::BONE_SLACK); }))
                    fail("an accepted bone hit's box is skipped", id, q);
        }
        if (min_t < bvh::inf()) {
            const double h = bone::hit_distance(bq.ray, min_t);
            if (!(h == min_hit || (std::isinf(h) && std::isinf(min_hit)))) fail("h of the smallest t is not the smallest h", id, q);
        }
        const bool want = bone::visible(min_hit, bq.ray.len);
        if (decided && want) fail("a deciding hit on a visible ray", id, q);
        walk(m, bq);
        const double h = bq.face >= 0 ? bone::hit_distance(bq.ray, bq.best) : bvh::inf();
        if (bone::visible(h, bq.ray.len) != want) fail("bone walk differs from the brute force", id, q);
        invisible += !want;
    }
    printf("mesh %d: %d faces, %d bone rays, %d accepted hits, %d invisible\n", id, F, n_rays, hits, invisible);
}

void check_scan(const Mesh& m, Rng& r, int n_rays, bool on_grid, int id) {
    const int F = m.faces();
    int blocked = 0;
    for (int q = 0; q < n_rays; ++q) {
        ScanQ sq;
        double end[3];
        for (int k = 0; k < 3; ++k) {
            if (on_grid) { sq.o[k] = k == 2 ? 4.0 : r.below(33) * 0.125; end[k] = k == 2 ? r.below(9) * 0.25 : sq.o[k]; }
            else { sq.o[k] = k == 2 ? 3.0 : 1.6 * r.unit() - 0.8; end[k] = k == 2 ? 1.6 * r.unit() - 0.8 : sq.o[k] + 0.2 * r.unit(); }
        }
        if (F && q % 2) {                                                               // a vertex of the mesh, as in a scan
            const double* t = m.face(r.below(F));
            for (int k = 0; k < 3; ++k) end[k] = t[k];
            if (on_grid) { sq.o[0] = end[0]; sq.o[1] = end[1]; }
        }
        for (int k = 0; k < 3; ++k) sq.d[k] = end[k] - sq.o[k];
        sq.len = sqrt((sq.d[0] * sq.d[0] + sq.d[1] * sq.d[1]) + sq.d[2] * sq.d[2]);
        sq.eps = on_grid ? (q % 4 ? 0.25 : 0.0) : 1e-4;
        sq.best = 1.0; sq.face = -1; sq.scale = 0.0;
        if (!m.levels.empty()) sq.scale = bvh::query_scale(sq.o, &m.levels.back()[0]);
        bool want = false;
        for (int at = 0; at < F; ++at) {
            double t;
            if (!sq.value(m.face(m.order[at]), m.order[at], t)) continue;
            want = true;
            if (!entered(m, at, [&](const double* box, double& bound) { return sq.skips(box, bound); })) fail("an accepted scan hit's box is skipped", id, q);
        }
        walk(m, sq);
        if ((sq.face >= 0) != want) fail("scan walk differs from the brute force", id, q);
        blocked += want;
    }
    printf("mesh %d: %d faces, %d scan segments, %d blocked\n", id, F, n_rays, blocked);
}

void check_pad(Rng& r) {
    for (int i = 0; i < 20000; ++i) {
        double o[3], d[3], box[6];
        for (int k = 0; k < 3; ++k) {
            o[k] = 4.0 * r.unit() - 2.0; d[k] = i % 3 == k ? 0.0 : 2.0 * r.unit() - 1.0;
            box[k] = 2.0 * r.unit() - 1.0; box[3 + k] = box[k] + r.unit();
        }
        if (i % 97 == 0) bvh::empty_box(box);
        const double scale = 8.0 * r.unit(), best = i % 5 ? 3.0 * r.unit() : bvh::inf();
        double b0, b1, b2;
        const bool s0 = bvh::ray_skips(o, d, box, scale, best, b0), s1 = bvh::ray_skips(o, d, box, scale, best, b1, bvh::SLACK);
        const bool s2 = bvh::ray_skips(o, d, box, scale, best, b2, bvh::BONE_SLACK);
        if (s0 != s1 || memcmp(&b0, &b1, sizeof b0) != 0) fail("the pad SLACK is not the existing rule", i, 0);
        if (s2 && !s0) fail("a larger pad skips more", i, 0);
    }
}

}  // namespace

int main() {
    Rng r{0x5669734368656b31ull};
    check_pad(r);
    const int sizes[][2] = {{0, 0}, {1, 1}, {8, 4}, {8, 8}, {16, 8}, {64, 32}};
    int id = 0;
    for (auto& s : sizes) {
        Mesh m;
        std::vector<double> rest;
        if (s[0]) { noisy_torus(r, s[0], s[1], 1.2, m.tri); noisy_torus(r, s[0], s[1], 0.0, rest); }
        if (s[0] == 1) { m.tri.resize(9); rest.resize(9); }
        build(m, id % 2 ? rest : m.tri);                                                // every other mesh in the order of its rest pose
        check_bone(m, r, 600, false, id);
        check_scan(m, r, 600, false, id);
        ++id;
    }
    for (int n : {65, 300}) {
        Mesh m;
        grid_soup(r, n, m.tri);
        build(m, m.tri);
        check_bone(m, r, 600, true, id);
        check_scan(m, r, 600, true, id);
        ++id;
    }
    if (failures) { printf("visibility_host_check: %d failures\n", failures); return 1; }
    printf("visibility_host_check: ok\n");
    return 0;
}
