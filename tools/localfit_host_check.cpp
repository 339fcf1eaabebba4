// The per-fit arithmetic of csrc/local_motion.hip (morig_amd/csrc/localfit_core.h) as a plain host program, so that it can be checked
// without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/localfit_host_check.cpp -o localfit_host_check
//     localfit_host_check IN OUT
// IN  (binary, native endianness): int32 n_verts, frames, n_ids, n_ladders, n_pairs; then int32 [n_verts + 1] the patch pointer; int32
//     [n_ids] the patch members; float64 [n_verts][3] the rest pose; float64 [n_verts][frames][3] the clip; int32 [n_ladders][3] candidate
//     counts under the three rungs; float64 [n_pairs][6] pairs of points.
// OUT: float64 [n_verts * frames][11] = (rot6d 6, trans 3, gap, residual); then int32 [n_ladders] the rung chosen; then float64 [n_pairs]
//     the distances.
// Besides, the program checks that the two columns of every rotation it writes are orthonormal to 1e-12 (exit status 3).
// tests/test_local_motion_host.py builds and runs it against tests/local_motion_oracle.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/localfit_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t h[5] = {0, 0, 0, 0, 0};
    if (fread(h, 4, 5, in) != 5) { fprintf(stderr, "bad header\n"); return 2; }
    const int32_t nv = h[0], frames = h[1], n_ids = h[2], n_ladders = h[3], n_pairs = h[4];
    for (int k = 0; k < 5; ++k)
        if (h[k] < 0 || h[k] > (1 << 22)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> ptr((size_t)nv + 1), ids((size_t)n_ids), ladders((size_t)n_ladders * 3), rungs((size_t)n_ladders);
    std::vector<double> src((size_t)nv * 3), traj((size_t)nv * frames * 3), pairs((size_t)n_pairs * 6), dists((size_t)n_pairs);
    std::vector<double> res((size_t)nv * frames * 11);
    if (fread(ptr.data(), 4, ptr.size(), in) != ptr.size() || fread(ids.data(), 4, ids.size(), in) != ids.size() ||
        fread(src.data(), 8, src.size(), in) != src.size() || fread(traj.data(), 8, traj.size(), in) != traj.size() ||
        fread(ladders.data(), 4, ladders.size(), in) != ladders.size() || fread(pairs.data(), 8, pairs.size(), in) != pairs.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    if (ptr[0] != 0 || ptr[nv] != n_ids) { fprintf(stderr, "bad patch pointer\n"); return 2; }
    for (int32_t v = 0; v < nv; ++v)
        if (ptr[v + 1] < ptr[v]) { fprintf(stderr, "bad patch pointer\n"); return 2; }
    for (int32_t v = 0; v < nv; ++v)
        for (int32_t t = 0; t < frames; ++t) {
            double* o = res.data() + ((size_t)v * frames + t) * 11;
            int bad = 0;
            morig_localfit::fit<double>(ids.data() + ptr[v], ptr[v + 1] - ptr[v], nv, src.data(), traj.data() + (size_t)t * 3, (long long)frames * 3,
                                        o, o + 6, o + 9, o + 10, &bad);
            if (bad) { fprintf(stderr, "vertex %d: a member outside the mesh\n", v); return 3; }
            if (ptr[v + 1] == ptr[v]) continue;
            const double a[3] = {o[0], o[1], o[2]}, b[3] = {o[3], o[4], o[5]};
            const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
            const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
            if (std::fabs(aa - 1.0) > 1e-12 || std::fabs(bb - 1.0) > 1e-12 || std::fabs(ab) > 1e-12) {
                fprintf(stderr, "vertex %d, frame %d: columns not orthonormal\n", v, t);
                return 3;
            }
        }
    for (int32_t k = 0; k < n_ladders; ++k) rungs[k] = morig_localfit::choose_rung(ladders[(size_t)k * 3], ladders[(size_t)k * 3 + 1], ladders[(size_t)k * 3 + 2]);
    for (int32_t k = 0; k < n_pairs; ++k) dists[k] = morig_localfit::dist(pairs.data() + (size_t)k * 6, pairs.data() + (size_t)k * 6 + 3);
    if (!res.empty()) fwrite(res.data(), 8, res.size(), out);
    if (!rungs.empty()) fwrite(rungs.data(), 4, rungs.size(), out);
    if (!dists.empty()) fwrite(dists.data(), 8, dists.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
