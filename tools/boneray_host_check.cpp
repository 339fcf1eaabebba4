// The per-joint statistics of csrc/labels.hip (morig_amd/csrc/boneray_core.h) as a plain host program, so that they can be checked without
// a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/boneray_host_check.cpp -o boneray_host_check
//     boneray_host_check IN OUT
// IN  (binary, native endianness): int32 n_joints, int64 n_values, float64 keep_factor, float64 fill; then int32 [n_joints] the number of
//     values of every joint (each at most 1 024); then float64 [n_values] the hit distances, joint after joint (+inf = a miss).
// OUT: float64 [n_joints][4] = (n_hit, n_kept, p20, featuresize); then uint8 [n_values] the kept flags.
// Besides select_serial the program checks that rank_of numbers the hits of every joint 0 .. n_hit - 1 without a gap (exit status 3).
// tests/test_labels_host.py builds and runs it against tests/labels_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/boneray_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0;
    int64_t n_values = 0;
    double keep_factor = 0.0, fill = 0.0;
    if (fread(&n, 4, 1, in) != 1 || fread(&n_values, 8, 1, in) != 1 || fread(&keep_factor, 8, 1, in) != 1 || fread(&fill, 8, 1, in) != 1 || n < 0 ||
        n > (1 << 24) || n_values < 0 || n_values > (1 << 26)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int32_t> counts((size_t)n);
    std::vector<double> t((size_t)n_values), stats((size_t)n * 4);
    std::vector<uint8_t> flags((size_t)n_values);
    if (fread(counts.data(), 4, counts.size(), in) != counts.size() || fread(t.data(), 8, t.size(), in) != t.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    int64_t at = 0;
    for (int32_t j = 0; j < n; ++j) {
        const int32_t m = counts[(size_t)j];
        if (m < 0 || m > morig_boneray::MAX_RAYS || at + m > n_values) { fprintf(stderr, "joint %d runs past the input or the limit\n", j); return 2; }
        const double* tj = t.data() + at;
        const morig_boneray::Stats st = morig_boneray::select_serial(tj, m, keep_factor, fill, flags.data() + at);
        std::vector<uint8_t> seen((size_t)st.n_hit, 0);
        for (int32_t i = 0; i < m; ++i) {
            if (!morig_boneray::hit(tj[i])) continue;
            const int r = morig_boneray::rank_of(tj, m, i);
            if (r < 0 || r >= st.n_hit || seen[(size_t)r]) { fprintf(stderr, "joint %d: rank %d of value %d is no permutation\n", j, r, i); return 3; }
            seen[(size_t)r] = 1;
        }
        stats[(size_t)j * 4] = (double)st.n_hit;
        stats[(size_t)j * 4 + 1] = (double)st.n_kept;
        stats[(size_t)j * 4 + 2] = st.p20;
        stats[(size_t)j * 4 + 3] = st.featuresize;
        at += m;
    }
    if (n > 0) fwrite(stats.data(), 8, stats.size(), out);
    if (n_values > 0) fwrite(flags.data(), 1, flags.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
