// The per-cell arithmetic of csrc/simplify.hip (morig_amd/csrc/quadric_core.h) as a plain host program, so that it can be checked without
// a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/quadric_host_check.cpp -o quadric_host_check
//     quadric_host_check IN OUT
// IN  (binary, native endianness): int32 n, int64 members in all, int64 corners in all; then per cell 5 int32 (members, corners, cx, cy, cz);
//     then per cell 4 float64 (the grid's minimum x, y, z and the cell size h); then the members, 3 float64 each, cell after cell; then
//     the corners, 9 float64 each (A, B, C of the corner's face), cell after cell.
// OUT: n x 3 float64, the output vertex of every cell. Every sum runs in the stored order.
// tests/test_simplify_oracle.py builds and runs it against tests/simplify_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/quadric_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0;
    int64_t n_members = 0, n_corners = 0;
    if (fread(&n, 4, 1, in) != 1 || fread(&n_members, 8, 1, in) != 1 || fread(&n_corners, 8, 1, in) != 1 || n < 0 || n > (1 << 24) ||
        n_members < 0 || n_members > (1 << 26) || n_corners < 0 || n_corners > (1 << 26)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int32_t> table((size_t)n * 5);
    std::vector<double> grid((size_t)n * 4), members((size_t)n_members * 3), corners((size_t)n_corners * 9), pos((size_t)n * 3);
    if (fread(table.data(), 4, table.size(), in) != table.size() || fread(grid.data(), 8, grid.size(), in) != grid.size() ||
        fread(members.data(), 8, members.size(), in) != members.size() || fread(corners.data(), 8, corners.size(), in) != corners.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    int64_t m0 = 0, k0 = 0;
    for (int32_t q = 0; q < n; ++q) {
        const int32_t nm = table[(size_t)q * 5], nk = table[(size_t)q * 5 + 1];
        if (nm < 0 || nk < 0 || m0 + nm > n_members || k0 + nk > n_corners) { fprintf(stderr, "cell %d runs past the input\n", q); return 2; }
        double s[3] = {0.0, 0.0, 0.0}, cen[3];
        for (int64_t i = m0; i < m0 + nm; ++i)
            for (int k = 0; k < 3; ++k) s[k] = s[k] + members[(size_t)i * 3 + k];
        for (int k = 0; k < 3; ++k) cen[k] = s[k] / (double)nm;
        morig_quadric::Acc acc;
        morig_quadric::zero(acc);
        for (int64_t i = k0; i < k0 + nk; ++i) {
            const double* p = corners.data() + (size_t)i * 9;
            morig_quadric::corner(p, p + 3, p + 6, cen, acc);
        }
        morig_quadric::solve_clamp(acc, cen, grid.data() + (size_t)q * 4, grid[(size_t)q * 4 + 3], table.data() + (size_t)q * 5 + 2, pos.data() + (size_t)q * 3);
        m0 += nm;
        k0 += nk;
    }
    if (n > 0) fwrite(pos.data(), 8, pos.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
