// The closest-point rule of csrc/transfer.hip (morig_amd/csrc/pointtri_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/pointtri_host_check.cpp -o pointtri_host_check
//     pointtri_host_check IN OUT
// IN  (binary, native endianness): int32 n_points, int32 n_faces; then float64 [n_points][3] the points; then float64 [n_faces][9] the
//     triangles (a, b, c).
// OUT: int32 [n_points][2] = (face, region), -1 where no triangle has a distance below +inf; then float64 [n_points][4] = (b0, b1, b2,
//     squared distance), NaN there.
// Besides the winner the program checks for every pair that the barycentrics of a region have the zeros and ones the region states
// (exit status 3). tests/test_transfer_host.py builds and runs it against tests/transfer_oracle.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/pointtri_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0, nf = 0;
    if (fread(&n, 4, 1, in) != 1 || fread(&nf, 4, 1, in) != 1 || n < 0 || nf < 0 || n > (1 << 22) || nf > (1 << 22)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<double> pts((size_t)n * 3), tri((size_t)nf * 9), real((size_t)n * 4);
    std::vector<int32_t> ints((size_t)n * 2);
    if (fread(pts.data(), 8, pts.size(), in) != pts.size() || fread(tri.data(), 8, tri.size(), in) != tri.size()) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    using namespace morig_pointtri;
    static const int zero_at[7][3] = {{0, 1, 1}, {1, 0, 1}, {0, 0, 1}, {1, 1, 0}, {0, 1, 0}, {1, 0, 0}, {0, 0, 0}};
    for (int32_t i = 0; i < n; ++i) {
        const double* p = pts.data() + (size_t)i * 3;
        for (int32_t f = 0; f < nf; ++f) {
            const double* t = tri.data() + (size_t)f * 9;
            double b[3];
            const int r = closest_bary(p, t, t + 3, t + 6, b);
            if (r < 0 || r > FACE) { fprintf(stderr, "point %d, face %d: region %d\n", i, f, r); return 3; }
            for (int k = 0; k < 3; ++k)
                if (zero_at[r][k] && b[k] != 0.0) { fprintf(stderr, "point %d, face %d: region %d with b%d = %g\n", i, f, r, k, b[k]); return 3; }
            if ((r == VERTEX_A && b[0] != 1.0) || (r == VERTEX_B && b[1] != 1.0) || (r == VERTEX_C && b[2] != 1.0)) {
                fprintf(stderr, "point %d, face %d: vertex region %d without a weight of one\n", i, f, r);
                return 3;
            }
        }
        double bary[3] = {NAN, NAN, NAN}, d2 = NAN;
        int region = -1;
        ints[(size_t)i * 2] = closest_face_serial(p, tri.data(), nf, bary, &d2, &region);
        ints[(size_t)i * 2 + 1] = region;
        for (int k = 0; k < 3; ++k) real[(size_t)i * 4 + k] = bary[k];
        real[(size_t)i * 4 + 3] = d2;
    }
    if (n > 0) { fwrite(ints.data(), 4, ints.size(), out); fwrite(real.data(), 8, real.size(), out); }
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
