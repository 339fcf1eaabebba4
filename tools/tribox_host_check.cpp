// The triangle-against-voxel test of csrc/meshprep.hip (morig_amd/csrc/tribox_core.h) as a plain host program, so that it can be checked
// without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/tribox_host_check.cpp -o tribox_host_check
//     tribox_host_check IN OUT
// IN  (binary, native endianness): int32 n, then n triangles of 9 float64 each (three vertices in grid coordinates), then n voxels of
//     3 int32 each (i, j, k).
// OUT: n bytes, 1 where the triangle overlaps the closed cube [i, i + 1] x [j, j + 1] x [k, k + 1].
// tests/test_meshprep_oracle.py builds and runs it against the separating-axis test of tests/meshprep_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/tribox_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1 || n < 0 || n > (1 << 24)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<double> tri((size_t)n * 9);
    std::vector<int32_t> vox((size_t)n * 3);
    std::vector<uint8_t> hit(n);
    if (n > 0 && (fread(tri.data(), 8, tri.size(), in) != tri.size() || fread(vox.data(), 4, vox.size(), in) != vox.size())) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    for (int32_t q = 0; q < n; ++q) {
        morig_tribox::Tri t;
        const double* p = tri.data() + (size_t)q * 9;
        morig_tribox::prepare(p, p + 3, p + 6, t);
        hit[q] = morig_tribox::overlaps(t, vox[(size_t)q * 3], vox[(size_t)q * 3 + 1], vox[(size_t)q * 3 + 2]) ? 1 : 0;
    }
    if (n > 0) fwrite(hit.data(), 1, hit.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
