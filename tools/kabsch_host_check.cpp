// The rigid-fit core of csrc/piecewise.hip (morig_amd/csrc/kabsch_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kabsch_host_check.cpp -o kabsch_host_check
//     kabsch_host_check IN OUT
// IN  (binary, native endianness): int32 n, then n cross-covariances of 9 float64 each, row-major (tar_c^T src_c).
// OUT: n rotations of 9 float64 each, row-major, then n int32 sweep counts.
// tests/test_piecewise_host.py builds and runs it against the rotations recorded from the reference's own fits.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/kabsch_core.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1 || n < 0 || n > (1 << 24)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<double> M((size_t)n * 9), R((size_t)n * 9);
    std::vector<int32_t> sweeps(n);
    if (n > 0 && fread(M.data(), 8, M.size(), in) != M.size()) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t i = 0; i < n; ++i) sweeps[i] = morig_kabsch::rotation(M.data() + (size_t)i * 9, R.data() + (size_t)i * 9);
    if (n > 0) {
        fwrite(R.data(), 8, R.size(), out);
        fwrite(sweeps.data(), 4, sweeps.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
