// The ray-against-triangle test and the pixel ray of csrc/scan.hip (morig_amd/csrc/raytri_core.h) as a plain host program, so that they
// can be checked without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/raytri_host_check.cpp -o raytri_host_check
//     raytri_host_check IN OUT
// IN  (binary, native endianness): int32 n, then n decisions of 16 float64 each (origin 3, direction 3, A 3, B 3, C 3, near);
//     int32 m, then m cameras of 16 float64 each, then m rows of 5 int32 (kind, W, H, i, j).
// OUT: n rows of 6 float64 (hit as 0 / 1, det, un, vn, tn, t -- 0 without a hit), then m rows of 6 float64 (origin, direction).
// tests/test_scan_oracle.py builds and runs it against tests/scan_oracle.py, bit for bit.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/raytri_core.h"

static bool read_count(FILE* in, int32_t& n) { return fread(&n, 4, 1, in) == 1 && n >= 0 && n <= (1 << 24); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n = 0, m = 0;
    if (!read_count(in, n)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<double> dec((size_t)n * 16), res((size_t)n * 6);
    if (n > 0 && fread(dec.data(), 8, dec.size(), in) != dec.size()) { fprintf(stderr, "short input\n"); return 2; }
    if (!read_count(in, m)) { fprintf(stderr, "bad second header\n"); return 2; }
    std::vector<double> cams((size_t)m * 16), rays((size_t)m * 6);
    std::vector<int32_t> px((size_t)m * 5);
    if (m > 0 && (fread(cams.data(), 8, cams.size(), in) != cams.size() || fread(px.data(), 4, px.size(), in) != px.size())) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    for (int32_t q = 0; q < n; ++q) {
        const double* p = dec.data() + (size_t)q * 16;
        const morig_raytri::Num k = morig_raytri::numerators(p, p + 3, p + 6, p + 9, p + 12);
        double t = 0.0;
        const bool hit = morig_raytri::hit(k, p[15], t);
        double* r = res.data() + (size_t)q * 6;
        r[0] = hit ? 1.0 : 0.0; r[1] = k.det; r[2] = k.un; r[3] = k.vn; r[4] = k.tn; r[5] = hit ? t : 0.0;
    }
    for (int32_t q = 0; q < m; ++q) {
        const int32_t* a = px.data() + (size_t)q * 5;
        morig_raytri::pixel_ray(cams.data() + (size_t)q * 16, a[0], a[1], a[2], a[3], a[4], rays.data() + (size_t)q * 6, rays.data() + (size_t)q * 6 + 3);
    }
    if (n > 0) fwrite(res.data(), 8, res.size(), out);
    if (m > 0) fwrite(rays.data(), 8, rays.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
