// The shared arithmetic of csrc/meshcheck.hip (morig_amd/csrc/topo_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/topo_host_check.cpp -o topo_host_check
//     topo_host_check IN OUT
// IN  (binary, native endianness): int64 n_x, then n_x float64 coordinates; int64 n_keys, then n_keys int64 SORTED edge keys; int64
//     n_tri, then per triangle 9 float64 (A, B, C); int64 n_sums, then per sum int64 n and n float64 terms.
// OUT: n_x int64 coordinate keys; n_x int32 finite; n_keys int32 the class of the run that begins there; n_keys int64 the length of that
//     run; n_tri float64 areas; n_tri int32 zero-normal flags; n_sums float64: lane l of 64 adds the terms l, l + 64, ..., then the fold.
// tests/test_topology_oracle.py builds and runs it against tests/topology_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/topo_core.h"

namespace {

bool read_count(FILE* in, int64_t* n) { return fread(n, 8, 1, in) == 1 && *n >= 0 && *n <= (1 << 24); }

template <class T> bool read_all(FILE* in, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, in) == n;
}

template <class T> void write_all(FILE* out, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t n_x = 0, n_keys = 0, n_tri = 0, n_sums = 0;
    std::vector<double> xs, tris;
    std::vector<long long> keys;
    if (!read_count(in, &n_x) || !read_all(in, xs, (size_t)n_x) || !read_count(in, &n_keys) || !read_all(in, keys, (size_t)n_keys) ||
        !read_count(in, &n_tri) || !read_all(in, tris, (size_t)n_tri * 9) || !read_count(in, &n_sums)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    std::vector<long long> ckeys((size_t)n_x), run_len((size_t)n_keys);
    std::vector<int32_t> fin((size_t)n_x), cls((size_t)n_keys), zero((size_t)n_tri);
    std::vector<double> area((size_t)n_tri), sums((size_t)n_sums);
    for (int64_t i = 0; i < n_x; ++i) { ckeys[i] = morig_topo::coord_key(xs[i]); fin[i] = morig_topo::finite(xs[i]) ? 1 : 0; }
    for (int64_t i = 0; i < n_keys; ++i) cls[i] = morig_topo::classify_run(keys.data(), i, n_keys, &run_len[i]);
    for (int64_t i = 0; i < n_tri; ++i) {
        bool z = false;
        area[i] = morig_topo::tri_area(tris.data() + (size_t)i * 9, tris.data() + (size_t)i * 9 + 3, tris.data() + (size_t)i * 9 + 6, &z);
        zero[i] = z ? 1 : 0;
    }
    for (int64_t q = 0; q < n_sums; ++q) {
        int64_t n = 0;
        std::vector<double> terms;
        if (!read_count(in, &n) || !read_all(in, terms, (size_t)n)) { fprintf(stderr, "short sum %lld\n", (long long)q); return 2; }
        double lanes[64];
        for (int l = 0; l < 64; ++l) lanes[l] = 0.0;
        for (int64_t i = 0; i < n; ++i) lanes[i % 64] = lanes[i % 64] + terms[i];
        sums[q] = morig_topo::fold_lanes(lanes);
    }
    write_all(out, ckeys);
    write_all(out, fin);
    write_all(out, cls);
    write_all(out, run_len);
    write_all(out, area);
    write_all(out, zero);
    write_all(out, sums);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
