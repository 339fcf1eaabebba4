// The shared arithmetic of csrc/meshfix.hip (morig_amd/csrc/orient_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/meshfix_host_check.cpp -o meshfix_host_check
//     meshfix_host_check IN OUT
// IN  (binary, native endianness): int64 n_faces, then per face 3 int64 rows; int64 n_rec, then n_rec int64 SORTED record keys and n_rec
//     int32 record values; int64 n_tri, then per triangle 9 float64 (A, B, C); int64 n_dec, then per decision int64 nonorientable, int64
//     open, float64 S, int64 faces, int64 parity-1 faces; int64 n_sums, then per sum int64 n and n float64 terms.
// OUT: per record int32 the length of its run (capped at 3), int32 its place in it (capped at 2), int64 its cover edge; per face and
//     corner int64 the record key, then int32 the record value; per triangle float64 t(A, B, C), then t(A, C, B); per decision int32 the
//     class that flips, int32 whether the volume decided, int32 the report bits; per sum float64: lane l of 64 adds the terms l, l + 64,
//     ..., then the fold.
// tests/test_repair_oracle.py builds and runs it against tests/repair_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/orient_core.h"

namespace {

bool read_count(FILE* in, int64_t* n) { return fread(n, 8, 1, in) == 1 && *n >= 0 && *n <= (1 << 24); }

template <class T> bool read_all(FILE* in, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, in) == n;
}

template <class T> void write_all(FILE* out, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out);
}

struct Decision { int64_t nonorientable, open; double s; int64_t faces, par1; };

}  // namespace

int main(int argc, char** argv) {
    using namespace morig_orient;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t n_faces = 0, n_rec = 0, n_tri = 0, n_dec = 0, n_sums = 0;
    std::vector<long long> faces, keys;
    std::vector<int32_t> vals;
    std::vector<double> tris;
    std::vector<Decision> decs;
    static_assert(sizeof(Decision) == 40, "five 8-byte fields");
    if (!read_count(in, &n_faces) || !read_all(in, faces, (size_t)n_faces * 3) || !read_count(in, &n_rec) || !read_all(in, keys, (size_t)n_rec) ||
        !read_all(in, vals, (size_t)n_rec) || !read_count(in, &n_tri) || !read_all(in, tris, (size_t)n_tri * 9) || !read_count(in, &n_dec) ||
        !read_all(in, decs, (size_t)n_dec) || !read_count(in, &n_sums)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    std::vector<int32_t> count((size_t)n_rec), pos((size_t)n_rec), rval((size_t)n_faces * 3), cls((size_t)n_dec), byvol((size_t)n_dec), info((size_t)n_dec);
    std::vector<long long> cover((size_t)n_rec), rkey((size_t)n_faces * 3);
    std::vector<double> t((size_t)n_tri), tneg((size_t)n_tri), sums((size_t)n_sums);
    for (int64_t i = 0; i < n_rec; ++i) {
        int p = 0, c = 0;
        count[i] = run_shape(keys.data(), i, n_rec, &p);
        pos[i] = p;
        cover[i] = link_cover(keys.data(), vals.data(), i, n_rec, n_faces, &c);
        if (c != count[i]) { fprintf(stderr, "link_cover and run_shape disagree at %lld\n", (long long)i); return 2; }
    }
    for (int64_t f = 0; f < n_faces; ++f)
        for (int c = 0; c < 3; ++c) {
            const long long a = faces[(size_t)f * 3 + c], b = faces[(size_t)f * 3 + (c + 1) % 3];
            rkey[(size_t)f * 3 + c] = record_key(a, b);
            rval[(size_t)f * 3 + c] = record_val((int)f, a, b);
        }
    for (int64_t i = 0; i < n_tri; ++i) {
        const double* p = tris.data() + (size_t)i * 9;
        t[i] = signed_term(p, p + 3, p + 6);
        tneg[i] = signed_term(p, p + 6, p + 3);
    }
    for (int64_t i = 0; i < n_dec; ++i) {
        bool v = false;
        cls[i] = flip_class(decs[i].nonorientable != 0, decs[i].open != 0, decs[i].s, decs[i].faces, decs[i].par1, &v);
        byvol[i] = v ? 1 : 0;
        info[i] = root_info(decs[i].nonorientable != 0, decs[i].open != 0, decs[i].s, decs[i].faces, decs[i].par1);
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
    write_all(out, count);
    write_all(out, pos);
    write_all(out, cover);
    write_all(out, rkey);
    write_all(out, rval);
    write_all(out, t);
    write_all(out, tneg);
    write_all(out, cls);
    write_all(out, byvol);
    write_all(out, info);
    write_all(out, sums);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
