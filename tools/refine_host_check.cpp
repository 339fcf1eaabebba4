// The shared arithmetic of csrc/refine.hip (morig_amd/csrc/split_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/refine_host_check.cpp -o refine_host_check
//     refine_host_check IN OUT
// IN  (binary, native endianness): int64 n_faces, then per face 3 int64 corners, 3 int64 new vertices (negative: the edge from that
//     corner to the next is not marked) and 9 float64 (the positions of the corners); int64 n_pairs, then per pair 6 float64 (p, q).
// OUT: per face int32 the mask, int32 the rotation, int32 the diagonal (0 unless two edges are marked), int32 the number of children and
//     12 int64: the children, -1 behind the last; per pair float64 len2(p, q), float64 len2(q, p), int64 the image of len2(p, q), 3 float64
//     the midpoint.
// tests/test_refine_oracle.py builds and runs it against tests/refine_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/split_core.h"

namespace {

bool read_count(FILE* in, int64_t* n) { return fread(n, 8, 1, in) == 1 && *n >= 0 && *n <= (1 << 24); }

struct Face { int64_t v[3], mid[3]; double pos[9]; };
struct Pair { double p[3], q[3]; };

template <class T> bool read_all(FILE* in, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, in) == n;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace morig_split;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    static_assert(sizeof(Face) == 120 && sizeof(Pair) == 48, "packed 8-byte fields");
    int64_t n_faces = 0, n_pairs = 0;
    std::vector<Face> faces;
    std::vector<Pair> pairs;
    if (!read_count(in, &n_faces) || !read_all(in, faces, (size_t)n_faces) || !read_count(in, &n_pairs) || !read_all(in, pairs, (size_t)n_pairs)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    for (const Face& f : faces) {
        const int mid32[3] = {(int)f.mid[0], (int)f.mid[1], (int)f.mid[2]};
        const int mask = mask_of(mid32), r = rotation(mask);
        int diag = 0;
        if (marked_edges(mask) == 2)
            diag = frame_diagonal(f.pos + 3 * r, f.pos + 3 * ((r + 1) % 3), f.pos + 3 * ((r + 2) % 3), f.v[(r + 1) % 3], f.v[(r + 2) % 3]);
        long long kids[4][3];
        for (auto& k : kids) k[0] = k[1] = k[2] = -1;
        const long long v[3] = {f.v[0], f.v[1], f.v[2]}, mid[3] = {f.mid[0], f.mid[1], f.mid[2]};
        const int made = children(v, mid, mask, diag, kids);
        const int32_t head[4] = {mask, r, diag, made};
        fwrite(head, 4, 4, out);
        fwrite(kids, 8, 12, out);
        if (made != child_count(mask)) { fprintf(stderr, "child count\n"); return 1; }
    }
    for (const Pair& p : pairs) {
        double m[3];
        midpoint(p.p, p.q, m);
        const double l[2] = {len2(p.p, p.q), len2(p.q, p.p)};
        const long long image = len2_image(l[0]);
        fwrite(l, 8, 2, out);
        fwrite(&image, 8, 1, out);
        fwrite(m, 8, 3, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
