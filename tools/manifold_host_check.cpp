// The shared arithmetic of csrc/meshsplit.hip (morig_amd/csrc/fan_core.h) as a plain host program, so that it can be checked without a
// device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/manifold_host_check.cpp -o manifold_host_check
//     manifold_host_check IN OUT
// IN  (binary, native endianness): int64 n_faces, then per face 3 int64 rows (three different rows per face, no duplicate face).
// OUT: per sorted record int64 its corner link, then per sorted record int32 the non-manifold mark.
// The program makes the records of every face (orient_core.h), sorts them stably by key with the permutation, asks fan_core.h for the
// link of every sorted position, and compares the result with a BRUTE-FORCE corner table: for every undirected edge the faces that
// hold it, found by a scan over all faces, and in each the corners that name its low and its high end, found by comparing rows. It
// exits 1 on the first difference. tests/test_manifold_oracle.py builds and runs it and compares OUT with tests/manifold_oracle.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../morig_amd/csrc/fan_core.h"

namespace {

template <class T> void write_all(FILE* out, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out);
}

int corner_of(const long long* face, long long row) {
    for (int c = 0; c < 3; ++c)
        if (face[c] == row) return c;
    return -1;
}

}  // namespace

int main(int argc, char** argv) {
    using namespace morig_fan;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t n_faces = 0;
    if (fread(&n_faces, 8, 1, in) != 1 || n_faces < 0 || n_faces > (1 << 20)) { fprintf(stderr, "bad count\n"); return 2; }
    std::vector<long long> faces((size_t)n_faces * 3);
    if (n_faces && fread(faces.data(), 8, faces.size(), in) != faces.size()) { fprintf(stderr, "short input\n"); return 2; }
    fclose(in);
    const long long n = 3 * n_faces;
    std::vector<long long> keys((size_t)n), order((size_t)n), skeys((size_t)n), links((size_t)n);
    std::vector<int> vals((size_t)n), svals((size_t)n);
    std::vector<int32_t> nm((size_t)n);
    for (long long f = 0; f < n_faces; ++f)
        for (int c = 0; c < 3; ++c) {
            const long long a = faces[f * 3 + c], d = faces[f * 3 + (c + 1) % 3];
            keys[f * 3 + c] = morig_orient::record_key(a, d);
            vals[f * 3 + c] = morig_orient::record_val((int)f, a, d);
        }
    std::iota(order.begin(), order.end(), 0LL);
    std::stable_sort(order.begin(), order.end(), [&](long long x, long long y) { return keys[x] < keys[y]; });
    for (long long i = 0; i < n; ++i) { skeys[i] = keys[order[i]]; svals[i] = vals[order[i]]; }
    for (long long i = 0; i < n; ++i) {
        int count, pos;
        links[i] = fan_link(skeys.data(), svals.data(), order.data(), i, n, n_faces, &count, &pos);
        nm[i] = (count >= 3 && pos == 0) ? 1 : 0;
        // the brute-force table of this record's edge
        const long long lo = skeys[i] >> 32, hi = skeys[i] & 0xffffffffLL;
        std::vector<long long> holders;
        for (long long f = 0; f < n_faces; ++f)
            if (corner_of(&faces[f * 3], lo) >= 0 && corner_of(&faces[f * 3], hi) >= 0) holders.push_back(f);
        long long before = 0;
        for (long long j = i; j > 0 && skeys[j - 1] == skeys[i]; --j) ++before;
        long long want = KEY_NONE;
        if (holders.size() == 2) {
            const long long f = holders[0], g = holders[1], end = before == 0 ? lo : hi;
            want = ((3 * f + corner_of(&faces[f * 3], end)) << 32) | ((3 * g + corner_of(&faces[g * 3], end)) << 1);
        }
        const int want_nm = holders.size() >= 3 && before == 0 ? 1 : 0;
        if (links[i] != want || nm[i] != want_nm || count != (int)std::min<size_t>(holders.size(), 3) || pos != (int)std::min<long long>(before, 2)) {
            fprintf(stderr, "record %lld (edge %lld, %lld): link %llx, expected %llx; mark %d, expected %d\n", i, lo, hi, (unsigned long long)links[i],
                    (unsigned long long)want, nm[i], want_nm);
            return 1;
        }
    }
    // node_at_lo / node_at_hi on every record, against the rows
    for (long long r = 0; r < n; ++r) {
        const long long a = faces[r], d = faces[(r - r % 3) + (r % 3 + 1) % 3];
        const int dir = a < d ? 1 : 0;
        if (faces[node_at_lo(r, dir)] != std::min(a, d) || faces[node_at_hi(r, dir)] != std::max(a, d)) {
            fprintf(stderr, "record %lld: the corners at its ends are wrong\n", r);
            return 1;
        }
    }
    write_all(out, links);
    write_all(out, nm);
    fclose(out);
    return 0;
}
