// The segment lookup and the workgroup layout of the ragged batches (morig_amd/csrc/ragged_core.h) as a plain host program, so that the text the kernels compile
// can be checked without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ragged_host_check.cpp -o ragged_host_check
//     ragged_host_check IN
// IN (text): the number of cases, then per case: n (segments), q (queries), the n + 1 entries of ptr, the q row indices.
// Prints four lines per case, segment_of for every query with (ptr type, index type) = (int32, int), (int32, int64), (int64, int),
// (int64, int64); "-" where a value does not fit the 32-bit type of that line. The tables hold ptr[0 .. n) and not ptr[n], in heap blocks
// of exactly that size: the search must not read further.
//     ragged_host_check --block-row IN
// IN: the number of cases, then per case: n (segments), width (rows per workgroup), the n + 1 entries of the row ptr, the n + 1 entries of
// blk_ptr. Prints one line per case: block_row for every (workgroup, thread) of the blk_ptr[n] workgroups as "seg:row", only where
// 0 <= row < rows(seg), the kernels' liveness test. blk_ptr is held as int32 in a heap block of n entries, as above.
// tests/test_ragged.py builds and runs it against numpy's searchsorted.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../morig_amd/csrc/ragged_core.h"

namespace {

template <class T> bool fits(const std::vector<long long>& v) {
    for (long long x : v)
        if (x < (long long)std::numeric_limits<T>::min() || x > (long long)std::numeric_limits<T>::max()) return false;
    return true;
}

template <class P, class I> void run(const std::vector<long long>& ptr, int n, const std::vector<long long>& queries) {
    if (!fits<P>(ptr) || !fits<I>(queries)) { printf("-\n"); return; }
    std::vector<P> table(ptr.begin(), ptr.begin() + n);
    for (size_t k = 0; k < queries.size(); ++k)
        printf(k ? " %d" : "%d", morig::segment_of(table.data(), n, (I)queries[k]));
    printf("\n");
}

int block_rows(FILE* in) {
    int cases = 0;
    if (fscanf(in, "%d", &cases) != 1 || cases < 0 || cases > (1 << 20)) { fprintf(stderr, "bad header\n"); return 2; }
    for (int c = 0; c < cases; ++c) {
        int n = 0, width = 0;
        if (fscanf(in, "%d %d", &n, &width) != 2 || n < 0 || n > (1 << 16) || width < 1 || width > 1024) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<long long> ptr(n + 1), blk(n + 1);
        for (std::vector<long long>* t : {&ptr, &blk})
            for (long long& v : *t)
                if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "bad table\n"); return 2; }
        if (!fits<int32_t>(blk) || blk[n] > (1 << 20)) { fprintf(stderr, "bad blk_ptr\n"); return 2; }
        std::vector<int32_t> table(blk.begin(), blk.begin() + n);
        for (int g = 0; g < (int)blk[n]; ++g)
            for (int t = 0; t < width; ++t) {
                const morig::BlockRow at = morig::block_row(table.data(), n, g, t, width);
                if (at.seg < 0 || at.seg >= n) { fprintf(stderr, "segment %d of %d\n", at.seg, n); return 1; }
                if (at.row >= 0 && at.row < ptr[at.seg + 1] - ptr[at.seg]) printf("%d:%lld ", at.seg, at.row);
            }
        printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--block-row") {
        FILE* in = fopen(argv[2], "r");
        if (!in) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        const int rc = block_rows(in);
        fclose(in);
        return rc;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s IN\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "r");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int cases = 0;
    if (fscanf(in, "%d", &cases) != 1 || cases < 0 || cases > (1 << 20)) { fprintf(stderr, "bad header\n"); return 2; }
    for (int c = 0; c < cases; ++c) {
        int n = 0, q = 0;
        if (fscanf(in, "%d %d", &n, &q) != 2 || n < 0 || n > (1 << 16) || q < 0 || q > (1 << 16)) { fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<long long> ptr(n + 1), queries(q);
        for (long long& v : ptr)
            if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "bad ptr\n"); return 2; }
        for (long long& v : queries)
            if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "bad query\n"); return 2; }
        run<int32_t, int>(ptr, n, queries);
        run<int32_t, int64_t>(ptr, n, queries);
        run<int64_t, int>(ptr, n, queries);
        run<int64_t, long long>(ptr, n, queries);
    }
    fclose(in);
    return 0;
}
