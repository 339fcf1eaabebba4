// The segment lookup of the ragged batches (morig_amd/csrc/ragged_core.h) as a plain host program, so that the text the kernels compile
// can be checked without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ragged_host_check.cpp -o ragged_host_check
//     ragged_host_check IN
// IN (text): the number of cases, then per case: n (segments), q (queries), the n + 1 entries of ptr, the q row indices.
// Prints four lines per case, segment_of for every query with (ptr type, index type) = (int32, int), (int32, int64), (int64, int),
// (int64, int64); "-" where a value does not fit the 32-bit type of that line. The tables hold ptr[0 .. n) and not ptr[n], in heap blocks
// of exactly that size: the search must not read further.
// tests/test_ragged.py builds and runs it against numpy's searchsorted.
#include <cstdint>
#include <cstdio>
#include <limits>
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

}  // namespace

int main(int argc, char** argv) {
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
