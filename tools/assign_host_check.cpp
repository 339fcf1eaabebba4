// The joint-matching core of csrc/metrics.hip (morig_amd/csrc/assign_core.h) as a plain host program, so that the algorithm can be
// checked without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/assign_host_check.cpp -o assign_host_check
//     assign_host_check IN OUT
// IN  (binary, native endianness): int32 n_problems, then per problem int32 n_rows, int32 n_cols and n_rows * n_cols float64, row-major.
// OUT: per problem int32 status (0 solved, 1 beyond the supported size, 4 no finite assignment), int32 n_pairs, then n_pairs int32
//      row indices (ascending) and n_pairs int32 column indices -- no pairs unless solved.
// The matrix goes into the solver's orientation through solver_index, exactly as the kernel fills its workspace; the arrays are sized to
// the problem (not to the maxima), so an index past a problem's rows or columns is an AddressSanitizer report.
// tests/test_metrics_host.py builds and runs it against scipy.optimize.linear_sum_assignment.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/assign_core.h"

static bool read_exact(void* dst, size_t size, size_t n, FILE* f) { return n == 0 || fread(dst, size, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_problems = 0;
    if (!read_exact(&n_problems, 4, 1, in) || n_problems < 0) { fprintf(stderr, "bad header\n"); return 2; }
    for (int32_t q = 0; q < n_problems; ++q) {
        int32_t dims[2];
        if (!read_exact(dims, 4, 2, in) || dims[0] < 0 || dims[1] < 0 || dims[0] > 4096 || dims[1] > 4096) { fprintf(stderr, "bad problem %d\n", q); return 2; }
        const int n_rows = dims[0], n_cols = dims[1];
        std::vector<double> given((size_t)n_rows * n_cols);
        if (!read_exact(given.data(), 8, given.size(), in)) { fprintf(stderr, "short problem %d\n", q); return 2; }
        int32_t head[2] = {0, 0};
        std::vector<int32_t> row_ind, col_ind;
        if (!morig_assign::supported(n_rows, n_cols)) {
            head[0] = 1;
        } else {
            const bool tr = morig_assign::transposed(n_rows, n_cols);
            const int nr = tr ? n_cols : n_rows, nc = tr ? n_rows : n_cols;
            std::vector<double> cost((size_t)nr * nc), u(nr), v(nc), shortest(nc);
            std::vector<int> path(nc), col4row(nr), row4col(nc);
            std::vector<unsigned char> in_SR(nr), in_SC(nc);
            for (int r = 0; r < n_rows; ++r)
                for (int c = 0; c < n_cols; ++c) cost[morig_assign::solver_index(r, c, n_rows, n_cols)] = given[(size_t)r * n_cols + c];
            morig_assign::State st = {u.data(), v.data(), shortest.data(), path.data(), col4row.data(), row4col.data(), in_SR.data(), in_SC.data()};
            morig_assign::OneLane lanes;
            if (!morig_assign::solve(cost.data(), nr, nc, st, lanes)) {
                head[0] = 4;
            } else {
                head[1] = nr;
                row_ind.assign(nr, -1);
                col_ind.assign(nr, -1);
                morig_assign::emit(st, n_rows, n_cols, row_ind.data(), col_ind.data(), lanes);
            }
        }
        fwrite(head, 4, 2, out);
        if (!row_ind.empty()) {
            fwrite(row_ind.data(), 4, row_ind.size(), out);
            fwrite(col_ind.data(), 4, col_ind.size(), out);
        }
    }
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
