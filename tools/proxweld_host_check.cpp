// The shared arithmetic of csrc/proxweld.hip (morig_amd/csrc/proxweld_core.h) as a plain host program, so that it can be checked
// without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/proxweld_host_check.cpp -o proxweld_host_check
//     proxweld_host_check IN OUT
// IN  (binary, native endianness): int64 n_cases, then per case int64 n_points, float64 eps, n_points x 3 float64. Every point with
//     three finite coordinates is a node.
// OUT: per case 4 float64 (the low corner of the finite box and the cell side), per point 3 int64 (its cell, -1 for a point that is no
//     node), int64 n_links, then n_links x 2 int64: the links (u, w), u < w, that the walk over the sorted cell keys finds, ascending.
// The program does what the kernels do with the same functions: the box by integer minima and maxima on the coordinate keys, the frame,
// the cell keys, a stable sort by key, the walk of every sorted position. tests/test_proxweld_oracle.py builds and runs it against the
// brute force of tests/proxweld_oracle.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <utility>
#include <vector>

#include "../morig_amd/csrc/proxweld_core.h"

namespace {

bool read_count(FILE* in, int64_t* n) { return fread(n, 8, 1, in) == 1 && *n >= 0 && *n <= (1 << 22); }

}  // namespace

int main(int argc, char** argv) {
    using namespace morig_prox;
    using namespace morig_topo;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int64_t n_cases = 0;
    if (!read_count(in, &n_cases)) { fprintf(stderr, "short input\n"); return 2; }
    for (int64_t c = 0; c < n_cases; ++c) {
        int64_t n = 0;
        double eps = 0.0;
        if (!read_count(in, &n) || fread(&eps, 8, 1, in) != 1) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<double> pts((size_t)n * 3);
        if (n > 0 && fread(pts.data(), 24, (size_t)n, in) != (size_t)n) { fprintf(stderr, "short input\n"); return 2; }
        // the box over the finite points, on the coordinate keys
        long long lo_key[3] = {KEY_NONE, KEY_NONE, KEY_NONE}, hi_key[3] = {-KEY_NONE - 1, -KEY_NONE - 1, -KEY_NONE - 1};
        std::vector<char> node((size_t)n);
        for (int64_t v = 0; v < n; ++v) {
            node[v] = morig_topo::finite(pts[v * 3]) && morig_topo::finite(pts[v * 3 + 1]) && morig_topo::finite(pts[v * 3 + 2]);
            if (!node[v]) continue;
            for (int d = 0; d < 3; ++d) {
                const long long k = coord_key(pts[v * 3 + d]);
                lo_key[d] = std::min(lo_key[d], k);
                hi_key[d] = std::max(hi_key[d], k);
            }
        }
        double frame[4] = {0.0, 0.0, 0.0, 0.0}, extent = 0.0;
        if (lo_key[0] != KEY_NONE)
            for (int d = 0; d < 3; ++d) {
                frame[d] = key_coord(lo_key[d]);
                const double e = key_coord(hi_key[d]) - frame[d];
                extent = e > extent ? e : extent;
            }
        frame[3] = cell_side(eps, extent);
        fwrite(frame, 8, 4, out);
        std::vector<long long> keys((size_t)n, KEY_NONE);
        for (int64_t v = 0; v < n; ++v) {
            long long cell[3] = {-1, -1, -1};
            if (node[v]) {
                for (int d = 0; d < 3; ++d) cell[d] = cell_coord(pts[v * 3 + d], frame[d], frame[3]);
                keys[v] = cell_key(cell[0], cell[1], cell[2]);
                if (key_x(keys[v]) != cell[0] || key_y(keys[v]) != cell[1] || key_z(keys[v]) != cell[2]) { fprintf(stderr, "key round trip\n"); return 1; }
            }
            fwrite(cell, 8, 3, out);
        }
        // the sort by key (stable: equal keys stay in ascending row order), then the walk of every sorted position
        std::vector<long long> order((size_t)n), skeys((size_t)n);
        std::iota(order.begin(), order.end(), 0LL);
        std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return keys[a] < keys[b]; });
        std::vector<double> pos((size_t)n * 3);
        for (int64_t i = 0; i < n; ++i) {
            skeys[i] = keys[order[i]];
            for (int d = 0; d < 3; ++d) pos[i * 3 + d] = pts[order[i] * 3 + d];
        }
        std::vector<std::pair<long long, long long>> links;
        const double eps2 = eps * eps;
        for (int64_t i = 0; i < n; ++i)
            walk_links(skeys.data(), order.data(), pos.data(), n, i, 0, n, eps2, [&](long long other) { links.emplace_back(order[i], other); });
        std::sort(links.begin(), links.end());
        const int64_t n_links = (int64_t)links.size();
        fwrite(&n_links, 8, 1, out);
        for (const auto& l : links) {
            const long long pair[2] = {l.first, l.second};
            fwrite(pair, 8, 2, out);
            if (edge_lo(edge_key(l.first, l.second)) != l.first || edge_hi(edge_key(l.first, l.second)) != l.second) { fprintf(stderr, "edge key\n"); return 1; }
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
