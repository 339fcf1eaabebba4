// The per-element arithmetic of csrc/motion_metrics.hip (morig_amd/csrc/curve_core.h) as a plain host program, so that it can be checked
// without a device and under the host sanitizers:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/curve_host_check.cpp -o curve_host_check
//     curve_host_check IN OUT
// IN  (binary, native endianness): int32 mode, int32 n_bins (1 .. 32), float32 [n_bins] the tolerances / thresholds; then
//     mode 0, one pair of morig_corr_hits: int32 n_pts, n_vtx, n_corr, nn_base; float32 [n_pts][3]; int32 [n_vtx] nn; int64 [n_corr][2];
//     mode 1, one mesh of morig_pr_counts: int32 n, normalize; float32 [n] pred; uint8 [n] gt.
// OUT: mode 0: int64 [n_bins] hits, then int64 the number of rows with an index outside the pair;
//      mode 1: int64 [n_bins] tp, int64 [n_bins] pp, int64 gp.
// The minimum / maximum of mode 1 is taken twice, serially and as the merge of four strided partial ranges (the shape of the kernel's
// reduction); the two must agree (exit status 3). tests/test_motion_metrics_host.py builds and runs it against
// tests/motion_metrics_oracle.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../morig_amd/csrc/curve_core.h"

template <class T> static bool get(FILE* in, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), in) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t head[2] = {0, 0};
    if (fread(head, 4, 2, in) != 2 || head[0] < 0 || head[0] > 1 || head[1] < 1 || head[1] > morig_curve::MAX_BINS) { fprintf(stderr, "bad header\n"); return 2; }
    const int mode = head[0], n_bins = head[1];
    std::vector<float> bins((size_t)n_bins);
    if (!get(in, bins)) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<int64_t> result;
    if (mode == 0) {
        int32_t dims[4];
        if (fread(dims, 4, 4, in) != 4 || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || dims[0] > (1 << 24) || dims[1] > (1 << 24) || dims[2] > (1 << 24)) {
            fprintf(stderr, "bad sizes\n");
            return 2;
        }
        const int n_pts = dims[0], n_vtx = dims[1], n_corr = dims[2], nn_base = dims[3];
        std::vector<float> pts((size_t)n_pts * 3);
        std::vector<int32_t> nn((size_t)n_vtx);
        std::vector<int64_t> corr((size_t)n_corr * 2);
        if (!get(in, pts) || !get(in, nn) || !get(in, corr)) { fprintf(stderr, "short input\n"); return 2; }
        result.assign((size_t)n_bins + 1, 0);
        for (int r = 0; r < n_corr; ++r) {
            int bad = 0;
            const uint32_t m = morig_curve::corr_row_mask(pts.data(), n_pts, nn.data(), n_vtx, nn_base, corr[2 * (size_t)r], corr[2 * (size_t)r + 1],
                                                          bins.data(), n_bins, &bad);
            result[(size_t)n_bins] += bad;
            for (int b = 0; b < n_bins; ++b) result[(size_t)b] += (m >> b) & 1u;
        }
    } else {
        int32_t dims[2];
        if (fread(dims, 4, 2, in) != 2 || dims[0] < 0 || dims[0] > (1 << 26)) { fprintf(stderr, "bad sizes\n"); return 2; }
        const int n = dims[0], normalize = dims[1];
        std::vector<float> pred((size_t)n);
        std::vector<uint8_t> gt((size_t)n);
        if (!get(in, pred) || !get(in, gt)) { fprintf(stderr, "short input\n"); return 2; }
        float mn = 0.f, mx = 1.f;
        if (normalize) {
            morig_curve::Range serial = morig_curve::range_empty(), part[4];
            for (int k = 0; k < 4; ++k) part[k] = morig_curve::range_empty();
            for (int i = 0; i < n; ++i) {
                serial = morig_curve::range_add(serial, pred[(size_t)i]);
                part[i & 3] = morig_curve::range_add(part[i & 3], pred[(size_t)i]);
            }
            float mn2, mx2;
            morig_curve::range_finish(serial, &mn, &mx);
            morig_curve::range_finish(morig_curve::range_merge(morig_curve::range_merge(part[0], part[1]), morig_curve::range_merge(part[2], part[3])),
                                      &mn2, &mx2);
            const bool same_mn = mn == mn2 || (mn != mn && mn2 != mn2), same_mx = mx == mx2 || (mx != mx && mx2 != mx2);      // +0 == -0: no count sees the sign
            if (!same_mn || !same_mx) { fprintf(stderr, "the merged range differs from the serial one\n"); return 3; }
        }
        result.assign((size_t)n_bins * 2 + 1, 0);
        for (int i = 0; i < n; ++i) {
            const float x = normalize ? morig_curve::normalised(pred[(size_t)i], mn, mx) : pred[(size_t)i];
            const uint32_t above = morig_curve::bin_mask(x, bins.data(), n_bins, 0);
            const uint32_t g = gt[(size_t)i] != 0 ? 0xffffffffu : 0u;
            result[(size_t)n_bins * 2] += g & 1u;
            for (int b = 0; b < n_bins; ++b) {
                result[(size_t)b] += ((above & g) >> b) & 1u;
                result[(size_t)n_bins + b] += (above >> b) & 1u;
            }
        }
    }
    fwrite(result.data(), 8, result.size(), out);
    fclose(in);
    if (fclose(out) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    return 0;
}
