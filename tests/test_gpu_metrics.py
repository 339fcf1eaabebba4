"""csrc/metrics.hip and morig_amd/metrics.py on the device, against the reference's recorded results (tests/golden/metrics_match.npz,
metrics_skel.npz; tools/make_metrics_golden.py) and tests/metrics_oracle.py.

Bounds: bone samples, squared nearest distances, the matching, hits, IoU, precision and recall are compared bit for bit (the matching by
total cost on the tie case). A distance is a square root of a bit-equal number: within 1 ulp, bit equal when the device's float64 square
root is correctly rounded (the test prints which; DESIGN.md section 15 records it). Every per-mesh mean and chamfer: SUM_TOL = 1e-11
absolute, from n <= 4096 terms below 4 (tests/test_metrics_oracle.py). Figures are printed before they are asserted (run with -s)."""
import numpy as np
import pytest
import torch

import metrics_oracle as mo
from morig_amd import metrics
from morig_amd.runtime import get_ops
from test_metrics_oracle import (GAP, MATCH, MATCH_META, N_SKEL, SHAPES, SKEL, SKEL_META, SUM_TOL, chain_rig, match_mesh, skel_eval_inputs,
                                 skel_rigs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}
host = lambda t: t.cpu().numpy()


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def all_rigs():
    return cached("rigs", lambda: [r for i in range(N_SKEL) for r in skel_rigs(i)])


def sampled():
    def run():
        samples, ptr = metrics.sample_skel(all_rigs(), device=DEV)
        return host(samples), host(ptr)
    return cached("samples", run)


def matched():
    return cached("match", lambda: metrics.match_joints(MATCH["pred"], MATCH["pred_ptr"], MATCH["gt"], MATCH["gt_ptr"], device=DEV))


def ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64)).max(initial=0)


# ------------------------------------------------------------------------------------------------------------------- bone samples
def test_sample_skel_equals_the_reference_bit_for_bit():
    samples, ptr = sampled()
    want = [SKEL[f"samples_{t}{i}"] for i in range(N_SKEL) for t in "ab"]
    counts = np.diff(ptr).tolist()
    print("bone-sample counts", counts)
    assert counts == [len(w) for w in want] and counts[0] == 40                                  # the star: half steps round to even
    assert samples.shape == (ptr[-1], 3) and np.array_equal(samples, np.concatenate(want))
    # the star's bones one by one: 1.5 -> 2, 2.5 -> 2, 4.5 -> 4, 5.5 -> 6, 6.5 -> 6, 7.5 -> 8 steps, the near miss of 3.5 and the zero-length bone
    star = all_rigs()[0]
    per_bone = [len(mo.sample_bone(star.pos[p], star.pos[c])) for p, c in mo.bones_of(star)]
    assert per_bone[:6] == [3, 3, 5, 7, 7, 9] and per_bone[7] == 1 and sum(per_bone) == counts[0]


# --------------------------------------------------------------------------------------------------------------- nearest distances
def test_nearest_distance_minima_are_bit_equal_and_distances_within_one_ulp():
    """sample sets against each other (past one LDS tile of b, several workgroups of a that span meshes) and joints against joints"""
    a_sets = [SKEL[f"samples_a{i}"] for i in range(N_SKEL)]
    b_sets = [SKEL[f"samples_b{i}"] for i in range(N_SKEL)]
    a, b = np.concatenate(a_sets), np.concatenate(b_sets)
    pa, pb = np.concatenate([[0], np.cumsum([len(x) for x in a_sets])]), np.concatenate([[0], np.cumsum([len(x) for x in b_sets])])
    want = np.concatenate([mo.nearest_sq(x, y) for x, y in zip(a_sets, b_sets)])
    sq = host(metrics.nearest_distance(a, pa, b, pb, squared=True, device=DEV))
    d = host(metrics.nearest_distance(a, pa, b, pb, device=DEV))
    off = ulps(d, np.sqrt(want))
    print(f"nearest_distance: {len(a)} sources, b sets up to {max(len(x) for x in b_sets)}; sqrt differs from numpy's by at most {off} ulp "
          f"({'correctly rounded here' if off == 0 else 'not correctly rounded'})")
    assert np.array_equal(sq, want) and off <= 1
    pred, gt = MATCH["pred"], MATCH["gt"]
    d, flags = metrics.nearest_distance(gt, MATCH["gt_ptr"], pred, MATCH["pred_ptr"], squared=True, return_flags=True, device=DEV)
    want = np.concatenate([mo.nearest_sq(match_mesh(m)[1], match_mesh(m)[0]) for m in range(len(SHAPES) - 1)])
    assert np.array_equal(host(d)[:len(want)], want) and np.isnan(host(d)[len(want):]).all() and host(flags).tolist() == [0] * 9 + [1]


def test_chamfers_are_within_the_summation_bound_of_the_reference():
    pairs = [skel_rigs(i) for i in range(N_SKEL)]
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    j2b, b2b = host(metrics.chamfer_j2b(a, b, device=DEV)), host(metrics.chamfer_b2b(a, b, device=DEV))
    j2j = host(metrics.chamfer_j2j(np.concatenate([r.pos for r in a]), np.concatenate([[0], np.cumsum([len(r.pos) for r in a])]),
                                   np.concatenate([r.pos for r in b]), np.concatenate([[0], np.cumsum([len(r.pos) for r in b])]), device=DEV))
    mj = host(metrics.chamfer_j2j(MATCH["pred"], MATCH["pred_ptr"], MATCH["gt"], MATCH["gt_ptr"], device=DEV))
    figs = dict(j2b=np.abs(j2b - SKEL["chamfer_j2b"]).max(), b2b=np.abs(b2b - SKEL["chamfer_b2b"]).max(),
                j2j=np.abs(j2j - SKEL["chamfer_j2j"]).max(), j2j_match=np.abs(mj[:-1] - MATCH["chamfer_j2j"][:-1]).max())
    print("chamfer |device - reference| max:", {k: f"{v:.2e}" for k, v in figs.items()}, "bound", SUM_TOL)
    assert max(figs.values()) <= SUM_TOL and np.isnan(mj[-1])
    # the per-mesh one-way means themselves
    sa = [SKEL[f"samples_a{i}"] for i in range(N_SKEL)]
    sb = [SKEL[f"samples_b{i}"] for i in range(N_SKEL)]
    pa, pb = np.concatenate([[0], np.cumsum([len(x) for x in sa])]), np.concatenate([[0], np.cumsum([len(x) for x in sb])])
    d = metrics.nearest_distance(np.concatenate(sa), pa, np.concatenate(sb), pb, device=DEV)
    means = host(get_ops().segment_mean(d, torch.from_numpy(pa.astype(np.int32)).to(DEV)))
    want = np.array([mo.oneway(x, y) for x, y in zip(sa, sb)])
    print("one-way means |device - oracle| max:", f"{np.abs(means - want).max():.2e}")
    assert np.abs(means - want).max() <= SUM_TOL


# ------------------------------------------------------------------------------------------------------------------------- matching
def test_match_joints_returns_scipys_assignment_on_the_parity_cases():
    m = matched()
    assert host(m["match_ptr"]).tolist() == MATCH["match_ptr"].tolist() and host(m["status"]).tolist() == [0] * len(SHAPES)
    row, col = host(m["row_ind"]), host(m["col_ind"])
    for b, shape in enumerate(SHAPES):
        m0, m1 = MATCH["match_ptr"][b], MATCH["match_ptr"][b + 1]
        assert np.array_equal(row[m0:m1], MATCH["row_ind"][m0:m1]) and np.array_equal(col[m0:m1], MATCH["col_ind"][m0:m1]), (b, shape)
    off = ulps(host(m["dist"]), MATCH["dist"])
    print("matched distances differ from numpy's by at most", off, "ulp")
    assert off <= 1


def test_tie_case_reaches_the_optimal_total():
    m = metrics.match_joints(MATCH["tie_pred"], [0, len(MATCH["tie_pred"])], MATCH["tie_gt"], [0, len(MATCH["tie_gt"])], device=DEV)
    row, col, dist = host(m["row_ind"]), host(m["col_ind"]), host(m["dist"])
    d = mo.dist_matrix(MATCH["tie_pred"], MATCH["tie_gt"])
    assert row.tolist() == list(range(6)) and len(set(col.tolist())) == 6 and col.min() >= 0 and col.max() < 8
    assert np.array_equal(dist, d[row, col]) and dist.sum() == MATCH_META["tie_total"]


def test_largest_supported_size_in_both_orientations():
    """128 x 256 and 256 x 128 (the cost matrix in global memory), and 48 x 128 / 128 x 48 (6144 entries: the largest that sits in LDS)"""
    rng = np.random.default_rng(11)
    sizes = [(128, 256), (256, 128), (48, 128), (128, 48)]
    gt, pred = [rng.random((g, 3)) for g, _ in sizes], [rng.random((p, 3)) for _, p in sizes]
    ptr = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    m = metrics.match_joints(np.concatenate(pred), ptr(pred), np.concatenate(gt), ptr(gt), device=DEV)
    row, col = host(m["row_ind"]), host(m["col_ind"])
    assert host(m["status"]).tolist() == [0] * 4
    for b in range(4):
        m0, m1 = m["match_ptr_host"][b], m["match_ptr_host"][b + 1]
        d = mo.dist_matrix(pred[b], gt[b])
        want_row, want_col = mo.linear_sum_assignment(d)
        total, want = d[row[m0:m1], col[m0:m1]].sum(), d[want_row, want_col].sum()
        print(f"{sizes[b]}: total {total:.12f}, scipy {want:.12f}")
        assert (np.diff(row[m0:m1]) > 0).all() and len(set(col[m0:m1].tolist())) == m1 - m0 and abs(total - want) <= 1e-9
        if b >= 2 and mo.assignment_gap(d) > GAP:
            assert np.array_equal(row[m0:m1], want_row) and np.array_equal(col[m0:m1], want_col)


def test_scores_are_exact():
    m = matched()
    sc = metrics.joint_scores(m, m["n_pred"], m["n_gt"], MATCH["fs"], MATCH["gt_ptr"], device=DEV)
    assert host(sc["hits"]).tolist() == MATCH["hits"].tolist()
    for k in ("iou", "precision", "recall"):
        assert np.array_equal(host(sc[k])[:-1], MATCH[k][:-1]), k                               # bit equal


# ------------------------------------------------------------------------------------------------------------------- evaluate_rigs
def evaluated():
    def run():
        n = len(SHAPES)
        return metrics.evaluate_rigs(MATCH["pred"], MATCH["pred_ptr"], [chain_rig(match_mesh(b)[1]) for b in range(n)],
                                     [match_mesh(b)[2] for b in range(n)], device=DEV)
    return cached("eval", run)


def test_evaluate_rigs_valid_means_and_report():
    res = evaluated()
    n = len(SHAPES)
    want = mo.evaluate([match_mesh(b)[0] for b in range(n)], [chain_rig(match_mesh(b)[1]) for b in range(n)], [match_mesh(b)[2] for b in range(n)])
    assert res["num_invalid"] == 1 and host(res["valid"]).tolist() == [True] * 9 + [False]
    for k in ("iou", "precision", "recall"):
        assert np.array_equal(host(res[k]), want[k], equal_nan=True) and float(res["mean"][k]) == want["mean"][k] == MATCH["means"][1 + ("iou", "precision", "recall").index(k)]
    print("CD-J2J mean |device - reference|", abs(float(res["mean"]["chamfer_j2j"]) - MATCH["means"][0]))
    assert abs(float(res["mean"]["chamfer_j2j"]) - MATCH["means"][0]) <= SUM_TOL
    assert metrics.format_report(res) == mo.format_report(want) == MATCH_META["report"]


def test_evaluate_rigs_with_predicted_rigs():
    preds, pred_rigs, gt_rigs, fss = skel_eval_inputs()
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in preds])])
    res = metrics.evaluate_rigs(np.concatenate(preds), ptr, gt_rigs, fss, pred_rigs=pred_rigs, device=DEV)
    want = mo.evaluate(preds, gt_rigs, fss, pred_rigs)
    keys = ("chamfer_j2j", "iou", "precision", "recall", "chamfer_j2b", "chamfer_b2b")
    assert res["num_invalid"] == 1 and host(res["valid"]).tolist() == [True] * 5 + [False]
    for j, k in enumerate(keys):
        assert np.abs(host(res[k])[:-1] - want[k][:-1]).max() <= SUM_TOL and np.isnan(host(res[k])[-1]), k
        assert abs(float(res["mean"][k]) - SKEL["eval_means"][j]) <= SUM_TOL, k
    assert host(res["hits"]).tolist() == SKEL["eval_hits"].tolist() + [0]
    assert metrics.format_report(res) == mo.format_report(want) == SKEL_META["report"]


def test_each_mesh_alone_gives_the_bits_it_gives_in_the_batch():
    res = evaluated()
    m = matched()
    row, col = host(m["row_ind"]), host(m["col_ind"])
    for b in range(len(SHAPES) - 1):
        pred, gt, fs = match_mesh(b)
        one = metrics.evaluate_rigs(pred, [0, len(pred)], [chain_rig(gt)], [fs], device=DEV)
        for k in ("chamfer_j2j", "iou", "precision", "recall"):
            assert host(one[k])[0].tobytes() == host(res[k])[b].tobytes(), (b, k)
        m0, m1 = MATCH["match_ptr"][b], MATCH["match_ptr"][b + 1]
        assert np.array_equal(host(one["match"]["row_ind"]), row[m0:m1]) and np.array_equal(host(one["match"]["col_ind"]), col[m0:m1])
    samples, ptr = sampled()
    rigs = all_rigs()
    for i in (0, 8, 9):                                                                        # the star, and the two largest sample sets
        alone, p = metrics.sample_skel([rigs[i]], device=DEV)
        assert host(p).tolist() == [0, ptr[i + 1] - ptr[i]] and np.array_equal(host(alone), samples[ptr[i]:ptr[i + 1]])
    pairs = [skel_rigs(i) for i in range(N_SKEL)]
    both = metrics.chamfer_b2b([p[0] for p in pairs], [p[1] for p in pairs], device=DEV)
    alone = metrics.chamfer_b2b([pairs[4][0]], [pairs[4][1]], device=DEV)
    assert host(alone)[0].tobytes() == host(both)[4].tobytes()


def test_a_second_run_gives_the_same_bits():
    first, m = evaluated(), matched()
    n = len(SHAPES)
    again = metrics.evaluate_rigs(MATCH["pred"], MATCH["pred_ptr"], [chain_rig(match_mesh(b)[1]) for b in range(n)],
                                  [match_mesh(b)[2] for b in range(n)], device=DEV)
    for k in ("chamfer_j2j", "iou", "precision", "recall", "hits"):
        assert host(again[k]).tobytes() == host(first[k]).tobytes(), k
    for k in ("row_ind", "col_ind", "dist"):
        assert host(again["match"][k]).tobytes() == host(m[k]).tobytes(), k
    assert all(host(again["mean"][k]).tobytes() == host(first["mean"][k]).tobytes() for k in first["mean"])
    samples, _ = sampled()
    assert np.array_equal(host(metrics.sample_skel(all_rigs(), device=DEV)[0]), samples)


def test_a_mesh_above_the_supported_size_raises_and_leaves_the_others_intact():
    rng = np.random.default_rng(5)
    sizes = [(7, 7), (129, 130), (33, 20), (2, 257)]                                           # (n_gt, n_pred)
    gt, pred = [rng.random((g, 3)) for g, _ in sizes], [rng.random((p, 3)) for _, p in sizes]
    ptr = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    with pytest.raises(metrics.AssignmentSizeError) as e:
        metrics.match_joints(np.concatenate(pred), ptr(pred), np.concatenate(gt), ptr(gt), device=DEV)
    assert e.value.meshes == [1, 3] and e.value.sizes == [(129, 130), (2, 257)]
    res = e.value.result
    assert host(res["status"]).tolist() == [0, 1, 0, 1]                                        # the kernel's status word says the same
    row, col, dist = host(res["row_ind"]), host(res["col_ind"]), host(res["dist"])
    for b in (0, 2):
        m0, m1 = res["match_ptr_host"][b], res["match_ptr_host"][b + 1]
        want_row, want_col, _ = mo.match(pred[b], gt[b])
        assert np.array_equal(row[m0:m1], want_row) and np.array_equal(col[m0:m1], want_col)
    for b in (1, 3):
        m0, m1 = res["match_ptr_host"][b], res["match_ptr_host"][b + 1]
        assert (row[m0:m1] == -1).all() and (col[m0:m1] == -1).all() and np.isnan(dist[m0:m1]).all()
