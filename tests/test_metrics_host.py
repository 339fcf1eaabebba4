"""CPU: (1) the matching core csrc/assign_core.h as the stand-alone program tools/assign_host_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program (never loaded into Python), against scipy's linear_sum_assignment; (2) the host logic
of morig_amd/metrics.py on an emulated op layer (tests/metrics_emulate.py through ``runtime._test_ops``): ptr handling, the invalid-mesh
bookkeeping, the report text, the ValueError of a rig without bones and the size refusal."""
import numpy as np
import pytest
import torch

import metrics_emulate
import metrics_oracle as mo
from morig_amd import metrics, runtime
from test_metrics_oracle import (GAP, MATCH, MATCH_META, SHAPES, SKEL, SKEL_META, SUM_TOL, chain_rig, match_mesh, skel_eval_inputs, skel_rigs)


# ------------------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    work = tmp_path_factory.mktemp("assign_host_check")
    exe = mo.build_host_check(work)
    return lambda matrices: mo.run_host_check(exe, matrices, work)


def check_against_scipy(matrices, results, by_assignment):
    """a valid one-to-one matching with ascending rows and scipy's total everywhere; scipy's very assignment where the optimum is unique"""
    for k, (d, (status, row, col)) in enumerate(zip(matrices, results)):
        want_row, want_col = mo.linear_sum_assignment(d)
        assert status == 0 and len(row) == len(col) == min(d.shape), k
        assert (np.diff(row) > 0).all() and len(set(col.tolist())) == len(col), k
        assert row.min(initial=0) >= 0 and row.max(initial=0) < max(d.shape[0], 1) and col.min(initial=0) >= 0 and col.max(initial=0) < max(d.shape[1], 1), k
        total, want = d[row, col].sum(), d[want_row, want_col].sum()
        assert abs(total - want) <= 1e-9 * max(1.0, abs(want)), (k, total, want)
        if by_assignment(k):
            assert np.array_equal(row, want_row) and np.array_equal(col, want_col), k


def test_host_program_on_the_fixture_matrices(host_check):
    mats = [mo.dist_matrix(*match_mesh(b)[:2]) for b in range(len(SHAPES) - 1)]
    mats += [mo.dist_matrix(SKEL[f"pos_a{i}"], SKEL[f"pos_b{i}"]) for i in SKEL_META["eval_meshes"]]
    check_against_scipy(mats, host_check(mats), lambda k: True)
    tie = mo.dist_matrix(MATCH["tie_pred"], MATCH["tie_gt"])
    (status, row, col), = host_check([tie])
    assert status == 0 and tie[row, col].sum() == MATCH_META["tie_total"] and len(set(col.tolist())) == len(col) == 6


def test_host_program_on_seeded_random_matrices(host_check):
    """3000 matrices up to 128 x 256 in both orientations: uniform costs (compared by assignment where the gap condition holds, which the
    first 300 are checked for; by total cost otherwise) and, every tenth, small integers (many optima: total cost)"""
    rng = np.random.default_rng(20261018)
    mats = []
    for k in range(3000):
        small = int(rng.integers(1, 129))
        large = int(rng.integers(small, 257))
        shape = (small, large) if k % 2 else (large, small)
        if k < 8:
            shape = [(128, 256), (256, 128), (128, 128), (1, 256), (256, 1), (1, 1), (64, 65), (65, 64)][k]
        mats.append(rng.integers(0, 4, shape).astype(np.float64) if k % 10 == 9 else rng.random(shape))
    unique = {k for k in range(300) if k % 10 != 9 and min(mats[k].shape) <= 40 and mo.assignment_gap(mats[k]) > GAP}
    assert len(unique) > 30
    check_against_scipy(mats, host_check(mats), lambda k: k in unique)


def test_host_program_refuses_what_the_kernel_refuses(host_check):
    res = host_check([np.zeros((129, 130)), np.zeros((2, 257)), np.zeros((257, 2)), np.zeros((0, 4)), np.zeros((3, 0)),
                      np.full((2, 3), np.nan), np.array([[np.inf, 1.0], [np.inf, 2.0]])])
    assert [r[0] for r in res] == [1, 1, 1, 0, 0, 4, 4] and all(len(r[1]) == 0 for r in res)


# ------------------------------------------------------------------------------------------------------------ the Python glue
@pytest.fixture()
def ops(monkeypatch):
    o = metrics_emulate.MetricOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


def batch_inputs():
    n = len(SHAPES)
    return MATCH["pred"], MATCH["pred_ptr"], [chain_rig(match_mesh(b)[1]) for b in range(n)], [match_mesh(b)[2] for b in range(n)]


def test_sample_skel_ptrs_and_the_one_host_read(ops):
    rigs = [r for i in range(3) for r in skel_rigs(i)]
    samples, ptr = metrics.sample_skel(rigs)
    want = [SKEL[f"samples_{t}{i}"] for i in range(3) for t in "ab"]
    assert ptr.dtype == torch.int32 and ptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np.array_equal(samples.numpy(), np.concatenate(want)) and ops.calls == ["bone_sample_counts", "bone_samples"]
    assert np.array_equal(metrics.rig_bones(rigs[0]), np.array(mo.bones_of(rigs[0])))


def test_a_rig_without_bones_raises_value_error(ops):
    with pytest.raises(ValueError, match="rig 1 has no bones"):
        metrics.sample_skel([skel_rigs(1)[0], chain_rig(np.zeros((1, 3)))])
    with pytest.raises(ValueError, match="no bones"):
        metrics.chamfer_b2b([chain_rig(np.zeros((1, 3)))], [skel_rigs(1)[0]])
    assert ops.calls == []


def test_bone_chamfers_sample_both_lists_in_one_call(ops):
    pairs = [skel_rigs(i) for i in range(4)]
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    j2b, b2b = metrics.chamfer_j2b(a, b), metrics.chamfer_b2b(a, b)
    assert ops.calls.count("bone_sample_counts") == 2                                            # one per public call
    assert np.abs(j2b.numpy() - SKEL["chamfer_j2b"][:4]).max() <= SUM_TOL and np.abs(b2b.numpy() - SKEL["chamfer_b2b"][:4]).max() <= SUM_TOL


def test_ptrs_are_host_metadata_and_are_checked(ops):
    pred, pp, gt, gp = MATCH["pred"], MATCH["pred_ptr"], MATCH["gt"], MATCH["gt_ptr"]
    for bad in (pp[1:], pp[::-1].copy(), np.append(pp[:-1], pp[-1] + 1), pp.astype(np.float64), pp[:1]):
        with pytest.raises(ValueError):
            metrics.match_joints(pred, bad, gt, gp)
    with pytest.raises(ValueError, match="same meshes"):
        metrics.chamfer_j2j(pred, pp, gt, np.array([0, len(gt)]))
    d = metrics.nearest_distance(gt, gp.tolist(), pred, torch.from_numpy(pp), squared=True)      # list, CPU tensor
    want = np.concatenate([mo.nearest_sq(match_mesh(b)[1], match_mesh(b)[0]) for b in range(len(SHAPES) - 1)])
    assert np.array_equal(d.numpy()[:len(want)], want) and np.isnan(d.numpy()[len(want):]).all()
    _, flags = metrics.nearest_distance(gt, gp, pred, pp, return_flags=True)
    assert flags.tolist() == [0] * 9 + [1]                                                       # the mesh without predictions: a flag, no number


def test_match_joints_layout(ops):
    m = metrics.match_joints(MATCH["pred"], MATCH["pred_ptr"], MATCH["gt"], MATCH["gt_ptr"])
    assert np.array_equal(m["match_ptr_host"], MATCH["match_ptr"]) and m["match_ptr"].tolist() == MATCH["match_ptr"].tolist()
    assert np.array_equal(m["row_ind"].numpy(), MATCH["row_ind"]) and np.array_equal(m["col_ind"].numpy(), MATCH["col_ind"])
    assert np.array_equal(m["dist"].numpy(), MATCH["dist"]) and m["status"].tolist() == [0] * len(SHAPES)
    sc = metrics.joint_scores(m, m["n_pred"], m["n_gt"], MATCH["fs"], MATCH["gt_ptr"])
    assert sc["hits"].tolist() == MATCH["hits"].tolist() and np.array_equal(sc["iou"].numpy()[:-1], MATCH["iou"][:-1])
    with pytest.raises(ValueError, match="one feature size per ground-truth joint"):
        metrics.joint_scores(m, m["n_pred"], m["n_gt"], MATCH["fs"][:-1], np.append(MATCH["gt_ptr"][:-1], MATCH["gt_ptr"][-1] - 1))


def test_size_refusal_names_the_mesh_and_keeps_the_others(ops):
    rng = np.random.default_rng(5)
    sizes = [(7, 7), (129, 130), (5, 3), (2, 257), (128, 256)]                                  # (n_gt, n_pred): the last one is the limit itself
    gt, pred = [rng.random((g, 3)) for g, _ in sizes], [rng.random((p, 3)) for _, p in sizes]
    ptr = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    with pytest.raises(metrics.AssignmentSizeError) as e:
        metrics.match_joints(np.concatenate(pred), ptr(pred), np.concatenate(gt), ptr(gt))
    assert e.value.meshes == [1, 3] and e.value.sizes == [(129, 130), (2, 257)] and "[1, 3]" in str(e.value)
    res = e.value.result
    assert res["status"].tolist() == [0, 1, 0, 1, 0]
    for b in (0, 2, 4):
        m0, m1 = res["match_ptr_host"][b], res["match_ptr_host"][b + 1]
        row, col, _ = mo.match(pred[b], gt[b])
        assert np.array_equal(res["row_ind"].numpy()[m0:m1], row) and np.array_equal(res["col_ind"].numpy()[m0:m1], col)
    m0, m1 = res["match_ptr_host"][1], res["match_ptr_host"][2]
    assert m1 - m0 == 129 and (res["row_ind"].numpy()[m0:m1] == -1).all() and np.isnan(res["dist"].numpy()[m0:m1]).all()


def test_evaluate_rigs_bookkeeping_and_report(ops):
    pred, pp, gt_rigs, fss = batch_inputs()
    res = metrics.evaluate_rigs(pred, pp, gt_rigs, fss)
    want = mo.evaluate([match_mesh(b)[0] for b in range(len(SHAPES))], gt_rigs, fss)
    assert res["num_invalid"] == 1 and res["valid"].tolist() == [True] * 9 + [False]
    for k in ("iou", "precision", "recall"):
        assert np.array_equal(res[k].numpy(), want[k], equal_nan=True) and float(res["mean"][k]) == want["mean"][k]
    assert np.abs(res["chamfer_j2j"].numpy()[:-1] - MATCH["chamfer_j2j"][:-1]).max() <= SUM_TOL and np.isnan(res["chamfer_j2j"].numpy()[-1])
    assert res["hits"].tolist() == MATCH["hits"].tolist() and "chamfer_j2b" not in res
    assert metrics.format_report(res) == MATCH_META["report"] == mo.format_report(want)
    flat = metrics.evaluate_rigs(torch.from_numpy(pred), pp.tolist(), gt_rigs, MATCH["fs"])      # feature sizes concatenated
    assert np.array_equal(flat["iou"].numpy(), res["iou"].numpy(), equal_nan=True)
    with pytest.raises(ValueError):
        metrics.evaluate_rigs(pred, pp, gt_rigs[:-1], fss[:-1])
    with pytest.raises(ValueError, match="one feature size per ground-truth joint"):
        metrics.evaluate_rigs(pred, pp, gt_rigs, fss[:-1] + [fss[-1][:-1]])


def test_evaluate_rigs_with_predicted_rigs(ops):
    preds, pred_rigs, gt_rigs, fss = skel_eval_inputs()
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in preds])])
    res = metrics.evaluate_rigs(np.concatenate(preds), ptr, gt_rigs, fss, pred_rigs=pred_rigs)
    assert ops.calls.count("bone_sample_counts") == 1 and res["num_invalid"] == 1 and res["valid"].tolist() == [True] * 5 + [False]
    idx = SKEL_META["eval_meshes"]
    assert np.abs(res["chamfer_j2b"].numpy()[:-1] - SKEL["chamfer_j2b"][idx]).max() <= SUM_TOL and np.isnan(res["chamfer_j2b"].numpy()[-1])
    assert np.abs(res["chamfer_b2b"].numpy()[:-1] - SKEL["chamfer_b2b"][idx]).max() <= SUM_TOL and np.isnan(res["chamfer_b2b"].numpy()[-1])
    keys = ("chamfer_j2j", "iou", "precision", "recall", "chamfer_j2b", "chamfer_b2b")
    assert all(abs(float(res["mean"][k]) - SKEL["eval_means"][j]) <= SUM_TOL for j, k in enumerate(keys))
    assert res["hits"].tolist() == SKEL["eval_hits"].tolist() + [0] and metrics.format_report(res) == SKEL_META["report"]
    all_invalid = metrics.evaluate_rigs(np.zeros((0, 3)), [0, 0], gt_rigs[:1], fss[:1], pred_rigs=[None])
    assert all_invalid["num_invalid"] == 1 and np.isnan(float(all_invalid["mean"]["iou"])) and np.isnan(all_invalid["chamfer_b2b"].numpy()).all()
