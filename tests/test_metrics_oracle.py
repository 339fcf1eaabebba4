"""tests/metrics_oracle.py (float64 numpy + scipy) against the reference's recorded results (tests/golden/metrics_match.npz,
metrics_skel.npz; tools/make_metrics_golden.py): bone samples bit for bit, chamfers within the summation bound, the matching exact; the
conditions the fixtures were generated under; the C ABI of the new entry points.

SUM_TOL: a mean of n <= 4096 float64 terms, each below 4, moves by at most about n * 2^-53 * 4 = 1.8e-12 when the order of the sum
changes; every chamfer is a half-sum of two such means. 1e-11 absolute covers it (the tests assert n and the magnitudes)."""
import types

import numpy as np

import metrics_oracle as mo
from morig_amd import formats
from test_loss_oracle import load

SUM_TOL, MAX_TERMS, MAX_TERM = 1e-11, 4096, 4.0
GAP, MARGIN = 1e-6, 1e-9
MATCH_META, MATCH = load("metrics_match")
SKEL_META, SKEL = load("metrics_skel")
SHAPES = [tuple(s) for s in MATCH_META["shapes"]]
N_SKEL = SKEL_META["n"]


def chain_rig(pos):
    """a stand-in with the three members the metrics read (pos, hierarchy, root_id): the joints exactly as given, in a chain"""
    return types.SimpleNamespace(pos=np.asarray(pos, dtype=np.float64), hierarchy=np.arange(-1, len(pos) - 1), root_id=0)


def match_mesh(b):
    """-> (pred, gt, fs) of mesh b of the matching batch"""
    g0, g1, p0, p1 = MATCH["gt_ptr"][b], MATCH["gt_ptr"][b + 1], MATCH["pred_ptr"][b], MATCH["pred_ptr"][b + 1]
    return MATCH["pred"][p0:p1], MATCH["gt"][g0:g1], MATCH["fs"][g0:g1]


def skel_rigs(i):
    """-> (rig a, rig b) of pair i as formats.Rig"""
    return tuple(formats.Rig.from_arrays(SKEL[f"pos_{t}{i}"], SKEL[f"hier_{t}{i}"], 0) for t in "ab")


def skel_eval_inputs():
    """the evaluation batch of the skeleton fixture: the EVAL meshes with rig a as the prediction, then one mesh without predicted joints
    -> (preds, pred_rigs, gt_rigs, fss)"""
    preds, pred_rigs, gt_rigs, fss = [], [], [], []
    for i in SKEL_META["eval_meshes"]:
        a, b = skel_rigs(i)
        preds.append(a.pos), pred_rigs.append(a), gt_rigs.append(b), fss.append(SKEL[f"fs{i}"])
    i = SKEL_META["eval_meshes"][0]
    preds.append(np.zeros((0, 3))), pred_rigs.append(None), gt_rigs.append(skel_rigs(i)[1]), fss.append(SKEL[f"fs{i}"])
    return preds, pred_rigs, gt_rigs, fss


def test_shapes_and_sizes_of_the_fixtures():
    assert SHAPES == [(1, 1), (1, 5), (5, 1), (7, 7), (24, 31), (33, 20), (64, 65), (65, 64), (96, 96), (12, 0)]
    assert np.array_equal(np.diff(MATCH["gt_ptr"]), [s[0] for s in SHAPES]) and np.array_equal(np.diff(MATCH["pred_ptr"]), [s[1] for s in SHAPES])
    assert np.array_equal(np.diff(MATCH["match_ptr"]), [min(s) for s in SHAPES]) and MATCH_META["num_invalid"] == 1
    counts = np.array(SKEL_META["counts"])
    assert counts.max() > 1024 and counts.min() < 16 and counts.max() <= MAX_TERMS              # past one tile of nearest_distance; a handful
    assert MATCH["gt"].max() < MAX_TERM ** 0.5 / 2 and all(np.abs(SKEL[f"pos_{t}{i}"]).max() <= 1.0 for t in "ab" for i in range(N_SKEL))


def test_bone_samples_equal_the_reference_bit_for_bit():
    for i in range(N_SKEL):
        for t, rig in zip("ab", skel_rigs(i)):
            assert np.array_equal(rig.pos, SKEL[f"pos_{t}{i}"])                                  # Rig's forward pass leaves these joints alone
            got, want = mo.sample_skel(rig), SKEL[f"samples_{t}{i}"]
            assert got.shape == want.shape and np.array_equal(got, want), (i, t)


def test_half_step_bones_round_to_even():
    star = skel_rigs(0)[0]
    lengths = np.abs(star.pos[1:]).max(axis=1)
    steps = lengths / mo.STEP
    assert list(steps[:6]) == [1.5, 2.5, 4.5, 5.5, 6.5, 7.5] and steps[6] != 3.5 and abs(steps[6] - 3.5) < 1e-12 and steps[7] == 0.0
    counts = [len(mo.sample_bone(star.pos[p], star.pos[c])) for p, c in mo.bones_of(star)]
    assert counts == [3, 3, 5, 7, 7, 9, int(np.round(steps[6])) + 1, 1]                          # 1.5 -> 2, 2.5 -> 2, 4.5 -> 4, 5.5 -> 6, ...
    assert sum(counts) == SKEL_META["counts"][0][0]


def test_chamfers_equal_the_reference_within_the_summation_bound():
    for i in range(N_SKEL):
        a, b = skel_rigs(i)
        assert abs(mo.chamfer_j2b(a, b) - SKEL["chamfer_j2b"][i]) <= SUM_TOL
        assert abs(mo.chamfer_b2b(a, b) - SKEL["chamfer_b2b"][i]) <= SUM_TOL
        assert abs(mo.chamfer(a.pos, b.pos) - SKEL["chamfer_j2j"][i]) <= SUM_TOL
    for b in range(len(SHAPES) - 1):
        pred, gt, _ = match_mesh(b)
        assert abs(mo.chamfer(pred, gt) - MATCH["chamfer_j2j"][b]) <= SUM_TOL
    assert np.isnan(MATCH["chamfer_j2j"][-1])


def test_matching_and_scores_equal_the_stored_ones():
    for b, (n_gt, n_pred) in enumerate(SHAPES[:-1]):
        pred, gt, fs = match_mesh(b)
        s = mo.scores(pred, gt, fs)
        m0, m1 = MATCH["match_ptr"][b], MATCH["match_ptr"][b + 1]
        assert np.array_equal(s["row"], MATCH["row_ind"][m0:m1]) and np.array_equal(s["col"], MATCH["col_ind"][m0:m1])
        assert np.array_equal(s["dist"], MATCH["dist"][m0:m1]) and (np.diff(s["row"]) > 0).all()
        assert s["hits"] == MATCH["hits"][b] and s["iou"] == MATCH["iou"][b] and s["precision"] == MATCH["precision"][b] and s["recall"] == MATCH["recall"][b]
    assert 0 < MATCH["hits"][:-1].sum() < MATCH["match_ptr"][-1]                                 # both outcomes of the threshold occur


def test_evaluation_means_and_report_equal_the_stored_ones():
    preds = [match_mesh(b)[0] for b in range(len(SHAPES))]
    res = mo.evaluate(preds, [chain_rig(match_mesh(b)[1]) for b in range(len(SHAPES))], [match_mesh(b)[2] for b in range(len(SHAPES))])
    assert res["num_invalid"] == 1 and list(res["valid"]) == [True] * 9 + [False]
    assert abs(res["mean"]["chamfer_j2j"] - MATCH["means"][0]) <= SUM_TOL
    assert [res["mean"][k] for k in ("iou", "precision", "recall")] == list(MATCH["means"][1:])
    assert mo.format_report(res) == MATCH_META["report"] and MATCH_META["report"].count("\n") == 3
    preds, pred_rigs, gt_rigs, fss = skel_eval_inputs()
    res = mo.evaluate(preds, gt_rigs, fss, pred_rigs)
    keys = ("chamfer_j2j", "iou", "precision", "recall", "chamfer_j2b", "chamfer_b2b")
    assert res["num_invalid"] == 1 and all(abs(res["mean"][k] - SKEL["eval_means"][j]) <= SUM_TOL for j, k in enumerate(keys))
    assert np.array_equal(res["hits"][:-1], SKEL["eval_hits"]) and mo.format_report(res) == SKEL_META["report"]


def test_fixture_conditions_hold():
    """a unique optimum (gap > 1e-6 when any matched pair is forbidden) and matched distances clear of their feature sizes (> 1e-9)"""
    cases = [match_mesh(b) for b in range(len(SHAPES) - 1)]
    cases += [(SKEL[f"pos_a{i}"], SKEL[f"pos_b{i}"], SKEL[f"fs{i}"]) for i in SKEL_META["eval_meshes"]]
    for pred, gt, fs in cases:
        d = mo.dist_matrix(pred, gt)
        row, col = mo.linear_sum_assignment(d)
        assert mo.assignment_gap(d) > GAP and mo.threshold_margin(d[row, col], fs[row]) > MARGIN
    stored = [g for g in MATCH_META["gaps"] if g is not None] + SKEL_META["gaps"]
    assert min(stored) > GAP and min([m for m in MATCH_META["margins"] if m is not None] + SKEL_META["margins"]) > MARGIN


def test_tie_case_has_integer_costs_and_many_optima():
    d = mo.dist_matrix(MATCH["tie_pred"], MATCH["tie_gt"])
    assert np.array_equal(d, np.round(d)) and mo.assignment_gap(d) == 0.0
    row, col = mo.linear_sum_assignment(d)
    assert d[row, col].sum() == MATCH_META["tie_total"]


def test_entry_points_are_exported():
    from morig_amd import abi, native
    names = ("morig_bone_sample_counts", "morig_bone_samples", "morig_nearest_distance", "morig_segment_mean", "morig_assign_joints",
             "morig_joint_scores", "morig_valid_mean")
    lib = native.load_library()
    for n in names:
        assert n in native.EXPORTS and hasattr(lib, n)
    assert lib.morig_abi_version() == 3
    assert (abi.CONSTANTS["MORIG_ASSIGN_MAX_SMALL"], abi.CONSTANTS["MORIG_ASSIGN_MAX_LARGE"], abi.CONSTANTS["MORIG_NEAREST_TILE"]) == (128, 256, 1024)
    # refused before anything is read or launched: negative sizes, missing pointers
    assert lib.morig_nearest_distance(None, None, 5, None, None, 0, 1, 0, None, None, None) == -1
    assert lib.morig_assign_joints(None, None, 0, None, None, 0, 2, None, 0, None, None, 0, None, None, None, None, None) == -1
    assert lib.morig_segment_mean(None, None, -1, 1, None, None) == -1
    assert lib.morig_bone_samples(None, 0, None, None, 0, 3, None, None) == -1
    kinds = [lib.morig_prof_name(k).decode() for k in range(64) if lib.morig_prof_name(k)]
    assert "rig_metrics" in kinds
