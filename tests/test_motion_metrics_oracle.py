"""CPU: tests/motion_metrics_oracle.py against the reference's own statements recorded in tests/golden/motion_metrics.npz
(tools/make_motion_metrics_golden.py): every count exactly, every ratio to the last bit; the float64 key-frame flow error against the
reference's float32 one; and the two comparison rules a hand-rolled numpy loop gets wrong, pinned on explicit values.

FLOW_F32_DEVIATION: the largest relative difference between the oracle's float64 per-frame error and the reference's float32 statement
(eval_deform.py:18: float32 squares, float32 pairwise mean) on the fixture, measured here on the CPU: 1.221e-7, one float32 ulp of the
result. The test asserts 4 x that."""
import numpy as np
import pytest

import motion_metrics_oracle as mo
from conftest import load_golden

META, G = load_golden("motion_metrics")
G = {k: v.numpy() for k, v in G.items()}
FLOW_F32_DEVIATION = 1.221e-7


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def corr_pairs():
    return [(G[f"corr_pts{b}"], G[f"corr_nnind{b}"], G[f"corr_rows{b}"]) for b in range(len(META["corr_pairs"]))]


def attn_meshes():
    return [(G[f"attn_pred{b}"], G[f"attn_gt{b}"]) for b in range(len(META["attn_meshes"]))]


def flow_meshes():
    return [(G[f"flow_pred{b}"], G[f"flow_gt{b}"]) for b in range(len(META["flow_meshes"]))]


def test_the_lists_are_the_references():
    assert same(G["tolerances"], np.array(mo.TOLERANCES)) and same(G["thresholds"], mo.THRESHOLDS)
    assert mo.THRESHOLDS[3] == 0.30000000000000004 and len(mo.THRESHOLDS) == 10


def test_corr_accuracy_equals_the_reference_statements():
    res = mo.corr_accuracy(corr_pairs())
    for b, (n_pts, n_vtx, n_corr) in enumerate(META["corr_pairs"]):
        assert res["count"][b] == n_corr and same(res["hits"][b], G[f"corr_hits{b}"])
        assert same(res["acc"][b], G[f"corr_acc{b}"]) or (n_corr == 0 and np.isnan(res["acc"][b]).all() and np.isnan(G[f"corr_acc{b}"]).all())
    assert res["n_valid"] == 4 and np.isnan(res["acc"][4]).all()                     # the pair without correspondences
    total = np.zeros(10)
    for b in range(4):
        total += G[f"corr_acc{b}"]
    assert same(res["curve"], total / 4) and (res["hits"][1] > 0).all() and (res["hits"][1] < 257).all()          # hits and misses at every tolerance


def test_corr_distances_keep_clear_of_the_tolerances():
    for pts, nnind, corr in corr_pairs():
        if len(corr):
            d = mo.corr_distance(pts, nnind, corr).astype(np.float64)
            assert np.abs(d[:, None] - np.array(mo.TOLERANCES)[None]).min() > META["margin"]


def test_pr_curve_equals_the_reference_statements():
    res = mo.pr_curve(attn_meshes())
    for b in range(len(META["attn_meshes"])):
        assert same(res["tp"][b], G[f"attn_tp{b}"]) and same(res["pp"][b], G[f"attn_pp{b}"]) and res["gp"][b] == G[f"attn_gp{b}"]
        assert same(res["precision"][b], G[f"attn_precision{b}"]) and same(res["recall"][b], G[f"attn_recall{b}"])
    mp, mr = np.zeros(10), np.zeros(10)
    for b in range(len(META["attn_meshes"])):
        mp += G[f"attn_precision{b}"]
        mr += G[f"attn_recall{b}"]
    assert same(res["mean_precision"], mp / 4) and same(res["mean_recall"], mr / 4)
    assert res["pp"][3, 0] == 1024 and res["pp"][3, 9] < 200 and res["tp"].max() > 100          # the minimum alone is not above 0


def test_attention_fixture_keeps_clear_of_the_inexact_thresholds():
    """the condition under which numpy 2's float64 comparison (the generating numpy) and the reference's float32 comparison agree"""
    thr = mo.THRESHOLDS
    inexact = thr[thr.astype(np.float32).astype(np.float64) != thr]
    assert len(inexact) == 8                                                         # all but 0.0 and 0.5
    for pred, _ in attn_meshes():
        x = mo.normalised(pred).astype(np.float64)
        assert np.abs(x[:, None] - inexact[None]).min() > META["margin"]


def test_flow_error_float64_against_the_reference_float32():
    per_frame, per_mesh = mo.keyframe_flow_errors(flow_meshes())
    worst = 0.0
    for b in range(len(META["flow_meshes"])):
        ref = G[f"flow_ref{b}"]
        assert ref.dtype == np.float32 and ref.shape == (META["keyframes"],)
        worst = max(worst, float((np.abs(per_frame[b] - ref.astype(np.float64)) / ref.astype(np.float64)).max()))
    print(f"float64 flow error against the reference's float32: largest relative difference {worst:.3e}")
    assert worst <= 4 * FLOW_F32_DEVIATION
    assert same(per_mesh, (((per_frame[:, 0] + per_frame[:, 1]) + per_frame[:, 2]) + per_frame[:, 3] + per_frame[:, 4]) / 5.0)


@pytest.mark.parametrize("t", [0.1, 0.3, 0.30000000000000004])
def test_the_promotion_trap_is_pinned(t):
    """a value equal to float32(t) is NOT above the threshold t: the comparison is float32, as under the reference's numpy 1.21; a float64
    comparison (numpy 2 with an np.float64 scalar from np.arange) would count it whenever float32(t) > t"""
    pred = np.array([0.0, np.float32(t), 1.0], dtype=np.float32)                     # normalising leaves the three as they are
    assert same(mo.normalised(pred), pred)
    tp, pp, gp = mo.pr_counts(pred, np.array([1, 1, 1]), thresholds=[t])
    assert pp.tolist() == [1] and tp.tolist() == [1] and gp == 3                       # only the 1.0
    if np.float64(np.float32(t)) > t:
        assert int((pred.astype(np.float64) > np.float64(t)).sum()) == 2               # what the float64 comparison would count


def test_a_distance_equal_to_the_tolerance_is_no_hit():
    t = np.float32(0.02)
    pts = np.array([[0, 0, 0], [0, t, 0], [0, np.nextafter(t, np.float32(0)), 0]], dtype=np.float32)
    assert mo.corr_distance(pts, [0], np.array([[0, 1]]))[0] == t
    assert mo.corr_hits(pts, [0], [[0, 1]], [0.02, 0.04]).tolist() == [0, 1]
    assert mo.corr_hits(pts, [0], [[0, 2]], [0.02, 0.04]).tolist() == [1, 1]           # one ulp below it is
