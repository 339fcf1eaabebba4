"""csrc/metrics.hip and csrc/assign_core.h on the device at the sizes their kernels branch on: the generated cases of
tests/metrics_cases.py (conditions asserted on the CPU by tests/test_metrics_cases.py) through the public functions of
morig_amd/metrics.py, and through ``get_ops()`` / the C entry point where a table is hand-made. The compare functions are the shared
ones; the bars are those of the module docstring of metrics_cases: bit equality for everything discrete, bone samples, squared nearest
distances, the restated means and the score ratios; 1 ulp for a square root; SUM_TOL against the oracle's pairwise np.mean. Figures are
printed before they are asserted (run with -s). Every device result is computed once and shared."""
import numpy as np
import pytest
import torch

import metrics_cases as mc
import metrics_oracle as mo
from morig_amd import metrics
from morig_amd.native import _p, _stream, check
from morig_amd.runtime import get_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def matched():
    """the 20 matching cases as two batches -> per case (row, col, dist), all status words"""
    def run():
        cases = mc.assign_cases()
        a, sa = mc.run_match(cases[:10], DEV)
        b, sb = mc.run_match(cases[10:], DEV)
        return a + b, np.concatenate([sa, sb])
    return cached("matched", run)


# ------------------------------------------------------------------------------------------------------------------------- matching
@pytest.mark.parametrize("k", range(len(mc.LANE_SHAPES) + len(mc.LDS_SHAPES)), ids=lambda k: "%dx%d" % (mc.LANE_SHAPES + mc.LDS_SHAPES)[k])
def test_matching_equals_scipys_pair_for_pair(k):
    """1 to 4 columns per lane in both orientations; the cost matrix on either side of AS_LDS_COST"""
    c = mc.assign_cases()[k]
    per, status = matched()
    assert status[k] == 0
    off = mc.check_matching(per[k], (c["row"], c["col"], c["dist"]), c["name"])
    print(f"{c['name']}: {c['cols_per_lane']} columns per lane, {'LDS' if c['in_lds'] else 'global'} cost, matched distances within {off} ulp")


def test_a_second_run_and_a_mesh_alone_give_the_batch_bits():
    cases = mc.assign_cases()
    per, _ = matched()
    again, _ = mc.run_match(cases[10:], DEV)
    assert all(mc.same_bits(x, y) for g, w in zip(again, per[10:]) for x, y in zip(g, w))
    for k in (7, 12, 13, 18):                                                                # 193 x 17, 128 x 256, 256 x 128, 79 x 79
        (alone,), _ = mc.run_match([cases[k]], DEV)
        assert all(mc.same_bits(x, y) for x, y in zip(alone, per[k])), cases[k]["name"]


def test_tie_cases_reach_the_optimal_total_exactly():
    for c in mc.tie_cases():
        (got,), status = mc.run_match([c], DEV)
        assert status.tolist() == [0]
        mc.check_valid_matching(got, c["d"], c["total"], c["name"])


def test_degenerate_sides():
    batch = mc.degenerate_batch()
    per, status = mc.run_match(batch, DEV)
    assert status.tolist() == [0] * len(batch)
    for m, got in zip(batch, per):
        if m["n_pred"] == 0:
            assert all(len(x) == 0 for x in got)
            continue
        mc.check_matching(got, mo.match(m["pred"], m["gt"]), "degenerate")
        (alone,), _ = mc.run_match([m], DEV)
        assert all(mc.same_bits(x, y) for x, y in zip(alone, got))


def test_non_finite_joints_follow_the_rule():
    """a NaN or infinite column is never chosen; status 0 when the others suffice, MORIG_ASSIGN_ST_INFEASIBLE with -1 / NaN pairs and 0
    hits when they do not; the healthy mesh of the batch is untouched"""
    batch = mc.nonfinite_batch()
    per, status, sc = mc.run_match(batch, DEV, fs=[m["fs"] for m in batch])
    print("status", status.tolist(), "hits", sc["hits"].tolist())
    assert status.tolist() == [m["want"][0] for m in batch] == [0, 4, 0, 4, 0]
    assert get_ops().ASSIGN_ST_INFEASIBLE == mc.ST_INFEASIBLE and get_ops().ASSIGN_ST_PTR == mc.ST_PTR
    for m, got in zip(batch, per):
        mc.check_matching(got, m["want"][1:], m["name"])
    mc.check_hits(sc["hits"], [5, 0, 5, 0, 5], "non-finite")
    mc.check_bits(sc["iou"], np.array([10 / 11, 0.0, 10 / 11, 0.0, 10 / 11]), "iou")
    (alone,), _ = mc.run_match([batch[4]], DEV)
    assert all(mc.same_bits(x, y) for x, y in zip(alone, per[4]))


def raw_assign(pred, pred_ptr, gt, gt_ptr, match_ptr, n_match, cost_off, n_cost, out):
    """morig_assign_joints itself, writing into the caller's (prefilled) outputs"""
    row, col, dist, status = out
    cost = torch.empty(n_cost, dtype=torch.float64, device=pred.device)
    check(get_ops().lib.morig_assign_joints(_p(pred), _p(pred_ptr), pred.shape[0], _p(gt), _p(gt_ptr), gt.shape[0], status.numel(), _p(match_ptr),
                                            n_match, _p(cost), _p(cost_off), n_cost, _p(row), _p(col), _p(dist), _p(status), _stream()),
          "morig_assign_joints")
    torch.cuda.synchronize()


def test_bad_tables_give_their_status_and_leave_the_others_alone():
    """Every damaged table is caught by assign_kernel's uniform check (csrc/metrics.hip, before anything of the mesh is addressed:
    ST_PTR, nothing written) or by `c1 - c0 < entries` (ST_SIZE, -1 / NaN written inside the mesh's own match segment)."""
    meshes, clean, variants = mc.table_batch()
    clean_out = mc.run_assign_tables(raw_assign, meshes, clean, DEV)
    assert clean_out[3].tolist() == [0, 0, 0, 0]
    for b, m in enumerate(meshes):
        seg = slice(clean["match_ptr"][b], clean["match_ptr"][b + 1])
        mc.check_matching(tuple(x[seg] for x in clean_out[:3]), mo.match(m["pred"], m["gt"]), "clean tables")
    for name, bad, status, tables in variants:
        got = mc.run_assign_tables(raw_assign, meshes, tables, DEV)
        print(name, "status", got[3].tolist())
        mc.check_assign_tables(clean_out, got, bad, status, name)


# ------------------------------------------------------------------------------------------------------------------------ threshold
def test_hits_are_counted_only_above_the_distance():
    batch = mc.threshold_batch()
    per, status, sc = mc.run_match(batch, DEV, fs=[c["fs"] for c in batch])
    assert status.tolist() == [0, 0, 0]
    for c, got in zip(batch, per):
        off = mc.check_matching(got, (c["want"]["row"], c["want"]["col"], c["want"]["dist"]), c["name"])
        assert off == 0                                                                          # square roots of perfect squares
    print("hits", sc["hits"].tolist(), "of", [c["n_gt"] for c in batch])
    mc.check_hits(sc["hits"], [c["want"]["hits"] for c in batch], "threshold")
    for k in mc.RATIOS:
        mc.check_bits(sc[k], np.array([c["want"][k] for c in batch]), k)
    h = mc.threshold_handmade()
    hits, ratios = mc.run_handmade_scores(h, DEV)
    print("hand-made pairs: hits", hits.tolist(), "of", h["sizes"])
    mc.check_hits(hits, h["hits"], "hand-made pairs")
    mc.check_bits(ratios, h["ratios"], "hand-made ratios")


# -------------------------------------------------------------------------------------------------------------------------- nearest
def test_nearest_at_the_tile_and_workgroup_sizes():
    c = mc.nearest_tiles()
    sq, d, flags = mc.run_nearest(get_ops(), mc.cat(c["a"]), mc.ptr(c["a"]), mc.cat(c["b"]), mc.ptr(c["b"]), DEV)
    off = mc.check_nearest(sq, d, np.concatenate(c["sq"]), "tiles")
    print(f"nearest tiles: sqrt within {off} ulp of numpy's")
    assert flags.tolist() == [0] * 6
    means = mc.run_segment_mean(get_ops(), d, mc.ptr(c["a"]), DEV)
    print("one-way means |device - oracle| max", mc.check_sum(means, c["oneway"], "one-way means"))
    pub = metrics.nearest_distance(mc.cat(c["a"]), mc.ptr(c["a"]), mc.cat(c["b"]), mc.ptr(c["b"]), squared=True, device=DEV)
    mc.check_bits(mc.host(pub), sq, "the public function")


def test_nearest_walks_the_meshes_of_a_workgroup():
    c = mc.nearest_walk()
    sq, d, flags = mc.run_nearest(get_ops(), c["a"], c["a_ptr"], c["b"], c["b_ptr"], DEV)
    print("flags", flags.tolist(), "NaN rows", int(np.isnan(sq).sum()))
    mc.check_nearest(sq, d, c["want"], "mesh walk")
    assert flags.tolist() == c["flags"]
    again, _, _ = mc.run_nearest(get_ops(), c["a"], c["a_ptr"], c["b"], c["b_ptr"], DEV)
    mc.check_bits(again, sq, "second run")


def test_nearest_gives_nan_where_np_min_does():
    """a NaN source row gives NaN; a NaN row of b (in the second LDS tile) gives NaN to every source of its mesh; squared and rooted"""
    c = mc.nearest_nan()
    pa = mc.ptr(c["a"])
    sq, d, flags = mc.run_nearest(get_ops(), mc.cat(c["a"]), pa, mc.cat(c["b"]), mc.ptr(c["b"]), DEV)
    print("NaN rows", np.flatnonzero(np.isnan(sq))[:5].tolist(), "...", int(np.isnan(sq).sum()), "of", len(sq))
    mc.check_nearest(sq, d, c["sq"], "NaN")
    assert flags.tolist() == [0, 0, 0]
    j2j = mc.host(metrics.chamfer_j2j(mc.cat(c["a"]), pa, mc.cat(c["b"]), mc.ptr(c["b"]), device=DEV))
    assert np.isnan(j2j[:2]).all() and abs(j2j[2] - mo.chamfer(c["a"][2], c["b"][2])) <= mc.SUM_TOL


# ---------------------------------------------------------------------------------------------------------------------------- means
def test_segment_mean_has_the_restated_order_bit_for_bit():
    c = mc.mean_case()
    got = mc.run_segment_mean(get_ops(), c["x"], c["ptr"], DEV)
    print("segment mean |device - fsum| max", mc.check_sum(got, c["fsum"], "segment mean against fsum"))
    mc.check_bits(got, c["order"], "segment mean against the kernel's order")
    bad = c["ptr"].copy()
    bad[4] = bad[5] + 1                                                                        # segment 4 descends: `e < s`, no element is read
    got_bad = mc.run_segment_mean(get_ops(), c["x"], bad, DEV)
    assert np.isnan(got_bad[4]) and mc.same_bits(got_bad[[1, 2, 5, 6, 7]], got[[1, 2, 5, 6, 7]])


def test_valid_mean_is_the_sequential_sum():
    for c in mc.valid_mean_cases():
        mc.check_bits(mc.run_valid_mean(get_ops(), c, DEV), c["want"], c["name"])


# ---------------------------------------------------------------------------------------------------------------------------- bones
@pytest.mark.parametrize("k", range(3), ids=["255", "256", "257"])
def test_bone_samples_across_the_workgroup_size(k):
    c = mc.bone_batches()[k]
    samples, p = metrics.sample_skel(c["rigs"], device=DEV)
    assert mc.host(p).tolist() == mc.ptr(c["samples"]).tolist()
    mc.check_bits(mc.host(samples), np.concatenate(c["samples"]), f"bones {c['n_bones']}")
    counts, _ = mc.run_bone_ops(get_ops(), mc.cat([r.pos for r in c["rigs"]]), metrics._pack_rigs(c["rigs"], "cpu")[2].numpy(), DEV)
    mc.check_bits(counts, c["counts"], "counts")


def test_refused_bones_count_zero_and_sample_skel_raises():
    c = mc.refused_bones()
    counts, samples = mc.run_bone_ops(get_ops(), c["pos"], c["bones"], DEV)
    print("counts", counts.tolist())
    mc.check_bits(counts, c["counts"], "refused bones: counts")
    mc.check_bits(samples, c["samples"], "refused bones: the neighbours' samples")
    healthy = mc.bone_batches()[0]["rigs"][0]
    pos = healthy.pos.copy()
    pos[4, 0] = np.nan
    with pytest.raises(ValueError, match=r"bone 3 of rig 1 .*2 such bone"):
        metrics.sample_skel([healthy, mc.chain_rig(pos)], device=DEV)
    far = healthy.pos.copy()
    far[-1] += 1e6
    with pytest.raises(ValueError, match=rf"bone {len(far) - 2} of rig 0"):
        metrics.chamfer_b2b([mc.chain_rig(far)], [healthy], device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------- whole
def whole(with_rigs):
    return cached(("whole", with_rigs), lambda: mc.run_whole(mc.whole_batch(), DEV, with_rigs))


@pytest.mark.parametrize("with_rigs", [False, True])
def test_evaluate_rigs_on_the_mixed_batch(with_rigs):
    c = mc.whole_batch()
    got = whole(with_rigs)
    worst = mc.check_whole(got, c["want"] if with_rigs else c["want_plain"], "whole batch")
    print(f"evaluate_rigs(pred_rigs={with_rigs}): chamfers within {worst:.2e} of the oracle (bound {mc.SUM_TOL}); report\n{got['report']}")
    assert got["status"].tolist() == [0] * 6
    again = mc.run_whole(c, DEV, with_rigs)
    for k in mc.RATIOS + mc.CHAMFERS + ("hits", "row", "col"):
        if k in got:
            mc.check_bits(again[k], got[k], f"second run: {k}")
    assert all(mc.same_bits(again["mean"][k], got["mean"][k]) for k in got["mean"])


def test_every_mesh_alone_gives_its_batch_bits():
    c = mc.whole_batch()
    got = whole(True)
    for b in range(len(c["preds"])):
        if len(c["preds"][b]) == 0:
            continue
        one = mc.run_whole(c, DEV, True, only=b)
        for k in mc.RATIOS + mc.CHAMFERS + ("hits",):
            mc.check_bits(one[k][0], got[k][b], f"mesh {b} alone: {k}")
