"""CPU: the generated cases of tests/metrics_cases.py, judged from the oracle alone (tests/metrics_oracle.py) before the device sees them
(tests/test_metrics_differential.py). For every family: the case reaches the branch it is named for, the input conditions hold (the gap
condition for EVERY matching case, none excused), and the packing the device file uses gives the oracle's results when sent through
morig_amd/metrics.py on the emulated operators (tests/metrics_emulate.py). Last, the shared compare functions are shown to reject planted
errors: a swapped pair, one hit more, one ulp in a squared distance, one ulp in a mean."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as mc
import metrics_emulate
import metrics_oracle as mo
from morig_amd import metrics, runtime
from test_metrics_oracle import GAP, SUM_TOL

DEV = "cpu"


@pytest.fixture()
def ops(monkeypatch):
    o = metrics_emulate.MetricOps()
    monkeypatch.setattr(runtime, "_test_ops", o)
    return o


# ------------------------------------------------------------------------------------------------------------------------- matching
def test_every_matching_case_has_a_unique_optimum_and_its_branch():
    cases = mc.assign_cases()
    assert [(c["n_gt"], c["n_pred"]) for c in cases] == mc.LANE_SHAPES + mc.LDS_SHAPES
    gaps = {c["name"]: mo.assignment_gap(c["d"]) for c in cases}
    print("smallest assignment gap", min(gaps.values()), "at", min(gaps, key=gaps.get))
    assert all(g > GAP for g in gaps.values()), gaps                                           # every case, none excused
    lanes = [c for c in cases if c["family"] == "lanes"]
    assert {c["cols_per_lane"] for c in lanes} == {1, 2, 3, 4}
    assert {c["cols_per_lane"] for c in lanes if c["transposed"]} >= {3, 4} and {c["cols_per_lane"] for c in lanes if not c["transposed"]} >= {1, 2, 3, 4}
    assert all(0.0 <= c[k].min() and c[k].max() < 1.0 for c in cases for k in ("gt", "pred"))
    lds = {c["name"]: (c["n_gt"] * c["n_pred"], c["in_lds"]) for c in cases if c["family"] == "lds"}
    assert lds == {"lds_78x78": (6084, True), "lds_64x96": (6144, True), "lds_96x64": (6144, True), "lds_79x79": (6241, False),
                   "lds_49x126": (6174, False)}
    assert all(metrics.MAX_SMALL >= min(c["n_gt"], c["n_pred"]) and metrics.MAX_LARGE >= max(c["n_gt"], c["n_pred"]) for c in cases)


def test_matching_cases_through_the_emulated_ops(ops):
    cases = mc.assign_cases()
    for part in (cases[:10], cases[10:]):                                                     # the two batches of the device file
        per, status = mc.run_match(part, DEV)
        assert status.tolist() == [0] * len(part)
        for c, got in zip(part, per):
            assert mc.check_matching(got, (c["row"], c["col"], c["dist"]), c["name"]) == 0


def test_tie_cases_are_exact_and_have_several_optima(ops):
    for c in mc.tie_cases():
        d = c["d"]
        assert np.array_equal(d, np.round(d)) and np.array_equal(d, c["norm"] * np.abs(c["a"][:, None] - c["b"][None, :]))
        assert len(set(c["a"].tolist())) < len(c["a"]) and mo.assignment_gap(d) == 0.0       # duplicated joints, at least 2 optimal matchings
        row, col = mo.linear_sum_assignment(d)
        swap = [k for k in range(len(row) - 1) if c["a"][row[k]] in c["a"][row[k + 1:]]]
        assert swap and c["total"] == d[row, col].sum() == float(int(c["total"]))
        (got,), status = mc.run_match([c], DEV)
        mc.check_valid_matching(got, d, c["total"], c["name"])
        assert status.tolist() == [0]


def test_degenerate_sides_through_the_emulated_ops(ops):
    batch = mc.degenerate_batch()
    assert [(m["n_gt"], m["n_pred"]) for m in batch][0][1] == 0 and batch[-1]["n_pred"] == 0 and (1, 1) in [(m["n_gt"], m["n_pred"]) for m in batch]
    per, status = mc.run_match(batch, DEV)
    assert status.tolist() == [0] * len(batch)
    for m, got in zip(batch, per):
        if m["n_pred"] == 0:
            assert all(len(x) == 0 for x in got)
        else:
            row, col, dist = mo.match(m["pred"], m["gt"])
            mc.check_matching(got, (row, col, dist), "degenerate")
            (alone,), _ = mc.run_match([m], DEV)
            assert all(mc.same_bits(x, y) for x, y in zip(alone, got))


def test_the_rule_for_non_finite_joints(ops):
    batch = mc.nonfinite_batch()
    by = {m["name"]: m for m in batch}
    for name in ("nan_spare", "inf_spare"):                                                  # the column is not needed: scipy's on the matrix without it
        m = by[name]
        keep = [j for j in range(m["n_pred"]) if j != m["bad"]]
        d = mo.dist_matrix(m["pred"][keep], m["gt"])
        row, col = mo.linear_sum_assignment(d)
        assert mo.assignment_gap(d) > GAP
        st, r, c, dist = m["want"]
        assert st == 0 and np.array_equal(r, row) and np.array_equal(c, np.array(keep)[col]) and mc.same_bits(dist, d[row, col]) and m["bad"] not in c
    for name in ("nan_needed", "nan_gt"):
        st, r, c, dist = by[name]["want"]
        assert st == mc.ST_INFEASIBLE == mo.ST_INFEASIBLE and (r == -1).all() and (c == -1).all() and np.isnan(dist).all() and len(r) == 5
    assert by["healthy"]["want"][0] == 0 and mo.assignment_gap(mo.dist_matrix(by["healthy"]["pred"], by["healthy"]["gt"])) > GAP
    with pytest.raises(ValueError):                                                           # why this is the product's own rule
        mo.match(by["nan_spare"]["pred"], by["nan_spare"]["gt"])
    per, status, sc = mc.run_match(batch, DEV, fs=[m["fs"] for m in batch])
    assert status.tolist() == [0, 4, 0, 4, 0]
    for m, got in zip(batch, per):
        mc.check_matching(got, m["want"][1:], m["name"])
    mc.check_hits(sc["hits"], [5, 0, 5, 0, 5], "non-finite")
    (alone,), _ = mc.run_match([by["healthy"]], DEV)
    assert all(mc.same_bits(x, y) for x, y in zip(alone, per[4]))


def test_bad_tables_on_the_emulated_ops(ops):
    meshes, clean, variants = mc.table_batch()
    clean_out = mc.run_assign_tables(ops.assign_joints, meshes, clean, DEV)
    assert clean_out[3].tolist() == [0, 0, 0, 0] and (clean_out[0] != mc.PREFILL["row"]).all()
    for b, m in enumerate(meshes):
        row, col, dist = mo.match(m["pred"], m["gt"])
        seg = slice(clean["match_ptr"][b], clean["match_ptr"][b + 1])
        mc.check_matching(tuple(x[seg] for x in clean_out[:3]), (row, col, dist), "clean tables")
    assert [v[0] for v in variants] == ["pred_descending", "pred_negative", "pred_past_the_array", "match_wrong_length", "cost_one_short"]
    for name, bad, status, tables in variants:
        assert sum(not np.array_equal(tables[k], clean[k]) for k in clean) == 1                 # one table, one entry
        mc.check_assign_tables(clean_out, mc.run_assign_tables(ops.assign_joints, meshes, tables, DEV), bad, status, name)
    # the conditions the kernel tests, on the numbers: nothing of the damaged mesh is addressable
    pp = variants[0][3]["pred_ptr"]
    assert pp[-1] < pp[-2] and variants[1][3]["pred_ptr"][0] < 0 and variants[2][3]["pred_ptr"][-1] > sum(m["n_pred"] for m in meshes)
    assert np.diff(variants[3][3]["match_ptr"])[-1] != min(meshes[-1]["n_gt"], meshes[-1]["n_pred"])
    assert np.diff(variants[4][3]["cost_off"])[-1] == meshes[-1]["n_gt"] * meshes[-1]["n_pred"] - 1


# ------------------------------------------------------------------------------------------------------------------------ threshold
def test_threshold_cases_sit_on_the_comparison(ops):
    batch = mc.threshold_batch()
    for c in batch:
        w = c["want"]
        assert np.array_equal(w["row"], np.arange(c["n_gt"])) and mc.same_bits(w["dist"], c["exact"]) and set(c["exact"]) == {5.0, 7.0, 9.0, 11.0, 15.0}
        kinds = np.sign(c["fs"] - w["dist"])
        assert {-1.0, 0.0, 1.0} == set(kinds) and w["hits"] == int((kinds > 0).sum())           # hits only where fs is ABOVE the distance
        assert np.abs(c["fs"] - w["dist"]).max() <= np.spacing(15.0)
        assert int(np.sum(w["dist"] <= c["fs"])) > w["hits"]                                      # `<=` for `<` counts more
    assert [c["n_gt"] for c in batch] == [63, 64, 65]
    per, status, sc = mc.run_match(batch, DEV, fs=[c["fs"] for c in batch])
    assert status.tolist() == [0, 0, 0]
    for c, got in zip(batch, per):
        assert mc.check_matching(got, (c["want"]["row"], c["want"]["col"], c["want"]["dist"]), c["name"]) == 0
    mc.check_hits(sc["hits"], [c["want"]["hits"] for c in batch], "threshold")
    for k in mc.RATIOS:
        mc.check_bits(sc[k], np.array([c["want"][k] for c in batch]), k)
    h = mc.threshold_handmade()
    assert h["sizes"][0] == 129 and h["hits"][0] > 64 and all(0 < x < n for x, n in zip(h["hits"], h["sizes"]))
    hits, ratios = mc.run_handmade_scores(h, DEV)
    mc.check_hits(hits, h["hits"], "hand-made pairs")
    mc.check_bits(ratios, h["ratios"], "hand-made ratios")


# -------------------------------------------------------------------------------------------------------------------------- nearest
def test_nearest_tile_cases(ops):
    c = mc.nearest_tiles()
    assert sorted({len(b) for b in c["b"]}) == [1, 1023, 1024, 1025, 2048, 2049] and sorted({len(a) for a in c["a"]}) == [1, 255, 256, 257, 513]
    for a, b, arg in zip(c["a"], c["b"], c["arg"]):
        last_tile = (len(b) - 1) // mc.TILE * mc.TILE
        assert arg[0] == len(b) - 1 >= last_tile and (len(a) == 1 or arg[1] == 0)                 # the LAST tile for one source, the first for another
        assert (arg >= last_tile).any() and (len(a) == 1 or (arg < mc.TILE).any())
        mc.sum_premises(len(a), 3.0 ** 0.5)
    sq, d, flags = mc.run_nearest(ops, mc.cat(c["a"]), mc.ptr(c["a"]), mc.cat(c["b"]), mc.ptr(c["b"]), DEV)
    assert mc.check_nearest(sq, d, np.concatenate(c["sq"]), "tiles") == 0 and flags.tolist() == [0] * 6
    means = mc.run_segment_mean(ops, d, mc.ptr(c["a"]), DEV)
    mc.check_sum(means, c["oneway"], "one-way means")


def test_nearest_mesh_walk_case(ops):
    c = mc.nearest_walk()
    groups = mc.workgroup_meshes(c["a_ptr"], len(c["a"]))
    assert max(hi - lo + 1 for lo, hi in groups) >= 4 and c["a_ptr"][0] == 37 and len(groups) == 3
    lo, hi = groups[0]
    served = [m for m in range(lo, hi + 1) if mc.WALK_A[m] > 0]
    assert served == [0, 2, 5] and mc.WALK_B[2] == 0 and all(mc.WALK_A[m] == 0 for m in (1, 3, 4))  # a flagged mesh between healthy ones, empty ones around it
    assert np.isnan(c["want"][:37]).all() and np.isnan(c["want"][c["a_ptr"][2]:c["a_ptr"][3]]).all() and np.isnan(c["want"]).sum() == 40
    sq, d, flags = mc.run_nearest(ops, c["a"], c["a_ptr"], c["b"], c["b_ptr"], DEV)
    mc.check_nearest(sq, d, c["want"], "mesh walk")
    assert flags.tolist() == c["flags"]


def test_nearest_follows_np_min_on_nan(ops):
    c = mc.nearest_nan()
    pa = mc.ptr(c["a"])
    want = c["sq"]
    assert np.isnan(want[3]) and np.isnan(want[:pa[1]]).sum() == 1 and np.isnan(want[pa[1]:pa[2]]).all() and not np.isnan(want[pa[2]:]).any()
    sq, d, flags = mc.run_nearest(ops, mc.cat(c["a"]), pa, mc.cat(c["b"]), mc.ptr(c["b"]), DEV)
    mc.check_nearest(sq, d, want, "NaN")
    assert flags.tolist() == [0, 0, 0]
    j2j = mc.host(metrics.chamfer_j2j(mc.cat(c["a"]), pa, mc.cat(c["b"]), mc.ptr(c["b"]), device=DEV))
    assert np.isnan(j2j[:2]).all() and abs(j2j[2] - mo.chamfer(c["a"][2], c["b"][2])) <= SUM_TOL


# ---------------------------------------------------------------------------------------------------------------------------- means
def test_segment_mean_order_is_restated(ops):
    c = mc.mean_case()
    assert [len(x) for x in c["xs"]] == mc.MEAN_SIZES and all(0.0 < x.min() and x.max() < 4.0 for x in c["xs"] if len(x))
    for x in c["xs"]:
        mc.sum_premises(len(x), x.max(initial=0.0))
    assert np.isnan(c["order"][0]) and c["order"][1] == c["xs"][1][0] and c["order"][2] == (c["xs"][2][0] + c["xs"][2][1]) / 2
    mc.check_sum(c["order"], c["fsum"], "the kernel's order against fsum")
    # the restatement by hand for one size: thread t adds x[t], x[t + 256], ...; then the tree
    x = c["xs"][6]
    sh = [math.fsum([]) for _ in range(256)]
    for t in range(256):
        for v in x[t::256]:
            sh[t] = sh[t] + float(v)
    h = 128
    while h:
        for t in range(h):
            sh[t] = sh[t] + sh[t + h]
        h >>= 1
    assert np.float64(sh[0]) / np.float64(len(x)) == c["order"][6]
    got = mc.run_segment_mean(ops, c["x"], c["ptr"], DEV)
    mc.check_sum(got, c["fsum"], "emulated segment mean")
    bad = c["ptr"].copy()
    bad[4] = bad[5] + 1                                                                        # mesh 3 ends past its successor's start, mesh 4 descends
    got_bad = mc.run_segment_mean(ops, c["x"], bad, DEV)
    assert np.isnan(got_bad[4]) and mc.same_bits(got_bad[[1, 2, 5, 6, 7]], got[[1, 2, 5, 6, 7]])


def test_valid_mean_cases(ops):
    for c in mc.valid_mean_cases():
        got = mc.run_valid_mean(ops, c, DEV)
        mc.check_bits(got, c["want"], c["name"])
        assert np.isnan(c["want"]).all() == (c["valid"].sum() == 0)
    assert [c["x"].shape[1] for c in mc.valid_mean_cases()] == [9, 9, 1, 65]


# ---------------------------------------------------------------------------------------------------------------------------- bones
def test_bone_batches(ops):
    for c in mc.bone_batches():
        rigs = c["rigs"]
        assert sum(len(mo.bones_of(r)) for r in rigs) == c["n_bones"] == len(c["counts"])
        total = int(c["counts"].sum())
        assert total % 256 != 0 and total == sum(len(s) for s in c["samples"])
        chain, star = rigs
        n = len(chain.pos)
        assert [int(c["counts"][k]) for k in (0, n // 2 - 1, n - 2)] == [1, 1, 1]                  # zero-length bones at the start, middle, end
        steps = np.abs(star.pos[1:]).max(axis=1) / mo.STEP
        per_axis = [[s for s, p in zip(steps, star.pos[1:]) if np.argmax(np.abs(p)) == ax and s % 1.0 == 0.5] for ax in range(3)]
        assert all(len(a) >= 2 for a in per_axis), per_axis                                       # exact half steps on every axis
        star_counts = c["counts"][n - 1:]
        assert [int(x) for x, s in zip(star_counts, steps) if s % 1.0 == 0.5] == [int(np.round(s)) + 1 for s in steps if s % 1.0 == 0.5]
        samples, p = metrics.sample_skel(rigs, device=DEV)
        mc.check_bits(mc.host(samples), np.concatenate(c["samples"]), f"bones {c['n_bones']}")
        assert mc.host(p).tolist() == mc.ptr(c["samples"]).tolist()


def test_refused_bones(ops):
    c = mc.refused_bones()
    assert c["counts"][c["refused"]].tolist() == [0, 0, 0, 0] and (np.delete(c["counts"], c["refused"]) >= 1).all()
    counts, samples = mc.run_bone_ops(ops, c["pos"], c["bones"], DEV)
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
@pytest.mark.parametrize("with_rigs", [False, True])
def test_whole_batch_through_the_emulated_ops(ops, with_rigs):
    c = mc.whole_batch()
    want = c["want"] if with_rigs else c["want_plain"]
    assert want["num_invalid"] == 1 and not want["valid"][2] and 0 < want["hits"].sum() < sum(min(len(p), len(r.pos)) for p, r in zip(c["preds"], c["gt_rigs"]))
    for p, r in zip(c["preds"], c["gt_rigs"]):
        if len(p):
            assert mo.assignment_gap(mo.dist_matrix(p, r.pos)) > GAP
            mc.sum_premises(max(len(mo.sample_skel(r)), len(mo.sample_skel(mc.chain_rig(p)))), 4.0 ** 0.5)
    got = mc.run_whole(c, DEV, with_rigs)
    mc.check_whole(got, want, "whole batch")
    assert ("chamfer_j2b" in got) == with_rigs and got["status"].tolist() == [0] * 6


# ------------------------------------------------------------------------------------------------- the compare functions can fail
def test_planted_errors_are_rejected():
    c = mc.assign_cases()[4]
    good = (c["row"].copy(), c["col"].copy(), c["dist"].copy())
    assert mc.check_matching(good, good, "self") == 0
    col = c["col"].copy()
    col[[7, 8]] = col[[8, 7]]                                                                    # one swapped pair
    with pytest.raises(AssertionError, match="another matching"):
        mc.check_matching((c["row"], col, c["dist"]), good, "swapped pair")
    two = c["dist"].copy()
    two[3] = np.nextafter(np.nextafter(two[3], 9.0), 9.0)
    with pytest.raises(AssertionError, match="2 ulp"):
        mc.check_matching((c["row"], c["col"], two), good, "two ulp")
    with pytest.raises(AssertionError, match="hits"):
        mc.check_hits([5, 0, 6], [5, 0, 5], "one hit more")
    t = mc.nearest_tiles()
    sq = np.concatenate(t["sq"])
    off = sq.copy()
    off[700] = np.nextafter(off[700], 9.0)                                                       # one ulp in a squared distance
    with pytest.raises(AssertionError, match="squared minima"):
        mc.check_nearest(off, np.sqrt(sq), sq, "planted")
    m = mc.mean_case()["order"]
    off = m.copy()
    off[5] = np.nextafter(off[5], 9.0)                                                           # one ulp in a mean
    with pytest.raises(AssertionError, match="not bit-equal"):
        mc.check_bits(off, m, "planted mean")
    with pytest.raises(AssertionError, match="not bit-equal"):
        mc.check_bits(np.array([0.0, 1.0]), np.array([-0.0, 1.0]), "signed zero")
    tie = mc.tie_cases()[0]
    row, col = mo.linear_sum_assignment(tie["d"])
    mc.check_valid_matching((row, col, tie["d"][row, col]), tie["d"], tie["total"], "scipy's own")
    worse = col.copy()
    worse[0] = [j for j in range(8) if j not in col and tie["d"][0, j] != tie["d"][0, col[0]]][0]
    with pytest.raises(AssertionError, match="total"):
        mc.check_valid_matching((row, worse, tie["d"][row, worse]), tie["d"], tie["total"], "a worse matching")
    with pytest.raises(AssertionError, match="SUM_TOL"):
        mc.check_sum(np.array([1.0 + 2e-11]), np.array([1.0]), "planted sum")
