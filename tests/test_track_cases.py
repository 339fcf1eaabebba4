"""tests/track_cases.py without a device: every generator terminates within its attempts and the ORACLE ALONE confirms the conditions of
every case; the structures the cases are named after (entry counts per joint and per vertex, tree shapes, roots, the LDS boundaries)
are recounted here; ``tracking.pack_problems`` is checked on every case against ``tracking_oracle.bfs`` and an independent recount of
the joint-major entry copy; the float32 twin of the oracle is measured against the reference's own float32 results on the eight
``track_solve.npz`` cases; and the family maxima of the twin's deviations (the tolerance inputs of
tests/test_tracking_differential.py) are computed and printed (run with -s). The twin also goes through the very comparison function
the device file uses, so that code is proven before a device sees it."""
import numpy as np
import pytest

import track_cases as tc
import tracking_oracle as tk
from morig_amd import tracking
from test_tracking_oracle import SOLVE, SOLVE_META, solve_problem


def entries_per_joint(c):
    return np.bincount(c["prob"]["ent_j"], minlength=c["spec"]["J"])


def entries_per_vertex(c):
    return np.diff(c["prob"]["vptr"])


def depth_and_widths(c):
    level_ptr = tk.bfs(c["prob"]["parent"], c["prob"]["root"])[1]
    return len(level_ptr) - 2, np.diff(level_ptr)


# ------------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", tc.NAMES)
def test_every_case_is_generated_and_meets_its_conditions(name):
    c = tc.case(name)
    spec, prob, want = c["spec"], c["prob"], c["want"]
    J, V = spec["J"], spec["V"]
    assert 1 <= c["attempts"] <= tc.ATTEMPTS and c["iter_time"] in (1, 2, 3, 25, 200) and c["lr"] in (5e-2, 1e-3) and c["w_invis"] in (0.0, 0.25)
    assert len(prob["parent"]) == J and len(prob["vismask"]) == V == len(prob["constraints"]) and prob["root"] == tc.root_of(spec)
    for k in ("locals_in", "offsets", "ent_w", "ent_x", "constraints", "vismask"):
        assert prob[k].dtype == np.float32, k
    margin = tc.vis_margin(c)
    print(f"\n{name}: attempts {c['attempts']}, vismask margin {margin:.2e} (>= {tc.VIS_MARGIN}), last loss {want['loss']:.3e} (>= {tc.LOSS_MIN}), "
          f"largest last gradient entry {tc.grad_scale(want):.3e} (>= {tc.GRAD_MIN})")
    assert margin >= tc.VIS_MARGIN
    visible = prob["vismask"] > np.float32(c["thrd"])
    if spec["vis"] == "all_invisible":
        assert not visible.any() and c["w_invis"] == 0 and want["loss"] == 0 and tc.grad_scale(want) == 0
    else:
        assert want["loss"] >= tc.LOSS_MIN and tc.grad_scale(want) >= tc.GRAD_MIN
    if spec["vis"] == "all_visible":
        assert visible.all()
    if spec["vis"] in ("mixed", "on_threshold") and V > 8:
        assert visible.any() and not visible.all()
    # the skin: weights as a rig file holds them, ascending joints inside a vertex, the rows of a skinned vertex sum to one
    n = entries_per_vertex(c)
    w = prob["ent_w"].astype(np.float64)
    assert np.array_equal(prob["ent_w"], np.round(w, 4).astype(np.float32)) and w.min(initial=1.0) > 0
    rows = np.zeros(V)
    np.add.at(rows, tk.entry_vertex(prob), w)
    assert np.abs(rows[n > 0] - 1).max(initial=0) <= 5e-4
    for v in range(V):
        js = prob["ent_j"][prob["vptr"][v]:prob["vptr"][v + 1]]
        assert np.all(np.diff(js) > 0)
    if spec["skin"] == "random":
        assert n.min() >= 1 and n.max() <= 4 and (J < 4 or V < 64 or set(n.tolist()) == {1, 2, 3, 4})
    # the entries hold the vertices in their joints' rest frames: skinning at zero angles gives the mesh back (times the rounded row sums)
    _, G, P = tk.forward(np.zeros((J, 3)), np.zeros(3), prob)
    assert np.abs(tk.skin(G, P, prob) - c["vtx"] * rows[:, None]).max() <= 1e-6
    assert np.isfinite(prob["constraints"]).all()
    # the float32 twin through the device file's comparison
    twin = tc.oracle(c, np.float32)
    dev = tc.compare("float32 twin", name, twin)
    assert dev == tc.twin_deviation(name)


def test_sizes_the_kernel_branches_on():
    specs = [tc.SPECS[n] for n in tc.NAMES]
    V, J = {s["V"] for s in specs}, {s["J"] for s in specs}
    assert {1, 64, 255, 256, 257, 511, 512, 513, 1023, 1024, 2049} <= V and {1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 300} <= J
    assert {s["iters"] for s in specs} == {1, 2, 3, 25, 200} and sum(s["iters"] == 200 for s in specs) == 1
    assert {s["lr"] for s in specs} == {5e-2, 1e-3} and {s["w_invis"] for s in specs} == {0.0, 0.25}
    assert {s["root"] for s in specs} == {"first", "last", "mid"} and len(tc.NAMES) >= 28
    # step D wraps: more joints than waves on either workgroup size; the per-thread joint loops wrap on 256 threads, the translation
    # slot j == J on a thread's second pass; a level wider than the workgroup
    assert any(s["J"] > 4 and s["V"] <= 512 for s in specs) and any(s["J"] > 16 and s["V"] > 512 for s in specs)
    assert any(s["J"] >= 256 and s["V"] <= 512 for s in specs)
    assert depth_and_widths(tc.case("star300"))[1].max() == 300 and tc.SPECS["star300"]["V"] <= 512
    for batch in tc.BATCHES.values():                                          # max_iter exceeds a problem's own
        assert len({tc.SPECS[n]["iters"] for n in batch}) > 1
    assert set(sum(tc.BATCHES.values(), ())) == set(tc.NAMES)
    assert max(tc.SPECS[n]["V"] for n in tc.BATCHES["threads256"]) == 512 < max(tc.SPECS[n]["V"] for n in tc.BATCHES["threads1024"])
    assert set(tc.BATCHES["threads256"]) < set(tc.BATCHES["threads1024"])


def test_lds_boundaries():
    s = tc.lds_sizes()
    Jl, K64 = tc.LDS_JOINTS, 64 * 1024
    print(f"\ndynamic LDS at {Jl} joints: V = {s['under']}: {tc.lds_bytes(Jl, s['under'])} B, V = {s['over']}: {tc.lds_bytes(Jl, s['over'])} B, "
          f"V = {s['largest']}: {tc.lds_bytes(Jl, s['largest'])} B (+ {tc.LDS_STATIC} = {tc.lds_bytes(Jl, s['largest']) + tc.LDS_STATIC} of "
          f"{tc.LDS_LIMIT}); exactly 64 KiB at (J, V) = {s['exact']}")
    assert tc.lds_bytes(Jl, s["under"]) <= K64 < tc.lds_bytes(Jl, s["over"]) and s["over"] == s["under"] + 1 > 513
    assert tc.lds_bytes(Jl, s["largest"]) + tc.LDS_STATIC <= tc.LDS_LIMIT < tc.lds_bytes(Jl, s["largest"] + 1) + tc.LDS_STATIC
    assert s["exact"] is not None and tc.lds_bytes(*s["exact"]) == K64 and "lds_exactly_64k" in tc.NAMES
    for name in ("star300", "j257_v512"):                                      # 256 threads above 64 KiB
        sp = tc.SPECS[name]
        assert sp["V"] <= 512 and sp["J"] >= 257 and tc.lds_bytes(sp["J"], sp["V"]) > K64
    for name, batch in tc.BATCHES.items():                                     # every batch fits
        lds = tc.lds_bytes(max(tc.SPECS[n]["J"] for n in batch), max(tc.SPECS[n]["V"] for n in batch))
        assert lds + tc.LDS_STATIC <= tc.LDS_LIMIT, name
    # the thread count is a function of the vertex count alone: 12 bytes more per vertex on either side, 8 bytes per wave at the switch
    assert tc.lds_bytes(5, 512) - tc.lds_bytes(5, 511) == 12 and tc.lds_bytes(5, 513) - tc.lds_bytes(5, 512) == 12 + 8 * (16 - 4)


def test_trees():
    depth, widths = depth_and_widths(tc.case("chain_depth64"))
    assert depth == 64 and widths.max() == 1
    depth, widths = depth_and_widths(tc.case("star300"))
    assert depth == 1 and widths.tolist() == [1, 300]
    root = tc.case("star300")["prob"]["root"]
    assert 0 < root < 300 and (tc.case("star300")["prob"]["parent"] == root).sum() == 300        # the child loop of step E
    depth, widths = depth_and_widths(tc.case("binary255"))
    assert depth == 7 and widths.tolist() == [1, 2, 4, 8, 16, 32, 64, 128]
    assert max(depth_and_widths(tc.case(n))[0] for n in tc.NAMES) == 64
    for name in tc.NAMES:
        c = tc.case(name)
        assert c["prob"]["parent"][c["prob"]["root"]] == -1 and (c["prob"]["parent"] < 0).sum() == 1


def test_skin_entries():
    for name in ("entries_per_joint_256", "entries_per_joint_1024"):
        c = tc.case(name)
        per = entries_per_joint(c)
        assert [per[j] for j in range(6)] == [0, 1, 63, 64, 65, 129] and per[6:].min() > 0 and per.sum() == len(c["prob"]["ent_j"])
    assert tc.SPECS["entries_per_joint_256"]["V"] <= 512 < tc.SPECS["entries_per_joint_1024"]["V"]
    c = tc.case("entries_per_vertex")
    n = entries_per_vertex(c)
    assert set(n.tolist()) == {0, 1, 8, 3} and min((n == k).sum() for k in (0, 1, 8)) >= 64
    c = tc.case("all_on_one_joint")
    assert set(c["prob"]["ent_j"].tolist()) == {2} and c["prob"]["parent"][2] >= 0
    silent = ~tc.subtree_has_entries(c["prob"]["parent"], c["prob"]["ent_j"])
    assert silent.sum() == 2 and np.all(c["want"]["g_angles"][silent] == 0) and np.all(c["want"]["g_angles"][~silent] != 0)
    c = tc.case("v257_j16_root_mid_w_invis")                                  # joints without weight inside a random skin
    assert {3, 11}.isdisjoint(c["prob"]["ent_j"].tolist())


def test_threshold_vertex_is_judged_on_the_float32_arrays():
    c = tc.case("on_threshold")
    k, vis = c["on_threshold"], c["prob"]["vismask"]
    assert vis[k] == np.float32(tc.THRD) and float(vis[k]) > tc.THRD                # float32(0.3) is above the float64 0.3 ...
    mask = tk.mask_of(vis, np.float32(c["thrd"]), c["w_invis"])
    assert mask[k] == c["w_invis"] == 0.25                                          # ... and not above itself: the vertex is invisible
    assert tk.mask_of(vis.astype(np.float64), c["thrd"], c["w_invis"])[k] == 1.0    # a float64 comparison would have seen it


# ------------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("name", tc.NAMES)
def test_pack_problems_against_the_oracle_tree_and_a_recount(name):
    c = tc.case(name)
    prob, J, V = c["prob"], c["spec"]["J"], c["spec"]["V"]
    other = tc.case("v64_j2")["prob"]                                          # a neighbour in front: every offset is non-zero
    t, n, max_j, max_v, max_iter, joint_ptr, vert_ptr = tracking.pack_problems([tc.problem("v64_j2"), tc.problem(name)], "cpu")
    t = {k: v.numpy() for k, v in t.items()}
    j0, v0, e0, E = 2, 64, len(other["ent_j"]), len(prob["ent_j"])
    assert n == 2 and max_j == max(J, 2) and max_v == max(V, 64) and max_iter == max(c["iter_time"], 2)
    assert joint_ptr == [0, 2, 2 + J] and vert_ptr == [0, 64, 64 + V] and t["iter_time"].tolist() == [2, c["iter_time"]]
    order, level_ptr, lo, hi = tk.bfs(prob["parent"], prob["root"])
    lv0, lv1 = t["level_off"][1], t["level_off"][2]
    assert np.array_equal(t["order"][j0:], order) and np.array_equal(t["level_ptr"][lv0:lv1], level_ptr) and lv1 == len(t["level_ptr"])
    assert np.array_equal(t["child_lo"][j0:], lo) and np.array_equal(t["child_hi"][j0:], hi) and np.array_equal(t["parent"][j0:], prob["parent"])
    assert t["root"].tolist() == [other["root"], prob["root"]]
    # vertex-major entries as given
    assert np.array_equal(t["vptr"][v0:], prob["vptr"] + e0) and np.array_equal(t["vent_j"][e0:], prob["ent_j"])
    xw = t["vent_xw"].reshape(-1, 4)[e0:]
    assert np.array_equal(xw[:, :3], prob["ent_x"]) and np.array_equal(xw[:, 3], prob["ent_w"])
    # the joint-major copy, recounted entry by entry: joint after joint, inside a joint the vertices ascending
    buckets = [[] for _ in range(J)]
    for v in range(V):
        for e in range(prob["vptr"][v], prob["vptr"][v + 1]):
            buckets[prob["ent_j"][e]].append((v, e))
    jptr, at = t["jptr"][j0:], e0
    jxw = t["jent_xw"].reshape(-1, 4)
    for j in range(J):
        assert jptr[j] == at and jptr[j + 1] == at + len(buckets[j])
        es = np.array([e for _, e in buckets[j]], dtype=np.int64)
        assert np.array_equal(t["jent_v"][at:at + len(es)], [v for v, _ in buckets[j]])
        assert np.array_equal(jxw[at:at + len(es), :3], prob["ent_x"][es].reshape(-1, 3)) and np.array_equal(jxw[at:at + len(es), 3], prob["ent_w"][es])
        at += len(es)
    assert at == e0 + E == len(t["jent_v"]) == t["jptr"][-1] == t["vptr"][-1]
    b1, b2 = tracking.bias_tables(max_iter)
    assert np.array_equal(t["bias1"], b1) and np.array_equal(t["bias2_sqrt"], b2)


# ------------------------------------------------------------------------------------------------------------------- the twin and the bounds
def test_tolerance_inputs():
    print("\n" + tc.table())
    for family in tc.FAMILIES:
        assert len(tc.FAMILIES[family]) >= 5
        for q, d in tc.deviations(family).items():
            assert np.isfinite(d) and d > 0, (family, q, d)
            want = max(tc.FACTOR * d, tc.FLOOR)
            assert tc.bounds(family)[q] == (min(want, tc.CAP) if q == "positions" else want)
    assert tc.FACTOR == 10.0 and tc.FLOOR == 2.0 ** -23 and tc.CAP == 1e-5
    assert set(tc.FAMILIES["short"]) | set(tc.FAMILIES["long"]) == set(tc.NAMES)


def test_twin_is_float32_throughout():
    c = tc.case("v257_j16_root_mid_w_invis")
    twin = tc.oracle(c, np.float32)
    for k in ("angles", "trans", "locals", "globals", "jpos", "g_angles", "g_trans"):
        assert twin[k].dtype == np.float32, k
    opt = tk.Adam(3, 5e-2, dtype=np.float32)
    p = opt.step(np.full(3, 0.01, dtype=np.float32), np.array([1e-3, -2.0, 0.0], dtype=np.float32))
    assert p.dtype == opt.m.dtype == opt.v.dtype == np.float32


@pytest.mark.parametrize("name", SOLVE_META["cases"])
def test_twin_stands_in_for_the_reference_arithmetic(name):
    """on the eight recorded cases the twin is as far from the float64 oracle as the reference's own float32 result is (the deviations
    the generator stored), within a factor of ten either way, quantity by quantity"""
    par, prob = SOLVE_META["params"][name], solve_problem(SOLVE, SOLVE_META, name)
    args = (prob, par["iter_time"], par["lr"], par["w_invis"], np.float32(par["thrd"]))
    want, twin = tk.solve(*args), tk.solve(*args, dtype=np.float32)
    dev = tc.deviation_of(twin, want)
    posed = np.abs(tk.skin(twin["globals"], twin["jpos"], prob, np.float32) - tk.skin(want["globals"], want["jpos"], prob)).max()
    mine = dict(dev_angles=dev["angles"], dev_vertices=max(dev["positions"], float(posed)), dev_loss=dev["loss"], dev_grad=dev["gradient"])
    stored = SOLVE_META["deviations"][name]
    print(f"\n{name}: " + ", ".join(f"{k[4:]} twin {mine[k]:.2e} | reference {stored[k]:.2e}" for k in mine))
    for k in mine:
        if stored[k] == 0 or mine[k] == 0:                                     # all_invisible: zero loss and gradient in either
            assert stored[k] == mine[k] == 0, k
        else:
            assert stored[k] / 10 <= mine[k] <= stored[k] * 10, (k, mine[k], stored[k])
