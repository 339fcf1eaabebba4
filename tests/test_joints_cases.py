"""CPU: the case tables of tests/joints_cases.py. Every case reaches the branch of csrc/joints.hip it names (shown on small Python
models of the kernels' control flow: bin index and population for the selections, the walk of `s` for the suppression, the box test for
the box kernel), the exactness and margin conditions of the mean-shift tables hold, and the numpy restatements the device is held to
agree with the independent reference oracle/joints.py: selection, counts, suppression and inside test exactly, mean-shift within 1e-11
(the bar tests/test_joints_host.py uses for modes of unit-box inputs; the observed maximum is printed)."""
import math

import numpy as np

import joints_cases as jc
from oracle import joints as O


def as_double(key):
    return float(np.array([key], dtype=np.uint64).view(np.float64)[0])


# ------------------------------------------------------------------------------------------------------------------ selection
def test_selection_restatement_equals_the_oracle():
    for c in jc.select_cases():
        if len(c["x"]) > 1000:
            continue                                                          # the oracle's n x n matrix; full16 is held row by row below
        for q in sorted(set(c["qs"]) | {0.0, 0.04, 0.3, 1.0}):
            q = min(q, 1.0)
            kth = jc.kth_distances(c["x"], jc.k_of(len(c["x"]), q))
            assert float(kth.sum() / len(kth)) == O.estimate_bandwidth(c["x"], q), (c["name"], q)
            want, bound = jc.bandwidth_bound(kth)
            assert abs(float(kth.sum() / len(kth)) - want) <= bound
    r = jc.select_ragged()
    for x in r["sets"]:
        for q in r["qs"]:
            if len(x):
                kth = jc.kth_distances(x, jc.k_of(len(x), q))
                assert float(kth.sum() / len(kth)) == O.estimate_bandwidth(x, q)
    big = next(c for c in jc.select_cases() if c["name"] == "full16")
    d = np.sqrt(((big["x"][big["rows"]][:, None, :] - big["x"][None, :, :]) ** 2).sum(-1))
    for k in (5, 32767):
        assert np.array_equal(np.partition(d, k - 1, axis=1)[:, k - 1], jc.kth_distances(big["x"], k, big["rows"]))


def all_ks(c):
    n = len(c["x"])
    return sorted(set(c["ks"]) | {jc.k_of(n, q) for q in c["qs"]})


def test_selection_models_select_the_kth_key():
    """both control-flow models end on the key whose root kth_distances gives, for every k of every case (first workgroup's rows)"""
    for c in jc.select_cases():
        rows = range(min(len(c["x"]), jc.K4_R))
        for k in all_ks(c):
            want = jc.kth_distances(c["x"], k, list(rows))
            for r in rows:
                keys = jc.keys_of(c["x"], r)
                assert math.sqrt(as_double(jc.model_kth4(keys, k)["key"])) == want[r], (c["name"], k, r)
                assert math.sqrt(as_double(jc.model_kth1(keys, k)["key"])) == want[r], (c["name"], k, r)


def test_selection_cases_reach_their_branches():
    cases = {c["name"]: c for c in jc.select_cases()}
    sizes = [len(c["x"]) for c in cases.values() if c["name"].startswith("n")]
    assert {n % jc.K4_R for n in sizes} == {0, 1, 2, 3} and {255, 256, 257, 513} <= set(sizes)          # shadow rows; the 256-thread stride
    assert all(c["max_n_one_row"] > 65535 for c in cases.values())
    assert all(jc.k_of(len(c["x"]), q) in c["ks"] for c in cases.values() if not c["name"].startswith("n") for q in c["qs"]
               if c["name"] not in ("coincident20", "x1000", "x1e-6", "x1e-10", "full16"))
    # K4_LIST: 64 bit-identical keys in the selected bin take the list pass, 65 take all five histogram passes
    for m, path, pops in ((64, "list", [64]), (65, "exhausted", [65] * 5)):
        c = cases[f"tie{m}"]
        keys = jc.keys_of(c["x"], 0)
        assert int((keys == np.float64(jc.TIE_D2).view(np.uint64)).sum()) == m and 2.0 ** -31 <= jc.TIE_D2 < 2.0
        for k in (5, c["tie_k"], 4 + m):
            got = jc.model_kth4(keys, k)
            assert (got["path"], got["pops"]) == (path, pops) and as_double(got["key"]) == jc.TIE_D2, (m, k, got)
        assert as_double(jc.model_kth4(keys, 5 + m)["key"]) > jc.TIE_D2 and as_double(jc.model_kth4(keys, 4)["key"]) < jc.TIE_D2
        print(f"tie{m}: pass-0 bin {got['first_bin']} holds {got['pops'][0]} keys -> {path}")
    # KTH_SMALL: 8 identical keys stop early with a full list, 9 run to pass 0 and overflow it
    got = jc.model_kth1(jc.keys_of(cases["small8"]["x"], 0), cases["small8"]["tie_k"])
    assert got["pop"] == jc.KTH_SMALL and got["nlist"] == jc.KTH_SMALL and got["stop"] > 0, got
    print("small8: stops after pass", got["stop"], "with", got["pop"], "keys")
    got = jc.model_kth1(jc.keys_of(cases["small9"]["x"], 0), cases["small9"]["tie_k"])
    assert got["pop"] == jc.KTH_SMALL + 1 and got["nlist"] == jc.KTH_SMALL + 1 and got["stop"] == 0, got
    # the same two constants with distinct keys: a full list that has to be ranked / sorted, and one key too many for it
    for m in (64, 65):
        c = cases[f"bin{m}"]
        keys = jc.keys_of(c["x"], 0)
        for k in c["ks"]:
            got = jc.model_kth4(keys, k)
            assert got["pops"][0] == m and got["path"] == "list" and len(got["pops"]) == (1 if m == 64 else 2), (m, k, got)
        group = np.sort(keys)[4:4 + m]
        assert len(np.unique(group)) == m and len({int(g) >> 46 for g in group}) == 1
        print(f"bin{m}: {m} distinct keys in bin {got['first_bin']} of pass 0, histogram passes {len(got['pops'])}")
    for m in (8, 9):
        c = cases[f"near{m}"]
        keys = jc.keys_of(c["x"], 0)
        assert len(np.unique(np.sort(keys)[c["below"]:c["below"] + m])) == m
        for k in c["ks"]:
            got = jc.model_kth1(keys, k)
            if m == 8:
                assert got["pop"] == got["nlist"] == jc.KTH_SMALL and got["stop"] > 0, got
            else:
                assert jc.KTH_SMALL + 1 in got["pops"] and got["pop"] <= jc.KTH_SMALL and got["stop"] > 0, got
        print(f"near{m}: selected-bin populations pass by pass {got['pops']}")
    keys = jc.keys_of(cases["coincident20"]["x"], 0)
    assert jc.model_kth4(keys, 9)["path"] == "generic_lo"
    got = jc.model_kth1(keys, 9)
    assert (got["stop"], got["pop"], got["nlist"]) == (0, 20, 20)
    # one workgroup, three states
    c = cases["mixed"]
    for k in (2, 4, 5):
        paths = [jc.model_kth4(jc.keys_of(c["x"], r), k)["path"] for r in range(4)]
        assert paths[:2] == ["generic_lo", "generic_total"] and all(p in ("list", "exhausted") for p in paths[2:]), (k, paths)
    for name, path, ks in (("x1000", "generic_total", (2, 19)), ("x1e-10", "generic_lo", (1, 2, 19))):
        c = cases[name]
        assert all(jc.model_kth4(jc.keys_of(c["x"], r), k)["path"] == path for r in range(len(c["x"])) for k in ks), name
    c = cases["x1e-6"]                                                                     # 2^-63 <= d2 < 2: pass 0 takes these
    assert all(jc.model_kth4(jc.keys_of(c["x"], r), k)["path"] in ("list", "exhausted") for r in range(len(c["x"])) for k in (2, 19))
    # 16-bit halves: row 0's bin holds 65 534 keys, the largest count a set of kth_nn4_kernel can give; row 1 shares its words
    c = cases["full16"]
    assert len(c["x"]) == 65535
    got = jc.model_kth4(jc.keys_of(c["x"], 0), 5)
    assert got["path"] == "exhausted" and got["pops"] == [65534] * 5 and 65534 <= 0xffff and as_double(got["key"]) == 0.25
    assert jc.model_kth4(jc.keys_of(c["x"], 1), 5)["path"] == "generic_lo"                 # 10 923 coincident copies: mixed with row 0
    assert jc.model_kth4(jc.keys_of(c["x"], 1), jc.k_of(65535, 0.5))["path"] == "exhausted"


# --------------------------------------------------------------------------------------------------------------------- counts
def test_counts_restatement_and_threshold():
    sets = [(c["name"], c["x"], c["hs"]) for c in jc.count_cases()]
    r = jc.count_ragged()
    sets += [(f"ragged{b}", x, tuple(h[b] for h in r["hs"])) for b, x in enumerate(r["sets"]) if len(x)]
    assert [len(c["x"]) for c in jc.count_cases()] == list(jc.COUNT_SIZES)
    for name, x, hs in sets:
        d2 = jc.sqdist(x, x)
        attn = np.zeros(len(x), np.float32)
        per_h = []
        for h in hs:
            got = jc.counts(x, h)
            assert np.array_equal(got, O.nms_meanshift(x, attn, h, 0.02)[2]), (name, h)
            T = jc.sqrt_le_threshold(h)
            assert np.array_equal(d2 <= T, np.sqrt(d2) <= h) and np.sqrt(T) <= h < np.sqrt(np.nextafter(T, np.inf)), (name, h)
            per_h.append(got)
        d, below, above, zero = hs
        if len(x) > 1:
            assert d > 0.0 and (np.sqrt(d2[0]) == d).any()                                         # the bandwidth is a rooted distance that occurs
            assert ((np.sqrt(d2[0]) == d) & (d2[0] > d * d)).any() and jc.sqrt_le_threshold(d) > d * d, name   # ... that h * h would miss
            assert per_h[1][0] < per_h[0][0] and per_h[2][0] >= per_h[0][0], name                  # one ulp below drops that pair
            assert per_h[3][0] >= 2 and zero == 0.0                                                # coincident points at bandwidth 0
        print(name, "counts of row 0 at d, below, above, 0:", [int(p[0]) for p in per_h])


# --------------------------------------------------------------------------------------------------------------------- greedy
def all_greedy():
    return list(jc.greedy_cases()) + [m for m in jc.greedy_ragged()["meshes"] if len(m["x"])]


def test_greedy_restatement_equals_the_oracle_and_the_walk():
    assert [len(c["x"]) for c in jc.greedy_cases()][:8] == [1, 63, 64, 65, 1023, 1024, 1025, 2100]
    assert tuple(c["name"] for c in jc.greedy_cases()) == jc.GREEDY_NAMES
    assert [len(m["x"]) for m in jc.greedy_ragged()["meshes"]] == list(jc.GREEDY_RAGGED)
    for c in all_greedy():
        args = (c["x"], c["attn"], c["h"])
        _, alive, cnt = O.nms_meanshift(c["x"], c["attn"], c["h"], c["thrd_density"], c["thrd_attn"])
        assert np.array_equal(cnt, jc.counts(c["x"], c["h"]))
        assert np.array_equal(jc.greedy(*args, c["orders"]["nms"], c["thrd_density"], c["thrd_attn"]), alive), c["name"]
        for name, order in c["orders"].items():
            assert sorted(order.tolist()) == list(range(len(c["x"])))
            walked, visits, skips = jc.greedy_walk(*args, order, c["thrd_density"], c["thrd_attn"])
            assert np.array_equal(walked, jc.greedy(*args, order, c["thrd_density"], c["thrd_attn"])), (c["name"], name)
        assert np.array_equal(c["orders"]["rev"], c["orders"]["nms"][::-1])


def test_greedy_cases_reach_their_branches():
    cases = {c["name"]: c for c in jc.greedy_cases()}
    c = cases["skip2100"]
    alive, visits, skips = jc.greedy_walk(c["x"], c["attn"], c["h"], c["orders"]["nms"], c["thrd_density"])
    assert visits[0] == 0 and skips == [1] and visits[1] >= 1 + jc.NMS_T, (visits[:3], skips)       # a full window of dead entries
    assert int(jc.counts(c["x"], c["h"]).max()) == 1100 and int(alive.sum()) == 1
    print("skip2100: visit 0, window skipped at s = 1, next visit at order index", visits[1])
    c = cases["attn_equal"]
    assert c["thrd_density"] == 1.0 and c["attn"][:10].max() == jc.ATTN_AT and c["attn"][10:20].max() == jc.ATTN_ABOVE
    assert jc.ATTN_AT == np.float32(0.7) and jc.ATTN_ABOVE > np.float32(0.7) and c["attn"][20:].max() < np.float32(0.7)
    for order in c["orders"].values():
        alive = jc.greedy(c["x"], c["attn"], c["h"], order, 1.0)
        assert (int(alive[:10].sum()), int(alive[10:20].sum()), int(alive[20:].sum())) == (0, 1, 0)
    c = cases["density_equal"]
    assert len(c["x"]) == 50 and (jc.counts(c["x"], c["h"]) == 1).all() and not 1 / 50 > c["thrd_density"]
    assert not jc.greedy(c["x"], c["attn"], c["h"], c["orders"]["nms"], c["thrd_density"]).any()
    c = cases["density_above"]
    assert len(c["x"]) == 50 and (jc.counts(c["x"], c["h"]) == 2).all()
    assert int(jc.greedy(c["x"], c["attn"], c["h"], c["orders"]["nms"], c["thrd_density"]).sum()) == 25


# ----------------------------------------------------------------------------------------------------------------- mean-shift
def test_lattice_cases_are_exact_in_any_order():
    """every term of every sum is an integer multiple of 2^-21 (2^-15 for the weights' sum) and the sum of their magnitudes stays below
    2^53 of those units: every partial sum in any order is exact. The float restatement equals the integer sums."""
    sizes = []
    for c in jc.lattice_cases():
        x, w = c["x"], c["w"]
        assert c["h"] == 0.25 and c["max_iter"] == 2 and np.abs(x).max() <= 1.0
        ints, worst = jc.lattice_sums_int(x, w)
        assert worst < 2 ** 53
        got = jc.meanshift_sums(x, w, c["h"])
        assert all(jc.same_bits(got[a], ints[a] / 2.0 ** 21) for a in range(3)) and jc.same_bits(got[3], ints[3] / 2.0 ** 15), c["name"]
        if w is not None:
            assert (w == 0).any() and w.dtype == np.float32
        sizes.append(len(x))
    assert sizes[:-1] == list(jc.SMALL_SIZES) + [jc.BIG] and any(c["w"] is not None and not c["w"].any() for c in jc.lattice_cases())


def test_box_cases_reach_the_second_chunk_and_every_wave():
    c = next(c for c in jc.lattice_cases() if len(c["x"]) == jc.BIG)
    for x, h in ((c["x"], c["h"]), (jc.generic_cases()[-1]["meshes"][1]["x"], 0.08)):
        near = jc.near_boxes(x, h)
        n_boxes = near.shape[0]
        assert n_boxes > 256
        both = near[:, :256].any(1) & near[:, 256:].any(1)
        print(f"n = {len(x)}: {n_boxes} boxes, {int(both.sum())} target boxes with near boxes in both chunks, near boxes per target "
              f"{int(near.sum(1).min())} .. {int(near.sum(1).max())}")
        assert both.any() and near.sum(1).max() > 8 and not near.all()                              # both chunks; two rounds of the deal; culling
    for c in jc.lattice_cases()[:len(jc.SMALL_SIZES)]:
        assert jc.near_boxes(c["x"], c["h"]).shape[0] == -(-len(c["x"]) // jc.MSB)


def test_meanshift_restatement_against_the_oracle():
    """within 1e-11 of oracle.meanshift_cluster wherever its n x n x 3 temporaries are affordable (every set of at most 513 points)"""
    worst = 0.0
    for c in jc.lattice_cases():
        if len(c["x"]) <= 513:
            got, _ = jc.meanshift(c["x"], c["w"], c["h"], 2)
            w = None if c["w"] is None else c["w"].reshape(-1, 1)
            worst = max(worst, float(np.abs(got - O.meanshift_cluster(c["x"], c["h"], w, 2)).max()))
    for c in jc.generic_cases():
        for m in c["meshes"]:
            if 0 < len(m["x"]) <= 513:
                for it in c["max_iters"]:
                    want = O.meanshift_cluster(m["x"], m["h"], m["w"].reshape(-1, 1), it)
                    worst = max(worst, float(np.abs(jc.modes_at(m, it) - want).max()))
    print("restatement against oracle.meanshift_cluster: max |diff| %.3e" % worst)
    assert worst <= jc.MODE_TOL


def test_generic_cases_keep_their_margin_and_stop_where_stated():
    cases = {c["name"]: c for c in jc.generic_cases()}
    assert [len(cases[f"n{n}"]["meshes"][0]["x"]) for n in jc.SMALL_SIZES + (jc.BIG,)] == list(jc.SMALL_SIZES + (jc.BIG,))
    for c in cases.values():
        for m in c["meshes"]:
            assert all(abs(d - jc.STOP) > jc.STOP_MARGIN for d in m["diffs"]), c["name"]
            assert len(m["states"]) == len(m["diffs"]) + 1 and all(d > jc.STOP for d in m["diffs"][:-1])
            assert jc.same_bits(jc.modes_at(m, 1), np.asarray(m["x"]))
    quick, slow = cases["stop_pair"]["meshes"]
    assert 2 <= len(quick["diffs"]) < 11 and quick["diffs"][-1] <= jc.STOP and len(slow["diffs"]) == 11 and min(slow["diffs"]) > jc.STOP
    print("stop_pair: the tight mesh stops after", len(quick["diffs"]), "steps, its neighbour runs 11")
    assert [len(m["x"]) for m in cases["ragged"]["meshes"]] == [0, 1, 32, 0, 33, 31, 0]
    assert [len(m["x"]) for m in cases["ragged_big"]["meshes"]] == [257, 8225, 40] and len(cases["ragged_big"]["meshes"][1]["diffs"]) == 2
    assert any(len(m["diffs"]) == 11 for n in jc.SMALL_SIZES for m in cases[f"n{n}"]["meshes"])


# ---------------------------------------------------------------------------------------------------------------- inside test
def test_inside_edges_round_where_stated():
    vox = jc.checker_grid()
    seen = set()
    for pt, axis, v, right, wrong, mid in jc.inside_edge_table():
        assert int(np.round(v)) == right and (abs(right - wrong) == 1 or v == 1e15), (v, right, wrong)
        assert jc.cell_value(vox, right, mid) != jc.cell_value(vox, wrong, mid), v                  # the fill differs between the two cells
        got = jc.inside(pt[None], vox, jc.EXACT_TRANSLATE, jc.EXACT_SCALE, jc.EXACT_DIMS0)[0]
        assert bool(got) == jc.cell_value(vox, right, mid), (v, axis)
        assert jc.voxel_coordinate(pt[axis], 0.0, jc.EXACT_SCALE, jc.EXACT_DIMS0) == v
        seen.add(v)
    vs = sorted(seen)
    assert {-0.5, 0.5, 1.5, 2.5, 86.5, 87.5, 88.0, -1.0, 1e15} <= seen and len(vs) == 11               # the halves are reached exactly
    assert vs[1] < -0.5 and vs[1] > -0.5000001 and 87.4999999 < vs[-4] < 87.5
    by_v = {v: (right, mid) for _, _, v, right, _, mid in jc.inside_edge_table()}
    assert jc.cell_value(vox, *by_v[-0.5]) is True and jc.cell_value(vox, *by_v[87.5]) is False     # -0.5 -> voxel 0, inside; 87.5 -> 88, outside


def test_inside_restatement_equals_the_oracle():
    assert [len(c["pts"]) for c in jc.inside_cases()] == [n for n in jc.INSIDE_SIZES for _ in range(2)]
    for c in jc.inside_cases():
        got = jc.inside(c["pts"], c["vox"], c["translate"], c["scale"], c["dims"][0])
        _, idx = O.inside_check(np.asarray(c["pts"]), c["vox"], c["translate"], c["scale"], c["dims"])
        want = np.zeros(len(c["pts"]), dtype=bool)
        want[np.atleast_1d(idx)] = True
        assert np.array_equal(got, want), c["name"]
        assert np.isfinite(c["pts"]).all() and np.abs(c["pts"]).max() <= 1e15
        if len(c["pts"]) > 1:
            assert got.any() and not got.all(), c["name"]
