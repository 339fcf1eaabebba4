"""tests/piecewise_cases.py without a device: every generator terminates within its attempts and the ORACLE ALONE confirms the conditions
and the structural property of every case; the oracle's discrete results -- counts, selections, refit flags, seeds, labels, members,
iteration counts -- are the same in float64 and in longdouble, which proves the margins real; the generator is deterministic; the
packing the device file uses (lists per mesh, sample slices per mesh) round-trips through morig_amd/piecewise.py on the emulated op layer
(tests/piecewise_emulate.py), whose results then pass the very comparison functions the device file uses; and those functions reject
planted errors. The yardsticks of tests/test_piecewise_differential.py (float64 oracle against longdouble oracle, per family) are
computed and printed here (run with -s)."""
import copy

import numpy as np
import pytest

import piecewise_cases as pc
import piecewise_emulate
import piecewise_oracle as po
from morig_amd import piecewise, runtime


@pytest.fixture()
def ops():
    emu = piecewise_emulate.PiecewiseOps()
    runtime._test_ops = emu
    try:
        yield emu
    finally:
        runtime._test_ops = None


def flat(runs):
    return [d for _, dd in runs for d in dd]


# ------------------------------------------------------------------------------------------------------------------- k-means
@pytest.mark.parametrize("name", pc.KM_NAMES)
def test_kmeans_case_meets_its_conditions_in_the_oracle_alone(name):
    c = pc.km_case(name)
    s, (labels, st) = c["spec"], c["want"]
    print(f"\n{name}: attempts {c['attempts']}, V {s['V']} D {s['D']} K {s['K']} {s['dtype']}, {st['n_iter']} iterations, {st['n_kept']} kept, "
          f"{len(st['reseeded'])} reseeds, row margin {st['row_margin']:.1e}, fit margin {st['fit_margin']:.1e}, reseed margin "
          f"{st['reseed_margin']:.1e}")
    assert 1 <= c["attempts"] <= pc.ATTEMPTS and s["max_iter"] <= 100 and s["V"] <= 2049
    assert c["X"].dtype == np.dtype(s["dtype"]) and c["verts"].dtype == np.float64 and 0 <= c["first"] < s["V"]
    assert np.abs(np.sqrt(np.sum(c["X"].astype(np.float64) ** 2, axis=1)) - 1).max() < 1e-6          # unit rows (D = 1: +-1)
    assert pc.KM_COND == dict(row_margin=1e-5, fit_margin=1e-5, reseed_margin=1e-5)
    for k, v in pc.KM_COND.items():
        assert st[k] >= v, (name, k, st[k])
    assert pc.km_property(c, labels, st), (name, s["prop"])
    # the same text in longdouble decides alike
    long_labels, long_st = pc.km_oracle(c, pc.LONG)
    assert long_st["centres_euc"].dtype == pc.LONG and np.finfo(pc.LONG).nmant >= 63
    pc.km_compare("longdouble oracle", name, long_labels, long_st, centres=False)
    assert long_st["reseeded"] == st["reseeded"] and np.array_equal(long_st["last_labels"], st["last_labels"])


def test_kmeans_sizes_the_kernel_branches_on():
    S = pc.KM_SPECS
    fam = lambda f, k: {s[k] for s in S.values() if s["family"] == f}
    assert fam("thread stride", "V") == {1023, 1024, 1025, 2049} and fam("ballot chunks", "V") == {63, 64, 65, 128, 129}
    assert fam("embedding lanes", "D") == {1, 2, 3, 63, 64, 65, 127, 128} and fam("embedding lanes", "dtype") == {"float32", "float64"}
    assert fam("cluster rounds", "K") == {1, 15, 16, 17, 33, 49, 64} and (S["rounds_k64_d128"]["D"], S["rounds_k64_d128"]["V"]) == (128, 1025)
    assert S["reseed_v40_k64"]["V"] < S["reseed_v40_k64"]["K"] == 64
    assert (S["prune_v9_k1"]["V"], S["prune_v8_k1"]["V"], S["prune_v12_k20"]["V"], S["prune_v12_k20"]["K"]) == (9, 8, 12, 20)
    assert (S["loop_max_iter_0"]["max_iter"], S["loop_max_iter_1"]["max_iter"], S["loop_large_tol"]["tol"]) == (0, 1, 1e3)
    # the ragged batch: one width, type and K; no mesh after the first starts at a multiple of 64; one mesh reseeds
    batch = [S[n] for n in pc.KM_BATCH]
    assert len(batch) >= 5 and len({(s["D"], s["K"], s["dtype"], s["max_iter"], s["tol"]) for s in batch}) == 1
    starts = np.cumsum([s["V"] for s in batch])[:-1]
    assert [s["V"] for s in batch] == [65, 1025, 9, 257, 129, 120] and np.all(starts % 64 != 0)
    assert any(len(pc.km_case(n)["want"][1]["reseeded"]) > 0 for n in pc.KM_BATCH)
    for n in pc.KM_NO_CLUSTER:
        assert pc.km_case(n)["want"][1]["n_kept"] == 0
    # what the families are for, recounted from the oracle's state
    st = pc.km_case("reseed_coincident_k40")["want"][1]
    assert {k for _, k in st["reseeded"]} >= {16, 31, 32, 39} and len(np.unique(pc.km_case("reseed_coincident_k40")["verts"], axis=0)) == 12
    m = pc.km_case("prune_8_and_9")["want"][1]["members"]
    assert sorted(m.tolist()) == [8, 9, 25, 30, 40]
    assert pc.km_case("prune_last_survives")["want"][1]["members"].tolist()[-1] == 60


def test_the_centre_sum_adds_rows_in_ascending_vertex_order():
    """ordered_sum is the documented order spelled out: a value that a pairwise or reversed sum rounds differently"""
    rows = np.array([[1.0], [2.0 ** -53], [2.0 ** -53], [-1.0]])
    assert po.ordered_sum(rows, [0, 1, 2, 3])[0] == 0.0 and po.ordered_sum(rows, [1, 2, 0, 3])[0] == 2.0 ** -52
    rng = np.random.default_rng(5)
    X, v = pc.unit_rows(rng.normal(size=(40, 4))), rng.normal(size=(40, 3))
    _, st = po.kernel_kmeans(X, v, 2, 1, 0.2, 0.0, 0)
    lab0 = po.kdist(X, v, X[st["seeds"]], v[st["seeds"]], 0.2).argmin(axis=1)
    for k in range(2):
        acc = np.zeros(3)
        for i in np.nonzero(lab0 == k)[0]:
            acc = acc + v[i]
        assert np.array_equal(st["centres_euc"][k], acc / np.sum(lab0 == k))


def test_an_empty_kept_set_is_reported_not_raised():
    c = pc.km_case("prune_v12_k20")
    labels, st = c["want"]
    assert st["n_kept"] == 0 and labels.dtype == np.int64 and np.all(labels == -1) and st["members"].sum() == 12


# ------------------------------------------------------------------------------------------------------------------- RANSAC
@pytest.mark.parametrize("name", pc.RS_NAMES)
def test_ransac_case_meets_its_conditions_in_the_oracle_alone(name):
    c = pc.rs_case(name)
    det = flat(c["want"])
    print(f"\n{name}: attempts {c['attempts']}, {len(c['meshes'])} meshes, {len(det)} problems, n_iter {c['n_iter']}, handles "
          f"{[len(d['handles']) for d in det][:12]}, refits {sum(d['refit'] for d in det)}")
    assert 1 <= c["attempts"] <= pc.ATTEMPTS and c["samples"].shape == (len(det), c["n_iter"], 3) and c["samples"].dtype == np.int32
    assert pc.RS_COND == dict(sigma_ratio=1e-3, sigma_ratio_vote=1e-3, dist_margin=1e-9, sum_gap=1e-9)
    for d in det:
        assert d["sigma_ratio_vote"] >= 1e-3 and d["dist_margin"] >= 1e-9, (name, d["label"])
        if d["R"] is not None:
            assert d["sigma_ratio"] >= 1e-3, (name, d["label"])
            assert d["refit"] or d["sum_gap"] > 1e-9, (name, d["label"], d["sum_gap"])
    assert pc.rs_property(name, c), (name, c["spec"]["prop"])
    # the same text in longdouble decides alike, and is the yardstick's other end
    ref = pc.rs_long(name)
    assert all(d["sums"].dtype == pc.LONG for d in flat(ref))
    pc.rs_discrete(name, flat(ref), c["want"])
    for a, b in zip(flat(ref), det):
        assert np.array_equal(a["inliers"], b["inliers"]) and (b["refit"] or a["by_sum"] == b["by_sum"])


def test_ransac_sizes_the_kernels_branch_on():
    S = pc.RS_SPECS
    assert pc.HANDLE_COUNTS == (4, 5, 64, 128, 129, 255, 256, 257, 512, 513, 1000)
    assert {s["n_iter"] for s in S.values() if s["family"] == "hypothesis counts"} == {1, 3, 4, 5, 7, 100}
    assert len(pc.SMALL_COUNTS) == 40 and set(pc.SMALL_COUNTS) == {5, 6, 7, 8, 9} and S["many_small"]["n_iter"] == 3
    assert set(pc.RS_FAMILIES) == {"handle counts", "hypothesis counts", "refit boundary", "late inliers", "selection", "no fit", "labels",
                                   "segment shapes", "input types"}
    det = flat(pc.rs_case("handles")["want"])
    assert [d["refit"] for d in det if len(d["handles"]) in (257, 513)] == [True, True]             # the fit kernel's second and third pass
    assert [d["refit"] for d in det if len(d["handles"]) in (512, 1000)] == [False, False]
    a, b, c, d = flat(pc.rs_case("share")["want"])
    assert [(len(x["handles"]), x["best_count"], x["refit"]) for x in (a, b, c, d)] == [(40, 14, False), (40, 15, True), (20, 7, False),
                                                                                        (20, 8, True)]
    assert 14.0 == 0.35 * 40 and not 14 > 0.35 * 40 and 7.0 == 0.35 * 20
    late = flat(pc.rs_case("late")["want"])[0]
    assert late["inliers"].min() >= 256 and late["refit"]
    m = pc.rs_case("labels")["meshes"][0]
    assert m["seg"].min() < 0 and m["seg"].max() > 2 ** 31 and m["seg"].dtype == np.int64


def test_yardsticks():
    """float64 oracle against longdouble oracle, per family: what tests/test_piecewise_differential.py multiplies by 16"""
    print("\n" + pc.table())
    for family in pc.RS_FAMILIES:
        y = pc.rs_yardstick(family)
        assert all(np.isfinite(v) for v in y.values()) and pc.rs_bounds(family) == {q: 16 * v for q, v in y.items()}
        assert max(y.values()) < 1e-9, (family, y)
    assert pc.FACTOR == 16


# ------------------------------------------------------------------------------------------------------------------- the generator
def test_the_generator_is_deterministic():
    for fn, name in ((pc.km_case, "reseed_coincident_k40"), (pc.km_case, "lanes_d65_float64"), (pc.rs_case, "share"), (pc.rs_case, "labels")):
        first = fn(name)
        fn.cache_clear()
        again = fn(name)
        assert again is not first and again["attempts"] == first["attempts"]
        if fn is pc.km_case:
            assert np.array_equal(again["X"], first["X"]) and np.array_equal(again["verts"], first["verts"]) and again["first"] == first["first"]
            assert np.array_equal(again["want"][0], first["want"][0]) and np.array_equal(again["want"][1]["centres_emb"], first["want"][1]["centres_emb"])
        else:
            assert np.array_equal(again["samples"], first["samples"])
            for a, b in zip(again["meshes"], first["meshes"]):
                assert all(np.array_equal(a[k], b[k]) for k in a)
            for a, b in zip(flat(again["want"]), flat(first["want"])):
                assert np.array_equal(a["sums"], b["sums"]) and (a["R"] is None) == (b["R"] is None)
    pc.rs_long.cache_clear()
    pc.rs_yardstick.cache_clear()


# ------------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("name", ["labels", "shapes", "no_problem", "float32", "many_small", "iter5"])
def test_ransac_packing_round_trips_through_the_host_code(ops, name):
    """the lists and sample slices of the device file through piecewise.piecewise_ransac on the emulated ops: the details come back
    problem by problem in the order of the oracle's runs and pass the device file's comparison with nothing to spare"""
    c = pc.rs_case(name)
    assert sum(len(s) for s in c["mesh_samples"]) == len(c["samples"])
    assert np.array_equal(np.concatenate([s.reshape(-1, c["n_iter"], 3) for s in c["mesh_samples"]]), c["samples"])
    details = []
    out = piecewise.piecewise_ransac(*pc.lists(c), samples=c["samples"], details=details)
    dev = pc.rs_compare("emulated ops", name, [o.numpy() for o in out], details)
    assert max(dev.values()) <= max(pc.rs_yardstick(c["spec"]["family"]).values())
    at = 0
    for i in range(len(c["meshes"])):                                          # a mesh alone takes its own slice of the samples
        alone, = piecewise.piecewise_ransac(*pc.lists(c, [i]), samples=c["mesh_samples"][i])
        assert np.array_equal(alone.numpy(), out[i].numpy())
        at += len(c["mesh_samples"][i])
    assert at == len(c["samples"])


def test_the_unfitted_problem_raises_through_the_host_code(ops):
    c = pc.rs_case("nofit")
    with pytest.raises(ValueError, match="mesh 1, label 9"):
        piecewise.piecewise_ransac(*pc.lists(c), samples=c["samples"])
    out = piecewise.piecewise_ransac(*pc.lists(c, [0, 2]), samples=np.concatenate([c["mesh_samples"][0], c["mesh_samples"][2]]))
    for o, i in zip(out, (0, 2)):                                              # the emulation moves vertex by vertex: a few ulps
        assert np.abs(o.numpy() - c["want"][i][0]).max() < 1e-14


def test_kmeans_batch_and_statuses_through_the_host_code(ops):
    cases = [pc.km_case(n) for n in pc.KM_BATCH]
    labels, states = piecewise.kernel_kmeans([c["X"] for c in cases], [c["verts"] for c in cases], n_clusters=6, first=[c["first"] for c in cases],
                                             return_state=True)
    for n, l, st in zip(pc.KM_BATCH, labels, states):
        assert pc.km_compare("emulated ops", n, l.numpy(), st) == 0.0
    for n in pc.KM_NO_CLUSTER:
        c, other = pc.km_case(n), pc.km_case("prune_v9_k1")
        if c["spec"]["K"] == 1:                                                # behind a healthy mesh: the message names mesh 1
            with pytest.raises(ValueError, match="mesh 1: no cluster keeps"):
                piecewise.kernel_kmeans([other["X"], c["X"]], [other["verts"], c["verts"]], n_clusters=1, first=[other["first"], c["first"]])
        else:
            with pytest.raises(ValueError, match="mesh 0: no cluster keeps"):
                piecewise.kernel_kmeans([c["X"]], [c["verts"]], n_clusters=c["spec"]["K"], first=[c["first"]])


# ------------------------------------------------------------------------------------------------------------------- planted errors
def oracle_as_device(name):
    """the float64 oracle's own run in the shape of the device's: it passes, and every planted error below is measured against it"""
    c = pc.rs_case(name)
    out = [np.array(o) for o, _ in c["want"]]
    det = [dict(copy.deepcopy(d), mesh=mi) for mi, (_, dd) in enumerate(c["want"]) for d in dd]
    return out, det


def test_the_ransac_comparison_rejects_planted_errors():
    name = "iter100"
    pc.rs_compare("float64 oracle", name, *oracle_as_device(name))

    def planted(change):
        out, det = oracle_as_device(name)
        change(out, det)
        with pytest.raises(AssertionError):
            pc.rs_compare("planted", name, out, det)

    def count_off_by_one(out, det):
        det[1]["counts"][7] += 1

    def perturbed_R(out, det):
        det[2]["R"][1, 2] += 1e-10

    def perturbed_t(out, det):
        det[0]["t"][0] += 1e-10

    def wrong_selection(out, det):
        det[1]["by_sum"] = (det[1]["by_sum"] + 1) % 100

    def flipped_refit(out, det):
        det[0]["refit"] = False

    def one_sum(out, det):
        det[2]["sums"][99] *= 1 + 1e-9

    def one_vertex(out, det):
        out[0][5, 1] += 1e-10

    def dropped_handle(out, det):
        det[2]["handles"] = det[2]["handles"][:-1]

    for change in (count_off_by_one, perturbed_R, perturbed_t, wrong_selection, flipped_refit, one_sum, one_vertex, dropped_handle):
        planted(change)
    # a vertex of a segment with < 4 handles that is not the target bit for bit
    out, det = oracle_as_device("shapes")
    pc.rs_compare("float64 oracle", "shapes", out, det)
    out[1][0, 0] = np.nextafter(out[1][0, 0], 1)
    with pytest.raises(AssertionError):
        pc.rs_compare("planted", "shapes", out, det)


def test_the_kmeans_comparison_rejects_planted_errors():
    name = "rounds_k17"
    labels, st = pc.km_case(name)["want"]
    pc.km_compare("float64 oracle", name, labels, st)

    def planted(change):
        l, s = labels.copy(), {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        out = change(l, s)
        with pytest.raises(AssertionError):
            pc.km_compare("planted", name, l if out is None else out, s)

    def one_label(l, s):
        l[1024] = (l[1024] + 1) % s["n_kept"]

    def one_member(l, s):
        s["members"][16] += 1

    def one_seed(l, s):
        s["seeds"][16] = s["seeds"][15]

    def one_ulp_in_a_centre(l, s):
        s["centres_emb"][16, 7] = np.nextafter(s["centres_emb"][16, 7], 2)

    def one_ulp_in_a_position(l, s):
        s["centres_euc"][0, 2] = np.nextafter(s["centres_euc"][0, 2], 9)

    def one_iteration_more(l, s):
        s["n_iter"] += 1

    def fit_past_its_bound(l, s):
        s["fit"] *= 1 + 1e-11

    for change in (one_label, one_member, one_seed, one_ulp_in_a_centre, one_ulp_in_a_position, one_iteration_more, fit_past_its_bound):
        planted(change)
