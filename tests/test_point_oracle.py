"""CPU: tests/point_oracle.py held to what already anchors the project -- the restated third-party primitives (oracle/pyg_primitives.py)
on ragged seeded clouds, the hand-computed known answers of tests/test_oracle_kat.py, the reference-made goldens that contain these
operations -- and the conditions every generated input of tests/test_point_deform_differential.py is stated to meet (near-tie cap,
weight-sum floor, sigmoid range, planted neighbours, ties), computed from the oracle alone on every run."""
import numpy as np
import pytest
import torch

import point_oracle as po
from conftest import load_golden
from helpers import data_from
from oracle import pyg_primitives as P


def _batch(ptr):
    return torch.repeat_interleave(torch.arange(len(ptr) - 1), torch.from_numpy(np.diff(ptr).astype(np.int64)))


def _clouds(counts, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, size=(sum(counts), 3)).astype(np.float32), po._ptr(counts)


# ---------------------------------------------------------------------------------------------------------------- primitives
def test_fps_equals_the_primitive_on_ragged_clouds():
    pos, ptr = _clouds([700, 33, 1, 1500, 64], 11)
    m = [int(np.ceil(0.5 * n)) for n in np.diff(ptr)]
    got = po.fps(pos, ptr, po._ptr(m))
    want = P.fps(torch.from_numpy(pos), _batch(ptr), ratio=0.5, random_start=False)
    assert np.array_equal(got, want.numpy())


def test_ball_query_equals_the_primitive():
    x, px = _clouds([900, 300, 70], 12)
    y, py = _clouds([200, 50, 9], 13)
    for r, mx in ((0.12, 64), (0.3, 16), (0.3, 1)):
        coo = po.ball_query(x, px, y, py, r, mx)
        row, col = P.radius(torch.from_numpy(x), torch.from_numpy(y), r, _batch(px), _batch(py), max_num_neighbors=mx)
        live = coo[0] >= 0
        assert np.array_equal(coo[1][live], row.numpy()) and np.array_equal(coo[0][live], col.numpy())
        assert np.array_equal(coo[0] < 0, coo[1] < 0)


def test_knn_search_and_apply_equal_the_primitives():
    x, px = _clouds([300, 1, 2500, 2], 14)
    y, py = _clouds([70, 40, 300, 5], 15)
    y[3] = x[10]                                                       # a coincident pair: the 1e-16 clamp
    feat = np.random.default_rng(16).normal(size=(len(x), 20)).astype(np.float32)
    for k in (1, 2, 3):
        idx, wgt = po.knn_search(x, px, y, py, k)
        yi, xi = P.knn(torch.from_numpy(x), torch.from_numpy(y), k, _batch(px), _batch(py))
        live = idx >= 0
        assert np.array_equal(np.nonzero(live)[0], yi.numpy()) and np.array_equal(idx[live], xi.numpy())
        assert (wgt[~live] == 0).all() and (idx[:, k:] == -1).all()
        want = P.knn_interpolate(torch.from_numpy(feat), torch.from_numpy(x), torch.from_numpy(y), _batch(px), _batch(py), k=k).numpy()
        got = po.knn_apply(feat, idx, wgt)
        # float64 against the primitive's float32: six roundings of a three-term weighted mean with positive weights
        assert (np.abs(got - want) <= 8 * 2.0 ** -24 * po.knn_apply_scale(feat, idx)).all()
    assert wgt[3, 0] == np.float32(1e16)


def test_cosine_knn_equals_the_primitive_on_separated_rows():
    c = po.cosine_case()
    y, x = torch.from_numpy(c["y"]), torch.from_numpy(c["x"])
    for k in (1, 5):
        res = po.cosine_knn(c["y"], c["ptr_y"], c["x"], c["ptr_x"], k)
        yi, xi = P.knn(x, y, k, _batch(c["ptr_x"]), _batch(c["ptr_y"]), cosine=True)
        want = np.full((len(c["y"]), k), -1, dtype=np.int32)
        slot = np.zeros(len(c["y"]), dtype=np.int64)
        for a, b in zip(yi.tolist(), xi.tolist()):
            want[a, slot[a]] = b
            slot[a] += 1
        sep = po.well_separated(res, k)
        assert np.array_equal(res.idx[sep], want[sep]) and np.array_equal(res.idx < 0, want < 0)
        # the float32 primitive, as a "device": every row passes the per-row rule
        bad, _ = po.cosine_rows_check(want, res, k, c["y"], c["x"], tau=4e-6)          # (the primitive divides by the norms again)
        assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_known_answers():
    line = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [10.0, 0, 0], [4.0, 0, 0], [5.0, 0, 0]], dtype=np.float32)
    assert po.fps(line, [0, 6], [0, 3]).tolist() == [0, 3, 5]
    assert po.fps(line, [0, 3, 6], [0, 2, 4]).tolist() == [0, 2, 3, 4]
    assert po.fps(line, [0, 3, 6], [0, 2, 4], start=[7, 2]).tolist() == [0, 2, 5, 3]            # out of range -> 0; start 2 of cloud 1
    tie = np.array([[0.0, 0, 0], [-2.0, 0, 0], [2.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [0.0, 0.5, 0]], dtype=np.float32)
    assert po.fps(tie, [0, 6], [0, 4]).tolist() == [0, 1, 2, 3]
    assert po.fps(tie[[0, 2, 1, 4, 3, 5]], [0, 6], [0, 4]).tolist() == [0, 1, 2, 3]
    x = np.array([[0.0, 0, 0], [0.5, 0, 0], [1.0, 0, 0], [0.2, 0, 0], [0.1, 0, 0]], dtype=np.float32)
    y = np.zeros((1, 3), dtype=np.float32)
    assert po.ball_query(x, [0, 5], y, [0, 1], 1.0, 3)[0].tolist() == [0, 1, 3]                # the point at exactly r is left out
    assert po.ball_query(x, [0, 5], y, [0, 1], 1.0, 6)[0].tolist() == [0, 1, 3, 4, -1, -1]
    coo, cnt = po.radius_sample(x, y, 1.0, 6, 0)
    assert coo[0].tolist() == [0, 1, 2, 3, 4, -1] and cnt.tolist() == [5]                       # inclusive
    far = [[0.9, 0.0, 0.0]] * 3 + [[0.0, 0.9, 0.0]] * 3 + [[1.0, 0.0, 0.0]] + [[0.1, 0.0, 0.0], [0.0, 0.1, 0.0]] * 32
    assert po.ball_query(np.array(far, dtype=np.float32), [0, 71], y, [0, 1], 1.0, 64)[0].tolist() == [0, 1, 2, 3, 4, 5] + list(range(7, 65))
    px = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0]], dtype=np.float32)
    py = np.array([[1.0, 0, 0], [2.0, 0, 0]], dtype=np.float32)
    idx, wgt = po.knn_search(px, [0, 3], py, [0, 2], 2)
    assert idx.tolist() == [[1, 0, -1], [1, 2, -1]] and wgt.tolist() == [[float(np.float32(1e16)), 1.0, 0.0], [1.0, 1.0, 0.0]]
    out = po.knn_apply(np.array([[10.0], [20.0], [40.0]], dtype=np.float32), idx, wgt)
    assert abs(out[0, 0] - 20.0) < 1e-12 and out[1, 0] == 30.0
    cx = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.05]])
    cy = np.array([[2.0, 0.1], [0.1, 3.0], [5.0, 0.0]])
    cx, cy = cx / np.linalg.norm(cx, axis=1, keepdims=True), cy / np.linalg.norm(cy, axis=1, keepdims=True)
    assert po.cosine_knn(cy, [0, 2, 3], cx, [0, 3, 4], 1).idx[:, 0].tolist() == [0, 1, 3]
    assert po.gather_rows(np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([1, -1, 0])).tolist() == [[3.0, 4.0], [0.0, 0.0], [1.0, 2.0]]
    s, rng = po.sigmoid_minmax(np.array([0.0, 0.0, np.log(3.0), 5.0, 5.0, 7.0]), [0, 3, 5, 5, 6])
    assert s[:3].tolist() == [0.0, 0.0, 1.0] and np.isnan(s[3:]).all() and rng[1] == 0.0


def test_radius_sample_against_the_reference_made_fixture():
    meta, a = load_golden("radius_cpu_kat")
    x, y = a["x"].numpy(), a["y"].numpy()
    coo, cnt = po.radius_sample(x, y, meta["r_exact"], meta["max_exact"], 5)
    live = coo[0] >= 0
    assert np.array_equal(np.stack([coo[0][live], coo[1][live]]), a["edges_exact"].numpy())
    mx = meta["max_over"]
    for seed in (1, 2):
        coo, cnt = po.radius_sample(x, y, meta["r_over"], mx, seed)
        assert np.array_equal(cnt, a["counts_over"].numpy())
        tab = coo[0].reshape(-1, mx)
        d = np.linalg.norm(y[:, None, :].astype(np.float64) - x[None].astype(np.float64), axis=-1)
        for k in range(len(y)):
            kept = tab[k][tab[k] >= 0]
            assert len(kept) == min(mx, cnt[k]) == len(set(kept.tolist())) and (d[k, kept] <= meta["r_over"] + 1e-6).all()
            if cnt[k] <= mx:
                assert kept.tolist() == np.nonzero(d[k] <= meta["r_over"] + 1e-9)[0].tolist()[:len(kept)]
    # the reservoir is uniform: over many rows and seeds every hit of an over-full row is kept about max / hits of the time
    x1 = np.zeros((40, 3), dtype=np.float32)
    y1 = np.zeros((2000, 3), dtype=np.float32)
    coo, _ = po.radius_sample(x1, y1, 0.5, 8, 77)
    freq = np.bincount(coo[0], minlength=40) / 2000.0
    assert np.abs(freq - 0.2).max() < 0.04                              # 8 of 40; standard deviation 0.009


# ---------------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", ["deformnet_ragged", "deformnet_three"])
def test_votes_reproduce_the_reference_made_deformnet_output(name):
    """the stored intermediates (features, normalised mask, positions) through the oracle's two k-NN calls and two votes, then through
    the pinned GCNDeform: the reference's own pred_flow"""
    from morig_amd import synth
    from oracle import nets
    meta, a = load_golden(name)
    m = synth.load_recipe(getattr(nets, meta["arch"])(**meta["kwargs"]).eval(), meta["recipe_seed"], mild=meta.get("mild", False))
    d = data_from(a)
    f, pf, vis = a["vtx_feature"].numpy(), a["pts_feature"].numpy(), a["pred_vismask"].numpy()
    ptr = po._ptr(np.bincount(a["batch"].numpy()))
    pptr = po._ptr(np.bincount(a["pts_batch"].numpy()))
    k = meta["kwargs"]["num_interp"]
    to_pts = po.cosine_knn(f, ptr, pf, pptr, k)
    l1 = np.full((len(f), 4), np.nan)
    l1, rows, wsum, _ = po.flow_vote(0, to_pts.idx, f, pf, a["pos"].numpy(), a["pts"].numpy(), vis, l1)
    to_vis = po.cosine_knn(f, ptr, f, ptr, k, vis=vis, split=True)
    l1, rows1, _, _ = po.flow_vote(1, to_vis.idx, f, f, None, None, vis, l1)
    assert np.array_equal(rows1, vis.reshape(-1) < 0.5) and (to_vis.idx[~rows1] == -1).all()
    # the mask is the reference's sigmoid_minmax result: 0 and 1 in every mesh
    for b in range(len(ptr) - 1):
        assert vis[ptr[b]:ptr[b + 1]].min() == 0.0 and vis[ptr[b]:ptr[b + 1]].max() == 1.0
    pred = m.completing(d.vtx, torch.from_numpy(l1).float(), d.geo_edge_index, d.tpl_edge_index, d.vtx_batch)
    assert float((pred - a["out_pred_flow"]).abs().max()) <= 2e-5


def test_cosine_nn_on_the_corrnet_golden():
    meta, a = load_golden("corrnet_ragged")
    ov, op = a["out_vtx"].numpy(), a["out_pts"].numpy()
    ptr, pptr = po._ptr(np.bincount(a["batch"].numpy())), po._ptr(np.bincount(a["pts_batch"].numpy()))
    nn, sim, res = po.cosine_nn(ov, ptr, op, pptr)
    yi, xi = P.knn(a["out_pts"], a["out_vtx"], 1, a["pts_batch"], a["batch"], cosine=True)
    sep = po.well_separated(res, 1)
    assert sep.mean() >= 0.98 and np.array_equal(nn[sep], xi.numpy()[sep])
    assert np.abs(sim - (ov.astype(np.float64) * op[nn].astype(np.float64)).sum(1)).max() == 0.0


# ---------------------------------------------------------------------------------------------------------------- generated inputs
def test_fps_inputs_meet_their_conditions():
    cases = po.fps_cases()
    sizes = {c["max_n"] for c in cases.values()}
    assert set(po.FPS_SIZES) <= sizes and max(sizes) == 32768
    assert {c["pos"].shape[1] for c in cases.values()} == {3, 4, 7}
    for name, share in (("lattice_8192", 0.9), ("lattice_shuffled", 0.9), ("lattice_old_arm", 0.8)):
        c = cases[name]
        ties, steps = po.fps_tie_steps(c["pos"], c["ptr"], c["out_ptr"])
        print(f"{name}: {ties} of {steps} arg-max steps tie")
        assert ties >= share * steps                                    # "ties at almost every step"
    a, b = cases["lattice_8192"]["pos"], cases["lattice_shuffled"]["pos"]
    assert sorted(map(tuple, a[:, :3].tolist())) == sorted(map(tuple, b[:, :3].tolist())) and not np.array_equal(a[:, :3], b[:, :3])
    assert (np.ptp(cases["coincident"]["pos"][:, :3], axis=0) == 0).all()
    assert np.ptp(cases["plane"]["pos"][:, 2]) == 0 and (np.ptp(cases["line"]["pos"][:, 1:3], axis=0) == 0).all()
    assert cases["far_negative"]["pos"][:, :3].max() < -900
    nb = cases["near_bound"]["pos"]
    d_start, d_far = po.sqdist32(nb[128, :3], nb[0, :3]), po.sqdist32(nb[128, :3], nb[256, :3])
    assert 0.999 * d_start <= d_far < po.sqdist32(nb[384, :3], nb[0, :3]) < d_start          # an update that lowers a bucket's maximum by < 0.1 %
    assert po.fps(nb, [0, 512], [0, 4]).tolist() == [0, 256, 384, 128]                        # ... decides the third sample
    s = cases["starts"]
    n = np.diff(s["ptr"])
    assert ((s["start"] < 0) | (s["start"] >= n)).sum() == 2 and ((s["start"] > 0) & (s["start"] < n)).sum() == 2
    e = cases["empty_members"]
    assert 0 in np.diff(e["ptr"]).tolist() and 0 in np.diff(e["out_ptr"]).tolist()
    out = po.fps(e["pos"], e["ptr"], e["out_ptr"], fill=-7)
    assert (out[50:54] == -7).all() and (out[:50] >= 0).all() and (out[54:] >= 350).all()
    # clustered: 12 clusters far narrower than their spacing
    c = cases["clustered_8192"]["pos"][:, :3].astype(np.float64)
    got = po.fps(cases["clustered_8192"]["pos"], [0, 8192], [0, 12])
    d = np.linalg.norm(c[:, None, :] - c[got][None], axis=-1).min(1)
    assert d.max() < 0.03                                              # the first 12 samples are one per cluster: every point is near one


def test_ball_radius_knn_gather_inputs_meet_their_conditions():
    b = po.ball_case()
    assert np.diff(b["ptr_y"]).tolist().count(0) == 1 and np.diff(b["ptr_x"]).tolist().count(0) == 2
    assert b["x"].shape[1] != b["y"].shape[1]
    assert po.sqdist32(b["x"][330, :3], b["y"][48, :3]) == po.r2_of(0.25)                      # a point at exactly r
    for r in b["radii"]:
        coo = po.ball_query(b["x"], b["ptr_x"], b["y"], b["ptr_y"], r, 130).reshape(2, -1, 130)
        cnt = (coo[0] >= 0).sum(1)
        assert coo[0][40].tolist()[:2] == [322, -1]                    # 193 = 64 * 3 + 1 points, the hit in the last lane-step
        assert (330 in coo[0][48].tolist()) == (r == 0.5)
        assert (cnt[45:48] == 0).all()                                 # centres facing an empty point cloud
        print(f"ball r={r}: hits per centre min {cnt.min()} max {cnt.max()}")
    assert cnt.max() == 130 and cnt.min() == 0
    rc = po.radius_case()
    _, cnt = po.radius_sample(rc["x"], rc["y"], 0.3, 64, 0)
    assert (cnt > 64).sum() >= 20 and ((cnt > 0) & (cnt < 64)).sum() >= 20 and (cnt[10:13] == 0).all() and cnt[13] == 1
    assert po.sqdist32(rc["x"][20, :3], rc["y"][13, :3]) == po.r2_of(0.25)                     # inclusive: a hit at exactly r
    kc = po.knn_case()
    idx, wgt = po.knn_search(kc["x"], kc["ptr_x"], kc["y"], kc["ptr_y"], 3)
    assert sorted(kc["planted"]) == [3, 4, 5, 6]
    for c, spots in kc["planted"].items():
        ys = int(kc["ptr_y"][c])
        for t in range(min(3, len(spots))):
            assert idx[ys + t, 0] == spots[t]                          # the nearest source of target t sits ON the planted position
        assert set(spots) <= set(idx[ys:ys + 3].reshape(-1).tolist())
        assert wgt[ys + 3, 0] == np.float32(1e16)                      # the coincident pair
        xs = int(kc["ptr_x"][c])
        assert idx[ys + 4, :2].tolist() == [xs + 40, xs + 600] and wgt[ys + 4, 0] == wgt[ys + 4, 1]
        d5 = po.sqdist32(kc["x"][xs:int(kc["ptr_x"][c + 1]), :3], kc["y"][ys + 5, :3])
        assert idx[ys + 5].tolist() == [xs + 60, xs + 61, xs + 50] and d5[50] == d5[700] and np.sort(d5)[1] < d5[50] == np.sort(d5)[3]
    assert kc["planted"][6][-1] == int(kc["ptr_x"][7]) - 1 and (2049 % 2) == 1                 # the odd tail holds a nearest neighbour
    assert (idx[:255, 1:] == -1).all() and (idx[255:511, 2] == -1).all()                       # fewer than k sources
    g = po.gather_case()
    assert len(g["idx"]) * g["cols"] > 4096 * 256 and (g["idx"] == -1).sum() > 1000


@pytest.mark.parametrize("k", range(1, 9))
def test_cosine_inputs_stay_under_the_near_tie_cap(k):
    """Condition, not measurement: at most 2 % of the rows of a generated case are not well separated (gaps of 2 tau among the first
    min(k, n_live) + 1 similarities); unit Gaussian 64-d rows measure 0.3 .. 0.5 %"""
    c = po.cosine_case()
    res = po.cosine_knn(c["y"], c["ptr_y"], c["x"], c["ptr_x"], k)
    s = po.split_case()
    res2 = po.cosine_knn(s["f"], s["ptr"], s["f"], s["ptr"], k, vis=s["vis"], split=True)
    print(f"k={k}: near-tie share all-rows {po.near_tie_share(res, k):.4f} split {po.near_tie_share(res2, k):.4f}")
    assert po.near_tie_share(res, k) <= 0.02 and po.near_tie_share(res2, k) <= 0.02
    # the oracle's own lists pass the per-row rule, duplicates included
    assert po.cosine_rows_check(res.idx, res, k, c["y"], c["x"], c["dup_group"])[0] == []
    assert po.cosine_rows_check(res2.idx, res2, k, s["f"], s["f"], s["dup_group"])[0] == []
    q = int(c["ptr_y"][6]) + 3
    xs = int(c["ptr_x"][6])
    assert res.idx[q, :min(k, 6)].tolist() == [xs + d for d in po.DUPES[:k]]
    # nine equal candidates in one lane's share of one tile: more than any K, so the first K by index are the answer
    assert all(d // 32 == 4 and d % 8 < 4 for d in po.LANE_DUPES) and len(po.LANE_DUPES) == 9
    assert res.idx[int(c["ptr_y"][9]) + 5].tolist() == [int(c["ptr_x"][9]) + d for d in po.LANE_DUPES[:k]]
    assert res2.idx[int(s["ptr"][7]) + 5].tolist() == [int(s["ptr"][7]) + d for d in po.LANE_DUPES[:k]]
    q = int(s["ptr"][7]) + 3
    assert res2.idx[q, :min(k, 6)].tolist() == [int(s["ptr"][7]) + d for d in po.DUPES[:k]]
    assert (res.idx[c["ptr_y"][8]:c["ptr_y"][9]] == -1).all()          # an empty candidate cloud
    assert (res2.idx[s["ptr"][9]:s["ptr"][10]] == -1).all() and (res2.idx[s["ptr"][10]:s["ptr"][11]] == -1).all() and (res2.idx[0] == -1).all()


def test_cosine_rule_rejects_wrong_lists():
    """the rule itself: a swapped well-separated pair, a duplicate out of order, a foreign cloud and a wrong padding are all reported"""
    c = po.cosine_case()
    k = 5
    res = po.cosine_knn(c["y"], c["ptr_y"], c["x"], c["ptr_x"], k)
    sep = po.well_separated(res, k)
    q = int(np.nonzero(sep & (res.idx[:, k - 1] >= 0))[0][0])
    for edit in ("swap", "dupe", "foreign", "pad"):
        g = res.idx.copy()
        if edit == "swap":
            g[q, [0, 1]] = g[q, [1, 0]]
        elif edit == "dupe":
            q2 = int(c["ptr_y"][6]) + 3
            g[q2, [0, 1]] = g[q2, [1, 0]]
        elif edit == "foreign":
            g[q, 0] = (res.hi[q]) % len(c["x"])
        else:
            g[q, k - 1] = -1
        assert po.cosine_rows_check(g, res, k, c["y"], c["x"], c["dup_group"])[0], edit


@pytest.mark.parametrize("n", [255, 256, 257])
def test_flow_inputs_keep_the_weight_sums_away_from_zero(n):
    c = po.flow_case(n)
    vis = c["vis"].reshape(-1)
    for k in (1, 5, 8):
        idx = po.punch_holes(po.cosine_knn(c["f"], c["ptr"], c["pf"], c["pptr"], k).idx)
        l1, rows, wsum, vsum = po.flow_vote(0, idx, c["f"], c["pf"], c["pos"], c["ppos"], c["vis"], np.full((n, 4), np.nan))
        nan = np.isnan(l1[:, 0])
        assert np.array_equal(nan, vis == 0) and nan.sum() >= 10 and (np.abs(wsum[~nan]) >= 1e-2).all()
        if k >= 3:
            assert ((idx[:, 1] == -1) & (idx[:, 2] >= 0)).any()         # -1 inside a list
        if k > 3:
            assert (idx[c["ptr"][2]:, 3:] == -1).all() and (idx[c["ptr"][2]:, 0] >= 0).all()     # the 3-point cloud pads
        idx2 = po.cosine_knn(c["f"], c["ptr"], c["f"], c["ptr"], k, vis=c["vis"], split=True).idx
        l2, rows2, wsum2, _ = po.flow_vote(1, idx2, c["f"], c["f"], None, None, c["vis"], l1)
        hidden = vis < 0.5
        assert np.array_equal(rows2, hidden) and np.array_equal(l2[~hidden], l1[~hidden], equal_nan=True)
        no_seen = np.arange(n) >= c["ptr"][2]
        assert hidden[no_seen].all() and np.isnan(l2[no_seen, :3]).all()                       # a mesh without a visible vertex
        cmp = hidden & ~no_seen
        assert (np.abs(wsum2[cmp]) >= 1e-2).all() and cmp.sum() >= 40


def test_sigmoid_inputs_meet_their_conditions():
    c = po.sigmoid_case()
    out, rng = po.sigmoid_minmax(c["x"][:, 1], c["ptr"])
    sizes = np.diff(c["ptr"]).tolist()
    assert sizes == po.SIG_N and sizes[3] == 0 and np.abs(c["x"][:, 1]).max() <= 30.0
    for b, n in enumerate(sizes):
        seg = out[c["ptr"][b]:c["ptr"][b + 1]]
        if b in (0, 7):
            assert np.isnan(seg).all() and rng[b] == 0.0               # one vertex; a constant mesh
        elif n:
            assert rng[b] >= 0.1 and seg.min() == 0.0 and seg.max() == 1.0
    m = c["x"][c["ptr"][4]:c["ptr"][5], 1]
    assert int(np.argmin(m)) == 200 and int(np.argmax(m)) == 250 and np.sort(m)[1] >= -2.0     # the minimum belongs to the fourth wave alone
