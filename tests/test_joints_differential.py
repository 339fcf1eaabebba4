"""csrc/joints.hip on the device at the sizes its kernels branch on: the cases of tests/joints_cases.py (their conditions are asserted
on the CPU by tests/test_joints_cases.py) through ``get_ops()``, through morig_amd/joints.py, and through the C entry points where the
caller owns a workspace (the per-row ``kth_ws`` of the bandwidth, ``counts``, ``alive``: prefilled with a sentinel, with guard rows behind
the last mesh). Bars, from joints_cases' docstring: k-th distances, counts, survivors, inside masks and the lattice mean-shift step are
compared bit for bit with the numpy restatements; the bandwidth is within n * 2^-53 of the correctly rounded mean; generic mean-shift
modes are within 1e-11 of the restatement, and bit-equal between a mesh alone and the mesh in its batch. Figures are printed before they
are asserted (run with -s). Every restated result is computed once per process and shared.

Not covered: MORIG_KTH_ROWS=1: the switch is read once per process, so a test cannot reach it without a child process. The one-row selection kernel is reached
instead by passing max_n = 65536 to the batched entry point."""
import functools
import time
import types

import numpy as np
import pytest
import torch

import joints_cases as jc
from morig_amd import joints as J
from morig_amd.native import _p, _stream, check
from morig_amd.runtime import get_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 5                                                    # rows behind the last mesh that nothing may write
KTH_SENTINEL, COUNT_SENTINEL, ALIVE_SENTINEL = -7.0, -77, 0xAB


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))                       # a copy: the tables' arrays are read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def cat_pts(sets):
    return dev(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in sets]))


def ptr_dev(sets):
    return dev(jc.ptr_of([len(x) for x in sets]))


def split(a, sets):
    p = jc.ptr_of([len(x) for x in sets])
    return [a[p[b]:p[b + 1]] for b in range(len(sets))]


@functools.lru_cache(maxsize=None)
def want_kth(name, k):
    c = CASES[name]
    return jc.kth_distances(c["x"], k, c.get("rows"))


CASES = {c["name"]: c for c in jc.select_cases()}
for _b, _x in enumerate(jc.select_ragged()["sets"]):
    CASES[f"ragged{_b}"] = dict(name=f"ragged{_b}", x=_x, rows=None)


# ------------------------------------------------------------------------------------------------------------------ selection
def kth_one_set(x, k):
    """morig_knn_bandwidth: the one-set launch with a given k -> (per-row k-th distances, bandwidth)"""
    P = dev(x)
    ws = torch.full((len(x) + GUARD,), KTH_SENTINEL, dtype=torch.float64, device=DEV)
    bw = torch.empty(1, dtype=torch.float64, device=DEV)
    check(get_ops().lib.morig_knn_bandwidth(_p(P), len(x), k, _p(ws), _p(bw), _stream()), "morig_knn_bandwidth")
    ws = host(ws)
    assert (ws[len(x):] == KTH_SENTINEL).all()
    return ws[:len(x)], float(bw.item())


def kth_batched(sets, q, max_n):
    """morig_knn_bandwidth_batched -> (per-row k-th distances of every mesh, bandwidths); max_n = 65536 launches the one-row kernel"""
    P, ptr = cat_pts(sets), ptr_dev(sets)
    n = P.shape[0]
    ws = torch.full((n + GUARD,), KTH_SENTINEL, dtype=torch.float64, device=DEV)
    bw = torch.full((len(sets),), KTH_SENTINEL, dtype=torch.float64, device=DEV)
    check(get_ops().lib.morig_knn_bandwidth_batched(_p(P), _p(ptr), len(sets), n, max_n, float(q), _p(ws), _p(bw), _stream()),
          "morig_knn_bandwidth_batched")
    ws = host(ws)
    assert (ws[n:] == KTH_SENTINEL).all(), "written behind the last mesh"
    return split(ws[:n], sets), host(bw)


def check_kth(name, k, kth, bw, what):
    c = CASES[name]
    want = want_kth(name, k)
    got = kth if c.get("rows") is None else kth[c["rows"]]
    assert jc.same_bits(got, want), (name, what, k, np.flatnonzero(got != want)[:8])
    mean, bound = jc.bandwidth_bound(kth)                     # every row of kth, the checked ones bit-equal to the restatement
    print(f"{name} {what} k={k}: {len(want)} rows bit-equal, bandwidth {bw!r} against {mean!r}: off by {abs(bw - mean):.3e}, bound {bound:.3e}")
    assert abs(bw - mean) <= bound, (name, what, k)


@pytest.mark.parametrize("name", [c["name"] for c in jc.select_cases()])
def test_kth_distances_are_exact_through_every_launch(name):
    """per-row k-th distances bit-equal to kth_distances and the bandwidth within n * 2^-53 of their correctly rounded mean: the one-set
    launch with a given k, the batched launch with max_n = n (kth_nn4_kernel) and with max_n = 65536 (kth_nn_kernel<true>). full16, the
    65 535-point set, is checked on rows 0..7 and every 977th."""
    c = CASES[name]
    n, t0 = len(c["x"]), time.time()
    for k in c["ks"]:
        kth, bw = kth_one_set(c["x"], k)
        check_kth(name, k, kth, bw, "one set")
    for q in c["qs"]:
        for max_n in (n, c["max_n_one_row"]):
            (kth,), bws = kth_batched([c["x"]], q, max_n)
            check_kth(name, jc.k_of(n, q), kth, float(bws[0]), "four rows" if max_n == n else "one row")
    print(f"{name}: {time.time() - t0:.2f} s")


def test_a_set_alone_gives_the_bits_it_gives_in_the_batch():
    """every set of at most 513 points and the ragged sizes (0, 1, 4, 0, 5, 3, 0) as ONE batch: per mesh the restated distances, the
    bits of the set alone, 0.0 as the bandwidth of an empty mesh, nothing written behind the last mesh"""
    names = [c["name"] for c in jc.select_cases() if len(c["x"]) <= 513]
    sets = [CASES[m]["x"] for m in names[:6]] + list(jc.select_ragged()["sets"]) + [CASES[m]["x"] for m in names[6:]]
    names = names[:6] + [f"ragged{b}" for b in range(len(jc.SELECT_RAGGED))] + names[6:]
    for q in jc.select_ragged()["qs"]:
        for max_n in (max(len(x) for x in sets), jc.ONE_ROW_MAX_N):
            per, bws = kth_batched(sets, q, max_n)
            for name, x, kth, bw in zip(names, sets, per, bws):
                if len(x) == 0:
                    assert bw == 0.0 and len(kth) == 0
                    continue
                assert jc.same_bits(kth, want_kth(name, jc.k_of(len(x), q))), (name, q, max_n)
                (alone,), bw_alone = kth_batched([x], q, max_n if max_n == jc.ONE_ROW_MAX_N else len(x))
                assert jc.same_bits(alone, kth) and bw_alone[0] == bw, (name, q, max_n)
    r = jc.select_ragged()
    for q in r["qs"]:
        for max_n in (max(r["sizes"]), jc.ONE_ROW_MAX_N):
            per, bws = kth_batched(r["sets"], q, max_n)
            via_ops = host(get_ops().knn_bandwidth_batched(cat_pts(r["sets"]), ptr_dev(r["sets"]), max_n, q))
            assert jc.same_bits(via_ops, bws)
            for b, (x, kth) in enumerate(zip(r["sets"], per)):
                assert len(x) == 0 or jc.same_bits(kth, want_kth(f"ragged{b}", jc.k_of(len(x), q)))
    for name in ("n5", "tie64", "mixed"):                                      # the public one-set wrappers give the raw launch's bandwidth
        c = CASES[name]
        k = c["ks"][-1]
        assert float(get_ops().knn_bandwidth(dev(c["x"]), k).item()) == kth_one_set(c["x"], k)[1]
    x = CASES["n257"]["x"]
    assert float(J.estimate_bandwidth(dev(x), 0.04).item()) == kth_one_set(x, jc.k_of(257, 0.04))[1]


# --------------------------------------------------------------------------------------------------------------------- counts
def counts_batched(sets, hs):
    """morig_nms_counts_batched into a prefilled buffer with guard rows"""
    P, ptr, bw = cat_pts(sets), ptr_dev(sets), dev(np.asarray(hs, dtype=np.float64))
    n = P.shape[0]
    out = torch.full((n + GUARD,), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    check(get_ops().lib.morig_nms_counts_batched(_p(P), _p(ptr), len(sets), n, max(max(len(x) for x in sets), 1), _p(bw), _p(out), _stream()),
          "morig_nms_counts_batched")
    out = host(out)
    assert (out[n:] == COUNT_SENTINEL).all(), "written behind the last mesh"
    return split(out[:n], sets)


def counts_sorted(sets, hs):
    """morig_nms_counts_sorted on the Morton-sorted points, as the product sorts them (morig_morton_keys + a stable argsort)"""
    P, ptr, bw = cat_pts(sets), ptr_dev(sets), dev(np.asarray(hs, dtype=np.float64))
    n, max_n = P.shape[0], max(max(len(x) for x in sets), 1)
    ops = get_ops()
    keys = torch.empty(n, dtype=torch.int64, device=DEV)
    check(ops.lib.morig_morton_keys(_p(P), _p(ptr), len(sets), n, _p(keys), _stream()), "morig_morton_keys")
    mesh_of = np.repeat(np.arange(len(sets)), [len(x) for x in sets])
    assert np.array_equal(host(keys) >> 30, mesh_of), "segment_of: the mesh bits of the Morton keys"
    perm = torch.argsort(keys, stable=True)
    Ps = P[perm].contiguous()
    bbox = torch.empty(len(sets) * ((max_n + 31) // 32) * 6, dtype=torch.float64, device=DEV)
    cs = torch.full((n + GUARD,), COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    check(ops.lib.morig_nms_counts_sorted(_p(Ps), _p(ptr), len(sets), n, max_n, _p(bw), _p(bbox), _p(cs), _stream()), "morig_nms_counts_sorted")
    assert bool((cs[n:] == COUNT_SENTINEL).all()), "written behind the last mesh"
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    out[perm] = cs[:n]
    return split(host(out), sets)


@pytest.mark.parametrize("k", range(len(jc.COUNT_SIZES)), ids=lambda k: f"n{jc.COUNT_SIZES[k]}")
def test_counts_equal_the_rooted_compare(k):
    """nms_counts, nms_counts_batched and morig_nms_counts_sorted at a rooted distance that occurs, one ulp below, one ulp above, and 0.0"""
    c = jc.count_cases()[k]
    for h in c["hs"]:
        want = jc.counts(c["x"], h).astype(np.int32)
        plain = host(get_ops().nms_counts(dev(c["x"]), dev(np.array([h]))))
        (batched,), (srt,) = counts_batched([c["x"]], [h]), counts_sorted([c["x"]], [h])
        via_ops = host(get_ops().nms_counts_batched(dev(c["x"]), ptr_dev([c["x"]]), len(c["x"]), dev(np.array([h]))))
        print(f"{c['name']} h={h!r}: row 0 counts {int(want[0])}, device {int(plain[0])} / {int(batched[0])} / {int(srt[0])}")
        assert jc.same_bits(plain, want) and jc.same_bits(batched, want) and jc.same_bits(srt, want) and jc.same_bits(via_ops, want), (c["name"], h)


def test_counts_of_a_ragged_batch():
    """(0, 1, 32, 0, 33, 31, 0) with a bandwidth per mesh, the four kinds of bandwidth in turn"""
    r = jc.count_ragged()
    for hs in r["hs"]:
        want = [jc.counts(x, h).astype(np.int32) for x, h in zip(r["sets"], hs)]
        for got in (counts_batched(r["sets"], hs), counts_sorted(r["sets"], hs)):
            assert all(jc.same_bits(g, w) for g, w in zip(got, want)), hs


# --------------------------------------------------------------------------------------------------------------------- greedy
@functools.lru_cache(maxsize=None)
def want_alive(name, order):
    c = greedy_table()[name]
    return jc.greedy(c["x"], c["attn"], c["h"], c["orders"][order], c["thrd_density"], c["thrd_attn"])


@functools.lru_cache(maxsize=None)
def greedy_table():
    return {c["name"]: c for c in list(jc.greedy_cases()) + list(jc.greedy_ragged()["meshes"])}


def greedy_one(c, order):
    got = get_ops().nms_greedy(dev(c["x"]), dev(c["attn"]), dev(np.array([c["h"]])), dev(order, torch.int32), c["thrd_density"], c["thrd_attn"])
    return host(got)


@pytest.mark.parametrize("name", jc.GREEDY_NAMES)
def test_greedy_survivors_for_every_order(name):
    c = greedy_table()[name]
    for kind, order in c["orders"].items():
        want = want_alive(name, kind)
        got = greedy_one(c, order)
        print(f"{name} order {kind}: {int(want.sum())} survivors, device {int(got.sum())}")
        assert np.array_equal(got, want), (name, kind)
    if name == "n1025":                                                        # the reference-named function visits in numpy's order
        kept = J.nms_meanshift(dev(c["x"]), dev(c["attn"]), c["h"], c["thrd_density"])
        assert jc.same_bits(host(kept), c["x"][want_alive(name, "nms")])


def test_greedy_of_a_ragged_batch():
    """(0, 1, 64, 0, 1025, 63, 0), per-mesh bandwidths: nms_greedy_batched equals the restatement and each mesh alone; `alive` is
    written only inside the meshes' own rows"""
    r = jc.greedy_ragged()
    ms = r["meshes"]
    sets = [m["x"] for m in ms]
    P, ptr, bw = cat_pts(sets), ptr_dev(sets), dev(np.array([m["h"] for m in ms]))
    A = dev(np.concatenate([m["attn"] for m in ms]))
    n = P.shape[0]
    for kind in ("nms", "perm", "rev"):
        order = dev(np.concatenate([m["orders"][kind] for m in ms]), torch.int32)
        alive = torch.full((n + GUARD,), ALIVE_SENTINEL, dtype=torch.uint8, device=DEV)
        check(get_ops().lib.morig_nms_greedy_batched(_p(P), _p(A), _p(ptr), len(ms), n, _p(bw), _p(order), r["thrd_density"], r["thrd_attn"],
                                                     _p(alive), _stream()), "morig_nms_greedy_batched")
        alive = host(alive)
        assert (alive[n:] == ALIVE_SENTINEL).all() and set(np.unique(alive[:n]).tolist()) <= {0, 1}
        via_ops = host(get_ops().nms_greedy_batched(P, A, ptr, bw, order, r["thrd_density"], r["thrd_attn"]))
        assert np.array_equal(via_ops, alive[:n].astype(bool))
        for m, got in zip(ms, split(alive[:n].astype(bool), sets)):
            if len(m["x"]):
                assert np.array_equal(got, want_alive(m["name"], kind)), (m["name"], kind)
                assert np.array_equal(got, greedy_one(m, m["orders"][kind])), (m["name"], kind)


# ----------------------------------------------------------------------------------------------------------------- mean-shift
def ms_inputs(meshes):
    sets = [m["x"] for m in meshes]
    W = None if meshes[0]["w"] is None else dev(np.concatenate([m["w"] for m in meshes]))
    return cat_pts(sets), W, ptr_dev(sets), max(max(len(x) for x in sets), 1), dev(np.array([m["h"] for m in meshes], dtype=np.float64))


def ms_plain(m, it):
    return host(get_ops().meanshift(dev(m["x"]), None if m["w"] is None else dev(m["w"]), dev(np.array([m["h"]])), it))


def ms_batched(meshes, it):
    P, W, ptr, max_n, bw = ms_inputs(meshes)
    return split(host(get_ops().meanshift_batched(P, W, ptr, max_n, bw, it)), [m["x"] for m in meshes])


def ms_sorted(meshes, it):
    """-> (modes per mesh, counts per mesh, the counts nms_counts_batched gives for those modes)"""
    P, W, ptr, max_n, bw = ms_inputs(meshes)
    modes, cnt = get_ops().meanshift_batched_sorted(P, W, ptr, max_n, bw, it, with_counts=True)
    assert jc.same_bits(host(get_ops().meanshift_batched_sorted(P, W, ptr, max_n, bw, it)), host(modes)), "a second run"
    want_cnt = get_ops().nms_counts_batched(modes, ptr, max_n, bw)
    sets = [m["x"] for m in meshes]
    return split(host(modes), sets), split(host(cnt), sets), split(host(want_cnt), sets)


@pytest.mark.parametrize("k", range(len(jc.SMALL_SIZES) + 2), ids=lambda k: jc.lattice_cases()[k]["name"])
def test_lattice_step_is_bit_equal_on_every_path(k):
    """one step on the exact lattice: meanshift, meanshift_batched and meanshift_batched_sorted against meanshift_step, bit for bit"""
    c = jc.lattice_cases()[k]
    want = jc.meanshift_step(c["x"], c["w"], c["h"])
    plain, (batched,) = ms_plain(c, 2), ms_batched([c], 2)
    (srt,), (cnt,), (want_cnt,) = ms_sorted([c], 2)
    print(f"{c['name']}: moved by up to {np.abs(want - c['x']).max():.3e}; differing values: plain {int((plain != want).sum())}, "
          f"batched {int((batched != want).sum())}, sorted {int((srt != want).sum())}")
    assert jc.same_bits(plain, want) and jc.same_bits(batched, want) and jc.same_bits(srt, want)
    assert jc.same_bits(cnt, want_cnt) and (len(want) > 513 or jc.same_bits(cnt.astype(np.int64), jc.counts(want, c["h"])))


@pytest.mark.parametrize("name", jc.GENERIC_NAMES)
def test_generic_meanshift_on_every_path(name):
    """clustered sets with weights: the three paths within 1e-11 of the restatement; the batch bit-equal to every mesh alone (the mesh
    of stop_pair that converged early included, while its neighbour ran all steps); the sorted path bit-equal to itself alone and to a
    second run; its counts those of nms_counts_batched on the modes it returned; max_iter = 1 returns the input bits"""
    c = jc.generic_case(name)
    ms = c["meshes"]
    live = [b for b, m in enumerate(ms) if len(m["x"])]
    for it in c["max_iters"]:
        want = [jc.modes_at(m, it) for m in ms]
        batched = ms_batched(ms, it)
        srt, cnt, want_cnt = ms_sorted(ms, it)
        alone = {b: ms_plain(ms[b], it) for b in live}
        worst = [max((float(np.abs(g[b] - want[b]).max()) for b in live), default=0.0) for g in (alone, batched, srt)]
        print(f"{name} max_iter {it}: max |diff| to the restatement: alone {worst[0]:.3e}, batched {worst[1]:.3e}, sorted {worst[2]:.3e}; "
              f"steps run per mesh {[len(m['diffs'][:it - 1]) for m in ms]}")
        assert max(worst) <= jc.MODE_TOL
        for b in live:
            assert jc.same_bits(batched[b], alone[b]), (name, it, b)
            one, one_cnt, _ = ms_sorted([ms[b]], it)
            assert jc.same_bits(srt[b], one[0]) and jc.same_bits(cnt[b], one_cnt[0]), (name, it, b)
            assert jc.same_bits(cnt[b], want_cnt[b]), (name, it, b)
            if it == 1:
                assert jc.same_bits(alone[b], np.asarray(ms[b]["x"])) and jc.same_bits(batched[b], alone[b]) and jc.same_bits(srt[b], alone[b])
    if name == "n257":                                                         # the reference-named function
        m = ms[0]
        got = host(J.meanshift_cluster(dev(m["x"]), m["h"], dev(m["w"]).reshape(-1, 1), 12))
        assert jc.same_bits(got, ms_plain(m, 12))


# ---------------------------------------------------------------------------------------------------------------- inside test
@pytest.mark.parametrize("k", range(2 * len(jc.INSIDE_SIZES)), ids=lambda k: f"{('exact', 'fixture')[k % 2]}_{jc.INSIDE_SIZES[k // 2]}")
def test_inside_mask_equals_the_rounded_cells(k):
    c = jc.inside_cases()[k]
    want = jc.inside(c["pts"], c["vox"], c["translate"], c["scale"], c["dims"][0])
    P = dev(c["pts"])
    got = host(get_ops().inside_mask(P, dev(c["vox"].astype(np.uint8).reshape(-1)), c["translate"], c["scale"], c["dims"][0]))
    print(f"{c['name']}: {int(want.sum())} of {len(want)} inside, device {int(got.sum())}; differing rows {np.flatnonzero(got != want)[:8]}")
    assert np.array_equal(got, want)
    vox = types.SimpleNamespace(data=c["vox"], translate=c["translate"], scale=c["scale"], dims=c["dims"])
    pts_in, idx = J.inside_check(P, vox)
    assert np.array_equal(host(idx), np.flatnonzero(want)) and jc.same_bits(host(pts_in), np.asarray(c["pts"])[want])
