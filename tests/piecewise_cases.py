"""Generated cases for the rig-free tracker (csrc/piecewise.hip: ``kmeans_kernel``, ``ransac_vote_kernel``, ``ransac_fit_kernel``,
``ransac_apply_kernel``) at the sizes the kernels branch on, their oracle results (tests/piecewise_oracle.py in float64 and in
longdouble), the yardsticks made of the two, and the compare functions that tests/test_piecewise_cases.py (CPU) and
tests/test_piecewise_differential.py (device) share. Not a test file; numpy only, nothing of the reference, no GPU.

Every input comes from a seed: ``np.random.default_rng([TAG, crc32(name), attempt])``, drawn again (at most ATTEMPTS times, then a loud
failure) until the ORACLE ALONE confirms the conditions of the recorded fixtures and the structural property the case exists for, so
nothing is excluded afterwards:

    k-means  row_margin >= 1e-5, fit_margin >= 1e-5; where a cluster is reseeded, the reseed's vertex is the nearest by >= 1e-5 too
             (the column arg-min of a reseed is a decision like the row arg-min; the fixtures have no condition on it)
    RANSAC   sigma_ratio >= 1e-3, sigma_ratio_vote >= 1e-3, dist_margin >= 1e-9 and, where no refit happens, sum_gap > 1e-9. A problem
             that ends without a fit (every sum >= 1e10) uses no rotation: its sigma_ratio is not asked. The handle-count case asks
             sigma_ratio >= 0.05 of every used fit, so that one ill-conditioned problem does not set the bar of all eleven.

k-means inputs are clustered: blob centres plus noise of norm about 0.15 in the embedding (0.15 / sqrt(D) per component) and 0.1 per
component in position, rows renormalised; uniformly random unit rows do not reach the row margin. RANSAC segments are a rigid motion
of up to 0.6 rad with noise, outliers displaced by 0.5 to 1.0, or an unrelated target, as each case says. The sample triples come from
``piecewise.draw_ransac_samples`` on a seeded ``RandomState``: the same triples go to the oracle and the device.

Yardstick of the continuous RANSAC results: the deviation of the float64 oracle from its own longdouble run, the maximum over a family;
the device gets FACTOR = 16 times that (the factor of tests/test_gpu_piecewise.py: another order of the same sums and the kernel's
in-place Jacobi against the oracle's matrix products cost a few ulps each). k-means centres are compared bit for bit; the fit sum is
held to ``fit_f64_bound`` of tests/test_piecewise_oracle.py, for a float32 X too: the device promotes it exactly as the oracle does."""
import functools
import zlib

import numpy as np

import piecewise_oracle as po
from morig_amd import piecewise
from test_piecewise_oracle import fit_f64_bound

TAG = 0x707763
ATTEMPTS = 60
FACTOR = 16
W_EUC, TOL = 0.2, 1e-4
KM_COND = dict(row_margin=1e-5, fit_margin=1e-5, reseed_margin=1e-5)
RS_COND = dict(sigma_ratio=1e-3, sigma_ratio_vote=1e-3, dist_margin=1e-9, sum_gap=1e-9)
THRESHOLD, INLIER_DIST, REFIT_SHARE = 0.3, 5e-2, 0.35
LONG = np.longdouble


def _rng(name, attempt):
    return np.random.default_rng([TAG, zlib.crc32(name.encode()), attempt])


def unit_rows(a):
    return a / np.sqrt(np.sum(a * a, axis=1, keepdims=True))


# =================================================================================================================== k-means
def km_blobs(rng, s):
    """``sizes`` vertices per blob (or V vertices dealt at random over ``blobs``), shuffled"""
    D = s["D"]
    sizes = s.get("sizes")
    if sizes is None:
        nb = s.get("blobs", 2 * s["K"])
        which = np.concatenate([np.arange(nb), rng.integers(nb, size=max(s["V"] - nb, 0))])[:s["V"]]
    else:
        which = np.repeat(np.arange(len(sizes)), sizes)
        nb = len(sizes)
    which = which[rng.permutation(len(which))]
    cemb = unit_rows(rng.normal(size=(nb, D)))
    cpos = s["spread"] * unit_rows(rng.normal(size=(nb, 3))) if "spread" in s else rng.uniform(-1, 1, size=(nb, 3))
    X = unit_rows(cemb[which] + 0.15 / np.sqrt(D) * rng.normal(size=(len(which), D)))
    pos = cpos[which] + s.get("pos_noise", 0.1) * rng.normal(size=(len(which), 3))
    return X, pos, int(rng.integers(len(which))), which


def km_coincident(rng, s):
    """only ``distinct`` positions: farthest-point sampling runs out of them and repeats vertex 0, the repeated clusters stay empty"""
    X, pos, first, which = km_blobs(rng, dict(s, blobs=s["distinct"]))
    cpos = rng.uniform(-1, 1, size=(s["distinct"], 3))
    return X, cpos[which], first, which


def km_duplicates(rng, s):
    """``copies`` identical rows (position and embedding) among otherwise distinct vertices. Their position is a multiple of 2^-10, so
    that its sums and the mean are exact and the cluster of the copies keeps a centre that is bitwise the position of a copy"""
    X, pos, first, which = km_blobs(rng, s)
    at = rng.choice(len(X), size=s["copies"], replace=False)
    X[at], pos[at] = X[at[0]], np.round(pos[at[0]] * 1024) / 1024
    return X, pos, first, which


def km_last_survives(rng, s):
    """three far blobs of at most 8 vertices and a large one next to the blob of the first seed: farthest-point sampling reaches it last"""
    sizes = s["sizes"]
    which = np.repeat(np.arange(4), sizes)
    which = which[rng.permutation(len(which))]
    cpos = np.array([[5.0, 0, 0], [-5.0, 0, 0], [0, 5.0, 0], [5.0, 1.0, 0]])
    cemb = unit_rows(rng.normal(size=(4, s["D"])))
    X = unit_rows(cemb[which] + 0.15 / np.sqrt(s["D"]) * rng.normal(size=(len(which), s["D"])))
    pos = cpos[which] + 0.05 * rng.normal(size=(len(which), 3))
    return X, pos, int(np.nonzero(which == 0)[0][0]), which


KM_MAKERS = dict(blobs=km_blobs, coincident=km_coincident, duplicates=km_duplicates, last_survives=km_last_survives)


def _k(V, D, K, dtype="float32", make="blobs", prop="iterates", family="", max_iter=100, tol=TOL, **kw):
    return dict(V=V, D=D, K=K, dtype=dtype, make=make, prop=prop, family=family, max_iter=max_iter, tol=tol, **kw)


def km_specs():
    out = {}
    for V in (1023, 1024, 1025, 2049):
        out[f"stride_v{V}"] = _k(V, 8, 6, prop="second_pass" if V > 1024 else "iterates", family="thread stride")
    for V in (63, 64, 65, 128, 129):
        out[f"ballot_v{V}"] = _k(V, 16, 4, prop="last_chunk", family="ballot chunks")
    for D in (1, 2, 3, 63, 64, 65, 127, 128):
        for dt in ("float32", "float64"):
            out[f"lanes_d{D}_{dt}"] = _k(257, D, {1: 2, 2: 4}.get(D, 6), dt, prop="iterates", family="embedding lanes")
    for K in (1, 15, 16, 17, 33, 49, 64):
        out[f"rounds_k{K}"] = _k(1025, 8, K, prop="last_round", family="cluster rounds")
    out["rounds_k64_d128"] = _k(1025, 128, 64, prop="last_round", family="cluster rounds")
    out["reseed_coincident_k40"] = _k(300, 8, 40, make="coincident", distinct=12, prop="reseed_16_and_32", family="reseeds")
    out["reseed_v40_k64"] = _k(40, 8, 64, make="duplicates", copies=10, blobs=40, prop="reseed_32_and_survivor", family="reseeds")
    out["prune_8_and_9"] = _k(8 + 9 + 30 + 40 + 25, 8, 5, sizes=(8, 9, 30, 40, 25), spread=3.0, pos_noise=0.05, prop="members_8_and_9",
                              family="prune")
    out["prune_last_survives"] = _k(5 + 6 + 7 + 60, 8, 4, make="last_survives", sizes=(5, 6, 7, 60), prop="only_last_kept", family="prune")
    out["prune_v9_k1"] = _k(9, 8, 1, blobs=1, prop="kept_1", family="prune")
    out["prune_v8_k1"] = _k(8, 8, 1, blobs=1, prop="none_kept", family="prune")
    out["prune_v12_k20"] = _k(12, 8, 20, blobs=12, prop="none_kept", family="prune")
    out["loop_max_iter_0"] = _k(257, 8, 6, max_iter=0, prop="no_iteration", family="loop ends")
    out["loop_max_iter_1"] = _k(257, 8, 6, max_iter=1, prop="cut_at_1", family="loop ends")
    out["loop_large_tol"] = _k(257, 8, 6, tol=1e3, prop="stopped_at_1", family="loop ends")
    # the ragged batch: D = 8, K = 6, float32 (stride_v1025 is its second mesh); no v0 after the first is a multiple of 64
    out["batch_v65"] = _k(65, 8, 6, family="batch")
    out["batch_v9_copies"] = _k(9, 8, 6, make="duplicates", copies=9, blobs=2, prop="one_cluster_of_9", family="batch")
    out["batch_v257"] = _k(257, 8, 6, family="batch")
    out["batch_v129"] = _k(129, 8, 6, family="batch")
    out["batch_v120_reseeds"] = _k(120, 8, 6, make="coincident", distinct=4, prop="reseeds", family="batch")
    return out


KM_SPECS = km_specs()
KM_NAMES = tuple(KM_SPECS)
KM_BATCH = ("batch_v65", "stride_v1025", "batch_v9_copies", "batch_v257", "batch_v129", "batch_v120_reseeds")
KM_NO_CLUSTER = ("prune_v8_k1", "prune_v12_k20")


def km_property(c, labels, st):
    """the structure the case exists for, from the oracle's state"""
    s, K, V, m = c["spec"], c["spec"]["K"], c["spec"]["V"], st["members"]
    ks = [k for _, k in st["reseeded"]]
    p = s["prop"]
    if p == "iterates":                                                        # the centre update moved labels: a third iteration
        return st["n_iter"] >= 3 and st["n_kept"] >= 1
    if p == "second_pass":                                                     # vertices of a thread's second pass carry several labels
        return st["n_iter"] >= 3 and len(np.unique(labels[1024:])) >= min(2, V - 1024)
    if p == "last_chunk":                                                      # the last (partial) ballot chunk has members of a kept cluster
        return st["n_iter"] >= 3 and st["n_kept"] >= 2 and m.sum() == V
    if p == "last_round":                                                      # a cluster of the owning wave's last round has members
        return st["n_iter"] >= (3 if K > 1 else 2) and m[16 * ((K - 1) // 16):].sum() > 0 and (m > 0).sum() >= min(K, 12)
    if p == "reseed_16_and_32":
        return len(set(c["seeds_pos"])) < K and any(16 <= k < 32 for k in ks) and any(k >= 32 for k in ks)
    if p == "reseed_32_and_survivor":
        return V < K and any(k >= 32 for k in ks) and st["n_kept"] >= 1
    if p == "members_8_and_9":
        return 8 in m and 9 in m and st["n_kept"] == K - 1
    if p == "only_last_kept":
        return np.array_equal(np.nonzero(m > 8)[0], [K - 1]) and np.all(labels == 0)
    if p == "kept_1":
        return st["n_kept"] == 1 and m.tolist() == [9]
    if p == "none_kept":
        return st["n_kept"] == 0 and np.all(labels == -1) and m.max() <= 8
    if p == "no_iteration":
        return st["n_iter"] == 0 and np.array_equal(st["centres_euc"], c["verts"][st["seeds"]])
    if p == "cut_at_1":                                                        # the change of the fit sum was above tol: the cut ended the loop
        return st["n_iter"] == 1 and c["delta_first"] >= TOL + 1e-5
    if p == "stopped_at_1":                                                    # tol ended it, where the default tol would have gone on
        return st["n_iter"] == 1 and TOL + 1e-5 <= c["delta_first"] < s["tol"]
    if p == "one_cluster_of_9":
        return st["n_kept"] == 1 and len(ks) > 0 and m.max() == 9
    if p == "reseeds":
        return len(ks) > 0 and st["n_kept"] >= 1
    raise KeyError(p)


def km_oracle(c, dtype=np.float64):
    s = c["spec"]
    return po.kernel_kmeans(c["X"], c["verts"], s["K"], s["max_iter"], W_EUC, s["tol"], c["first"], dtype=dtype)


def km_conditions(st):
    return all(st[k] >= v for k, v in KM_COND.items())


@functools.lru_cache(maxsize=None)
def km_case(name):
    s = KM_SPECS[name]
    for attempt in range(ATTEMPTS):
        X, pos, first, _ = KM_MAKERS[s["make"]](_rng(name, attempt), s)
        c = dict(name=name, spec=s, X=np.ascontiguousarray(X.astype(s["dtype"])), verts=np.ascontiguousarray(pos), first=first)
        assert c["X"].shape == (s["V"], s["D"]) and c["verts"].shape == (s["V"], 3)
        labels, st = km_oracle(c)
        c["seeds_pos"] = [tuple(pos[i]) for i in st["seeds"]]
        if s["prop"] in ("cut_at_1", "stopped_at_1"):                          # |fit(seeds) - fit(first update)|, from a run of one iteration
            one = po.kernel_kmeans(c["X"], c["verts"], s["K"], 1, W_EUC, 0.0, first)[1]
            zero = po.kernel_kmeans(c["X"], c["verts"], s["K"], 0, W_EUC, 0.0, first)[1]
            c["delta_first"] = abs(zero["fit"] - one["fit"])
        if km_conditions(st) and km_property(c, labels, st):
            c.update(attempts=attempt + 1, want=(labels, st))
            return c
    raise AssertionError(f"k-means case {name}: no draw of {ATTEMPTS} met the conditions and the property {s['prop']!r}")


KM_DISCRETE = ("seeds", "n_iter", "n_kept", "members")


def km_compare(label, name, labels, st, centres=True):
    """print, then assert: a result (the device's, the longdouble oracle's) against the float64 oracle. Discrete results equal; with
    ``centres`` the centre arrays bit for bit and the fit sum within fit_f64_bound -> the fit sum's share of its bound"""
    c = km_case(name)
    want_labels, want = c["want"]
    for k in KM_DISCRETE:
        assert np.array_equal(np.asarray(st[k]), np.asarray(want[k])), (name, k, st[k], want[k])
    assert np.array_equal(np.asarray(labels), want_labels), (name, "labels", int(np.sum(np.asarray(labels) != want_labels)))
    if not centres:
        return 0.0
    bound = fit_f64_bound(dict(V=c["spec"]["V"], D=c["spec"]["D"], fit=want["fit"]))
    share = abs(float(st["fit"]) - want["fit"]) / bound if bound > 0 else abs(float(st["fit"]) - want["fit"])
    worst = max(float(np.abs(np.asarray(st[k], dtype=np.float64) - want[k]).max()) for k in ("centres_emb", "centres_euc"))
    print(f"\n{label} {name}: centres differ by at most {worst:.1e} (bar 0: bits), fit sum {float(st['fit']):.17g} vs {want['fit']:.17g}: "
          f"{share:.3f} of its bound {bound:.2e}")
    for k in ("centres_emb", "centres_euc"):
        got = np.asarray(st[k])
        assert got.dtype == np.float64 and np.array_equal(got, want[k]), (name, k, worst)
    if c["spec"]["dtype"] == "float32":                                        # the embedding centres hold float32 values
        assert np.array_equal(np.asarray(st["centres_emb"]).astype(np.float32).astype(np.float64), np.asarray(st["centres_emb"]))
    assert share <= 1.0, (name, "fit", st["fit"], want["fit"], bound)
    return share


# =================================================================================================================== RANSAC
def rotation(rng, angle=0.6):
    axis = rng.normal(size=3)
    axis /= np.sqrt(np.sum(axis * axis))
    a = rng.uniform(0.2, angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def far(rng, n, lo=0.5, hi=1.0):
    return unit_rows(rng.normal(size=(n, 3))) * rng.uniform(lo, hi, size=(n, 1))


def segment(rng, kind, nh, extra=0, **kw):
    """-> (src, dst, vis) of one segment: its ``nh`` handles first, in handle-list order, then ``extra`` vertices below the threshold.
    kinds: "motion" a rigid motion plus ``noise`` on every handle; "share" the motion on 25 % of the handles, the rest displaced (the
    smallest-sum hypothesis is used); "exact" an exact motion on the handle positions ``inliers``, the rest displaced; "unrelated" a
    target that has nothing of the source; "huge" every target displaced by about 1e10 in its own direction (no sum below 1e10)"""
    n = nh + extra
    src = rng.uniform(-0.5, 0.5, size=(n, 3)) + rng.uniform(-1, 1, size=3)
    R, t = rotation(rng), rng.uniform(-0.3, 0.3, size=3)
    dst = src @ R.T + t
    if kind == "motion":
        dst += kw.get("noise", 0.01) * rng.normal(size=(n, 3))
    elif kind == "share":
        dst += 0.005 * rng.normal(size=(n, 3))
        out = rng.permutation(nh)[:nh - nh // 4]
        dst[out] += far(rng, len(out), 0.2, 0.5)
    elif kind == "exact":
        inl = np.zeros(n, dtype=bool)
        inl[list(kw["inliers"])] = True
        dst[inl] += kw.get("noise", 0.0) * rng.normal(size=(int(inl.sum()), 3))
        dst[~inl] += far(rng, int((~inl).sum()))
    elif kind == "unrelated":
        dst = rng.uniform(-3.0, 3.0, size=(n, 3))                              # six times the source's size: no triple fits its own samples
    elif kind == "huge":
        dst = src + unit_rows(rng.normal(size=(n, 3))) * rng.uniform(1e10, 2e10, size=(n, 1))
    else:
        raise KeyError(kind)
    vis = np.concatenate([rng.uniform(0.35, 1.0, size=nh), rng.uniform(0.0, 0.25, size=extra)])
    return src, dst, vis


def mesh(rng, segs, dtype=np.float64):
    """segments [(label, kind, nh, extra, kw)] -> dict(src, dst, vis, seg): the vertices of the segments interleaved at random, each
    segment's own order kept (so a handle's position in its list is its position in ``segment``)"""
    parts = [segment(rng, kind, nh, extra, **kw) for _, kind, nh, extra, kw in segs]
    owner = np.repeat(np.arange(len(segs)), [len(p[0]) for p in parts])
    owner = owner[rng.permutation(len(owner))]
    V = len(owner)
    src, dst, vis = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    seg = np.zeros(V, dtype=np.int64)
    for i, (p, s) in enumerate(zip(parts, segs)):
        at = np.nonzero(owner == i)[0]
        src[at], dst[at], vis[at], seg[at] = p[0], p[1], p[2], s[0]
    return dict(src=src.astype(dtype), dst=dst.astype(dtype), vis=vis.astype(dtype), seg=seg)


def S(label, kind, nh, extra=3, **kw):
    return (label, kind, nh, extra, kw)


HANDLE_COUNTS = (4, 5, 64, 128, 129, 255, 256, 257, 512, 513, 1000)
SMALL_COUNTS = tuple(5 + i % 5 for i in range(40))
THREE = [[S(0, "motion", 20), S(1, "share", 70), S(2, "motion", 130)]]


def _b(meshes, n_iter, family, prop, dtype=np.float64):
    return dict(meshes=meshes, n_iter=n_iter, family=family, prop=prop, dtype=dtype)


RS_SPECS = {
    # refits at 4, 5, 128, 255, 257 and 513 handles (the fit kernel's second and third pass), the smallest sum elsewhere
    "handles": _b([[S(i, "share" if nh >= 64 and i % 2 == 0 else "motion", nh, noise=1e-3 if nh < 64 else 0.01)
                    for i, nh in enumerate(HANDLE_COUNTS)]], 100, "handle counts", "handle_counts"),
    **{f"iter{n}": _b(THREE, n, "hypothesis counts", "three_problems") for n in (1, 3, 4, 5, 7, 100)},
    "many_small": _b([[S(i, "motion", nh, 1, noise=1e-3) for i, nh in enumerate(SMALL_COUNTS)]], 3, "hypothesis counts", "forty_problems"),
    # noise of 1e-4 on the motion: an exact one gives every all-inlier hypothesis the same sum up to rounding, which sum_gap excludes
    "share": _b([[S(0, "exact", 40, inliers=range(0, 28, 2), noise=1e-4), S(1, "exact", 40, inliers=range(0, 30, 2), noise=1e-4),
                  S(2, "exact", 20, inliers=range(1, 15, 2), noise=1e-4), S(3, "exact", 20, inliers=range(1, 17, 2), noise=1e-4)]],
                100, "refit boundary", "share"),
    "late": _b([[S(0, "exact", 600, inliers=range(300, 600), noise=0.005), S(1, "exact", 10, inliers=range(4))]], 100, "late inliers", "late"),
    "selection": _b([[S(0, "exact", 30, inliers=range(3, 27, 2)), S(1, "unrelated", 30)]], 100, "selection", "selection"),
    "nofit": _b([[S(0, "motion", 30), S(1, "share", 40)], [S(5, "motion", 20), S(9, "huge", 12), S(11, "share", 33)], [S(0, "motion", 65)]],
                20, "no fit", "nofit"),
    "labels": _b([[S(-7, "motion", 30), S(2 ** 31 + 5, "share", 40), S(3, "motion", 12), S(2 ** 40, "motion", 2)]], 20, "labels", "labels"),
    "shapes": _b([[S(0, "motion", 30), S(1, "motion", 3, 5)], [S(4, "motion", 3, 4), S(2, "motion", 0, 6), S(9, "motion", 1, 0)],
                  [S(0, "share", 66)]], 20, "segment shapes", "shapes"),
    "no_problem": _b([[S(0, "motion", 3, 4), S(1, "motion", 2, 0)], [S(0, "motion", 1, 0)]], 20, "segment shapes", "no_problem"),
    "float32": _b([[S(0, "motion", 30), S(1, "share", 70), S(2, "motion", 3, 2)]], 20, "input types", "float32", np.float32),
}
RS_NAMES = tuple(RS_SPECS)
RS_FAMILIES = tuple(dict.fromkeys(s["family"] for s in RS_SPECS.values()))
QUANTITIES = ("R", "t", "vertices", "sums")


def rs_property(name, c):
    """the structure the batch exists for, from the float64 oracle's details"""
    p, det = RS_SPECS[name]["prop"], c["want"]
    flat = [d for _, dd in det for d in dd]
    nh = [len(d["handles"]) for d in flat]
    if p == "handle_counts":
        big = [d["refit"] for d in flat if len(d["handles"]) > 256]
        # every used fit well conditioned (s2 / s1 >= 0.05): one ill-conditioned problem would set the bar of all eleven
        return (tuple(nh) == HANDLE_COUNTS and any(big) and not all(big) and all(d["refit"] for d in flat[:2])
                and min(d["sigma_ratio"] for d in flat) >= 0.05)
    if p == "three_problems":
        return nh == [20, 70, 130] and [d["refit"] for d in flat] == [True, False, True]
    if p == "forty_problems":
        return tuple(nh) == SMALL_COUNTS and all(d["refit"] for d in flat)
    if p == "share":                                                           # 0.35 * 40 is 14.0 and 0.35 * 20 is 7.0 in float64
        return (REFIT_SHARE * 40 == 14.0 and REFIT_SHARE * 20 == 7.0 and [d["best_count"] for d in flat] == [14, 15, 7, 8]
                and [d["refit"] for d in flat] == [False, True, False, True])
    if p == "late":
        a, b = flat
        return (a["refit"] and b["refit"] and len(a["handles"]) == 600 and a["inliers"].min() >= 256 and len(a["inliers"]) > 210
                and b["inliers"].tolist() == [0, 1, 2, 3])
    if p == "selection":
        a, b = flat
        return (int(np.sum(a["counts"] == a["best_count"])) >= 2 and a["by_count"] == int(np.argmax(a["counts"])) and a["best_count"] == 12
                and b["by_count"] == -1 and b["best_count"] == 0 and not b["refit"] and b["by_sum"] >= 0 and np.all(b["counts"] == 0))
    if p == "nofit":
        bad = [d for d in det[1][1] if d["label"] == 9][0]
        return (bad["R"] is None and bad["by_sum"] == -1 and bad["by_count"] == -1 and np.all(bad["sums"] >= 1e10)
                and all(d["R"] is not None for d in flat if d is not bad) and len(flat) == 6)
    if p == "labels":
        return [d["label"] for d in flat] == [-7, 3, 2 ** 31 + 5] and len(np.unique(c["meshes"][0]["seg"][:12])) >= 3
    if p == "shapes":
        return [len(dd) for _, dd in det] == [1, 0, 1] and np.array_equal(det[1][0], c["meshes"][1]["dst"])
    if p == "no_problem":
        return all(len(dd) == 0 for _, dd in det) and len(c["meshes"][1]["src"]) == 1
    if p == "float32":
        return all(c["meshes"][0][k].dtype == np.float32 for k in ("src", "dst", "vis")) and len(flat) == 2
    raise KeyError(p)


def handle_counts(m):
    return [len(h) for h in po.segment_handles(m["vis"], m["seg"], THRESHOLD)[1]]


def rs_oracle(c, dtype=np.float64):
    """-> [(moved vertices, details)] per mesh; a problem without a fit stays in the details with R None"""
    return [po.piecewise_ransac(m["src"], m["dst"], m["vis"], m["seg"], smp, THRESHOLD, INLIER_DIST, REFIT_SHARE, dtype=dtype, unfitted="keep")
            for m, smp in zip(c["meshes"], c["mesh_samples"])]


def rs_conditions(det):
    for _, dd in det:
        for d in dd:
            if d["R"] is not None and d["sigma_ratio"] < RS_COND["sigma_ratio"]:
                return False
            if d["sigma_ratio_vote"] < RS_COND["sigma_ratio_vote"] or d["dist_margin"] < RS_COND["dist_margin"]:
                return False
            if not d["refit"] and d["R"] is not None and not d["sum_gap"] > RS_COND["sum_gap"]:
                return False
    return True


def split_samples(samples, counts_per_mesh):
    """the batch's [P, n_iter, 3] samples -> one slice per mesh, in the order draw_ransac_samples drew them"""
    out, at = [], 0
    for counts in counts_per_mesh:
        n = sum(h >= po.MIN_HANDLES for h in counts)
        out.append(samples[at:at + n])
        at += n
    assert at == len(samples)
    return out


@functools.lru_cache(maxsize=None)
def rs_case(name):
    s = RS_SPECS[name]
    for attempt in range(ATTEMPTS):
        rng = _rng(name, attempt)
        meshes = [mesh(rng, segs, s["dtype"]) for segs in s["meshes"]]
        counts = [handle_counts(m) for m in meshes]
        samples = piecewise.draw_ransac_samples([h for c in counts for h in c], s["n_iter"], np.random.RandomState(int(rng.integers(2 ** 31))))
        c = dict(name=name, spec=s, meshes=meshes, counts=counts, samples=samples, mesh_samples=split_samples(samples, counts),
                 n_iter=s["n_iter"])
        c["want"] = rs_oracle(c)
        if rs_conditions(c["want"]) and rs_property(name, c):
            c["attempts"] = attempt + 1
            return c
    raise AssertionError(f"RANSAC case {name}: no draw of {ATTEMPTS} met the conditions and the property {s['prop']!r}")


def lists(c, meshes=None):
    """the four lists piecewise.piecewise_ransac takes (``meshes``: indices; all by default)"""
    idx = range(len(c["meshes"])) if meshes is None else meshes
    return tuple([c["meshes"][i][k] for i in idx] for k in ("src", "dst", "vis", "seg"))


def rs_discrete(name, got, want):
    """assert: details per problem (the device's, flat with ``mesh``; or the oracle's per mesh) hold the oracle's discrete results"""
    flat = [(mi, d) for mi, (_, dd) in enumerate(want) for d in dd]
    assert len(got) == len(flat), (name, len(got), len(flat))
    for g, (mi, w) in zip(got, flat):
        key = (name, mi, w["label"])
        assert (g.get("mesh", mi), g["label"]) == (mi, w["label"]), key
        assert np.array_equal(g["handles"], w["handles"]), key
        assert np.array_equal(g["counts"], w["counts"]), (key, "counts")
        assert (g["by_count"], g["best_count"], bool(g["refit"])) == (w["by_count"], w["best_count"], w["refit"]), key
        if not w["refit"]:
            assert g["by_sum"] == w["by_sum"], (key, "by_sum")


def rs_deviation(got_out, got, want):
    """-> {R, t, vertices: largest absolute difference; sums: largest relative one} of a run against an oracle run"""
    dev = dict.fromkeys(QUANTITIES, 0.0)
    flat = [d for _, dd in want for d in dd]
    for g, w in zip(got, flat):
        if w["R"] is not None:
            dev["R"] = max(dev["R"], float(np.abs(np.asarray(g["R"], dtype=LONG) - w["R"]).max()))
            dev["t"] = max(dev["t"], float(np.abs(np.asarray(g["t"], dtype=LONG) - w["t"]).max()))
        dev["sums"] = max(dev["sums"], float(np.abs(np.asarray(g["sums"], dtype=LONG) / w["sums"] - 1).max()))
    for o, (w, _) in zip(got_out, want):
        if len(w):
            dev["vertices"] = max(dev["vertices"], float(np.abs(np.asarray(o, dtype=LONG) - w).max()))
    return dev


@functools.lru_cache(maxsize=None)
def rs_long(name):
    return rs_oracle(rs_case(name), LONG)


@functools.lru_cache(maxsize=None)
def rs_yardstick(family):
    """the float64 oracle against its own longdouble run: the maximum over the family's batches"""
    out = dict.fromkeys(QUANTITIES, 0.0)
    for name in RS_NAMES:
        if RS_SPECS[name]["family"] == family:
            want, ref = rs_case(name)["want"], rs_long(name)
            dev = rs_deviation([o for o, _ in want], [d for _, dd in want for d in dd], ref)
            out = {q: max(out[q], dev[q]) for q in QUANTITIES}
    return out


def rs_bounds(family):
    return {q: FACTOR * v for q, v in rs_yardstick(family).items()}


def rs_compare(label, name, got_out, got):
    """print, then assert: discrete results equal the float64 oracle's, continuous ones within FACTOR times the family's yardstick of
    the LONGDOUBLE oracle; vertices of segments with < 4 handles (and of a segment without a fit) bit for bit -> the deviations"""
    c, family = rs_case(name), RS_SPECS[name]["family"]
    rs_discrete(name, got, c["want"])
    dev, bar, yard = rs_deviation(got_out, got, rs_long(name)), rs_bounds(family), rs_yardstick(family)
    print(f"\n{label} {name} [{family}]: " + ", ".join(f"{q} {dev[q]:.2e} (yardstick {yard[q]:.2e}, bar {bar[q]:.2e})" for q in QUANTITIES))
    for q in QUANTITIES:
        assert dev[q] <= bar[q], (name, q, dev[q], bar[q])
    for o, m, (_, dd) in zip(got_out, c["meshes"], c["want"]):
        rank, handles = po.segment_handles(m["vis"], m["seg"], THRESHOLD)
        unfit = {d["label"] for d in dd if d["R"] is None}
        labels = np.unique(m["seg"])
        for l, h in enumerate(handles):
            if len(h) < po.MIN_HANDLES:
                assert np.array_equal(np.asarray(o)[rank == l], m["dst"][rank == l].astype(np.float64)), (name, "copy", int(labels[l]))
            elif int(labels[l]) in unfit:
                assert np.array_equal(np.asarray(o)[rank == l], m["src"][rank == l].astype(np.float64)), (name, "unfitted", int(labels[l]))
    return dev


def table(device=None):
    """the yardsticks per family (and the device's family maxima where given: {batch name: rs_deviation}), and the bars in use"""
    rows = ["family             quantity  f64 vs longdouble  bar" + ("        device" if device else "")]
    for family in RS_FAMILIES:
        for q in QUANTITIES:
            row = f"{family:18s} {q:9s} {rs_yardstick(family)[q]:.2e}           {rs_bounds(family)[q]:.2e}"
            if device:
                row += f"   {max(device[n][q] for n in RS_NAMES if RS_SPECS[n]['family'] == family and n in device):.2e}"
            rows.append(row)
    return "\n".join(rows)
