"""Fixtures of the rig-free tracker (tests/golden/piecewise_ransac.npz, piecewise_kmeans.npz), made by the reference's own
``Piecewise_RANSAC`` (utils/piecewise_ransac.py) and ``KernelKMeans`` (utils/kernel_kmeans.py), imported where they lie at generation time
(open3d and cv2 stubbed as empty modules, ``np.int = int``). ``np.random`` is seeded and its ``choice`` / ``randint`` are wrapped, so the
draws are recorded as the reference made them; ``icp`` and ``calc_dist`` of the instances are wrapped to record every fit and every distance
matrix. Nothing of the reference is written into the repository: only inputs, recorded draws, results and intermediate decisions.

piecewise_ransac  one ragged batch of float64 meshes:
  sizes     segments with 0, 3, 4, 63, 65 and 257 handles (plus vertices below the visibility threshold), each following one rigid motion
            with 1 % noise
  branches  labels {7, 2, 40} interleaved along the vertex order: 7 follows one motion (refit branch); 25 % of the handles of 2 follow
            the motion and the rest are displaced by 0.2 to 0.5 (smallest-sum branch); the target of 40 is unrelated to its source (no
            hypothesis has an inlier); visibility values equal to 0.3 (kept) and nextafter(0.3, 0) (not kept) among them
  single    a mesh of one segment
  one       a mesh with V = 1
piecewise_kmeans  (V 257, D 16, K 6); (V 1000, D 64, K 20), its embeddings drawn from a codebook of 64 rows so that the file stays small;
  coincident vertices (two seeds coincide: the reseed branch runs); (V 70, K 8) ending with a dropped cluster; the first case cut off at
  max_iter = 2; one float64-X case.

The seed is redrawn until these conditions hold (stored in meta, re-asserted by tests/test_piecewise_oracle.py):
  RANSAC   every fitted covariance -- the voting hypotheses and the fits that reach the output -- has s2 / s1 >= 1e-3; no handle
           distance within 1e-8 of the inlier distance; on the smallest-sum branch the two smallest distance sums of the problem
           differ by more than 1e-9 relative (on the refit branch that hypothesis is not used, and a segment of 4 handles has only
           4 distinct triples among its 100 draws, so sums equal up to rounding are certain there).
  k-means  every row arg-min has a margin >= 1e-5 to the nearest value that is not bitwise equal to it (identical centres give identical
           columns, where the first wins everywhere); | |delta fit| - tol | >= 1e-5 in every iteration.

Run from the repository root:  python tools/make_piecewise_golden.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import shim                                                        # noqa: E402
import make_skin_golden as msg                                                 # noqa: E402  (save)

SIGMA_RATIO, SIGMA_RATIO_VOTE, DIST_GAP, SUM_GAP, ROW_MARGIN, FIT_MARGIN = 1e-3, 1e-3, 1e-8, 1e-9, 1e-5, 1e-5
THRESHOLD, INLIER, SHARE = 0.3, 5e-2, 0.35


def reference():
    for name in ("open3d", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    np.int = int
    if shim.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, shim.REFERENCE_ROOT)
    pr = __import__("utils.piecewise_ransac", fromlist=["Piecewise_RANSAC"])
    km = __import__("utils.kernel_kmeans", fromlist=["KernelKMeans"])
    return pr.Piecewise_RANSAC, km.KernelKMeans


class Recorder:
    """wraps np.random.choice / randint while active"""

    def __enter__(self):
        self.choices, self.randints = [], []
        self._c, self._r = np.random.choice, np.random.randint

        def choice(*a, **k):
            out = self._c(*a, **k)
            self.choices.append(np.array(out))
            return out

        def randint(*a, **k):
            out = self._r(*a, **k)
            self.randints.append(int(out))
            return out

        np.random.choice, np.random.randint = choice, randint
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.randint = self._c, self._r


# ------------------------------------------------------------------------------------------------------------------------- RANSAC
def rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def moved(rng, pts, noise=0.01):
    R, t = rotation(rng, rng.uniform(0.2, 0.8)), rng.uniform(-0.2, 0.2, 3)
    return pts @ R.T + t + rng.normal(size=pts.shape) * noise


def ransac_meshes(rng):
    meshes = {}
    # sizes: label l has HANDLES[l] handles and a few vertices below the threshold
    src, dst, vis, seg = [], [], [], []
    for l, h in enumerate((0, 3, 4, 63, 65, 257)):
        extra = 5
        p = rng.uniform(-0.5, 0.5, (h + extra, 3)) + rng.uniform(-1, 1, 3)
        src.append(p)
        dst.append(moved(rng, p))
        vis.append(np.concatenate([rng.uniform(0.35, 1.0, h), rng.uniform(0.0, 0.25, extra)]))
        seg.append(np.full(h + extra, l))
    perm = rng.permutation(sum(len(s) for s in src))
    meshes["sizes"] = tuple(np.concatenate(a)[perm] for a in (src, dst, vis, seg))
    # branches: labels 7, 2, 40 interleaved
    n = 60
    p7, p2, p40 = (rng.uniform(-0.5, 0.5, (n, 3)) + o for o in ([0, 0, 0], [2, 0, 0], [0, 2, 0]))
    d7 = moved(rng, p7)
    d2 = moved(rng, p2, noise=0.002)
    out = rng.permutation(n)[:(3 * n) // 4]                                   # 75 % displaced by 0.2 .. 0.5
    dirs = rng.normal(size=(len(out), 3))
    d2[out] += dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(0.2, 0.5, (len(out), 1))
    d40 = rng.uniform(-1.5, 1.5, (n, 3)) * np.array([3.0, 0.3, 1.0])           # unrelated to its source
    src, dst = np.stack([p7, p2, p40], 1).reshape(-1, 3), np.stack([d7, d2, d40], 1).reshape(-1, 3)
    seg = np.tile([7, 2, 40], n)
    vis = rng.uniform(0.35, 1.0, 3 * n)
    vis[[0, 4, 8]] = 0.3                                                       # kept
    vis[[3, 7, 11]] = np.nextafter(0.3, 0)                                     # not kept
    low = rng.permutation(np.arange(12, 3 * n))[:15]
    vis[low] = rng.uniform(0.0, 0.29, 15)
    meshes["branches"] = (src, dst, vis, seg)
    p = rng.uniform(-0.5, 0.5, (40, 3))
    meshes["single"] = (p, moved(rng, p), rng.uniform(0.0, 1.0, 40), np.full(40, 5))
    meshes["one"] = (rng.uniform(-0.5, 0.5, (1, 3)), rng.uniform(-0.5, 0.5, (1, 3)), np.array([0.9]), np.array([3]))
    return meshes


def run_ransac(Ransac, seed):
    import piecewise_oracle as po
    rng = np.random.default_rng(seed)
    meshes = ransac_meshes(rng)
    np.random.seed(seed)
    arrs, metas, problems, all_samples = {}, [], [], []
    margins = dict(sigma_ratio=np.inf, sigma_ratio_vote=np.inf, dist_margin=np.inf, sum_gap=np.inf)
    fit_M, fit_R = [], []
    for mi, (name, (src, dst, vis, seg)) in enumerate(meshes.items()):
        deformer = Ransac(vismask_threshold=THRESHOLD)
        calls, icp = [], deformer.icp

        def wrapped(s, t, icp=icp, calls=calls):
            R, tr = icp(s, t)
            calls.append((np.array(s), np.array(t), np.array(R), np.array(tr).reshape(3)))
            return R, tr

        deformer.icp = wrapped
        with Recorder() as rec:
            out = deformer.run(src.copy(), dst, vis, seg)
        arrs.update({f"m{mi}_src": src, f"m{mi}_dst": dst, f"m{mi}_vis": vis, f"m{mi}_seg": seg.astype(np.int64), f"m{mi}_out": out})
        rank, handles = po.segment_handles(vis, seg, THRESHOLD)
        labels = np.unique(seg)
        solved = [l for l, h in enumerate(handles) if len(h) >= 4]
        assert len(rec.choices) == 100 * len(solved) and len(calls) >= 100 * len(solved)
        at = 0
        for k, l in enumerate(solved):
            h = handles[l]
            samples = np.array(rec.choices[100 * k:100 * (k + 1)], dtype=np.int32)
            hyp = calls[at:at + 100]
            at += 100
            counts, sums = np.zeros(100, dtype=np.int64), np.zeros(100)
            for i, (s, t, R, tr) in enumerate(hyp):
                assert np.array_equal(s, src[h][samples[i]])
                d = np.sqrt(np.sum((np.matmul(src[h], R.T) + tr - dst[h]) ** 2, axis=1))
                counts[i], sums[i] = np.sum(d < INLIER), d.sum()
                margins["dist_margin"] = min(margins["dist_margin"], float(np.min(np.abs(d - INLIER))))
            by_count, by_sum, best = po.select(counts, sums)
            refit = best > SHARE * len(h)
            if refit:
                s, t, R, tr = calls[at]
                at += 1
                assert len(s) == best
                fits = hyp + [(s, t, R, tr)]
            else:
                R, tr = hyp[by_sum][2], hyp[by_sum][3]
                fits = hyp
            used = [(s, t)] if refit else [hyp[by_sum][:2]]                    # the fit that reaches the output
            for key, which in (("sigma_ratio_vote", [f[:2] for f in hyp]), ("sigma_ratio", used)):
                for s_, t_ in which:
                    M = (t_ - t_.mean(0)).T @ (s_ - s_.mean(0))
                    sv = np.linalg.svd(M, compute_uv=False)
                    margins[key] = min(margins[key], float(sv[1] / sv[0]))
                    if np.linalg.det(M) < 0 and len(s_) > 3:
                        margins[key] = min(margins[key], float((sv[1] - sv[2]) / sv[0]))
            for s, t, R_, _ in fits[:10] + fits[100:] + [hyp[by_sum]] + ([hyp[by_count]] if by_count >= 0 else []):
                fit_M.append((t - t.mean(0)).T @ (s - s.mean(0)))
                fit_R.append(R_)
            two = np.sort(sums)[:2]
            if not refit:                                                      # only there the smallest-sum hypothesis is used
                margins["sum_gap"] = min(margins["sum_gap"], float((two[1] - two[0]) / two[1]))
            members = rank == l
            assert np.array_equal(out[members], np.matmul(src[members], R.T) + tr)
            problems.append(dict(mesh=mi, label=int(labels[l]), n_handles=len(h), by_count=by_count, by_sum=by_sum, best_count=best,
                                 refit=bool(refit)))
            p = len(problems) - 1
            arrs.update({f"p{p}_handles": h.astype(np.int64), f"p{p}_counts": counts, f"p{p}_sums": sums, f"p{p}_R": R, f"p{p}_t": tr})
            all_samples.append(samples)
        assert at == len(calls)
        metas.append(dict(name=name, V=len(src), handle_counts=[len(h) for h in handles]))
    arrs["samples"] = np.stack(all_samples)
    arrs["fit_M"], arrs["fit_R"] = np.array(fit_M), np.array(fit_R)
    by = {(p["mesh"], p["label"]): p for p in problems}
    ok = (margins["sigma_ratio"] >= SIGMA_RATIO and margins["sigma_ratio_vote"] >= SIGMA_RATIO_VOTE and margins["dist_margin"] >= DIST_GAP and margins["sum_gap"] > SUM_GAP
          and by[(1, 7)]["refit"] and not by[(1, 2)]["refit"] and by[(1, 2)]["best_count"] > 0
          and by[(1, 40)]["by_count"] == -1 and by[(1, 40)]["best_count"] == 0 and not by[(1, 40)]["refit"]
          and all(by[(0, l)]["refit"] for l in (2, 3, 4, 5)))
    meta = dict(meshes=metas, problems=problems, seed=seed, threshold=THRESHOLD, inlier_dist=INLIER, refit_share=SHARE, n_iter=100,
                conditions=dict(sigma_ratio=SIGMA_RATIO, sigma_ratio_vote=SIGMA_RATIO_VOTE, dist_margin=DIST_GAP, sum_gap=SUM_GAP), margins=margins)
    return ok, meta, arrs


# ------------------------------------------------------------------------------------------------------------------------- k-means
def unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def kmeans_inputs(rng):
    cases = {}

    def blobs(V, D, n_blobs, dtype, codebook=None, spread=0.15, noise=0.5):
        centre = rng.integers(0, n_blobs, V)
        pos = rng.uniform(-1, 1, (n_blobs, 3))[centre] + rng.normal(size=(V, 3)) * spread
        proto = unit(rng.normal(size=(n_blobs, D)))
        if codebook:                                                           # few distinct rows: the file compresses
            book = unit(proto[rng.integers(0, n_blobs, codebook)] + rng.normal(size=(codebook, D)) * 0.3 / np.sqrt(D))
            own = [np.nonzero(np.argmax(book @ proto.T, 1) == b)[0] for b in range(n_blobs)]
            X = np.stack([book[rng.choice(own[c])] if len(own[c]) else proto[c] for c in centre])
        else:
            X = unit(proto[centre] + rng.normal(size=(V, D)) * noise / np.sqrt(D))
        return unit(X.astype(dtype)).astype(dtype), pos

    X, pos = blobs(257, 16, 6, np.float32, spread=0.45, noise=1.5)     # overlapping blobs: several iterations
    cases["v257"] = dict(X=X, verts=pos, K=6, max_iter=100)
    cases["cut"] = dict(X=X, verts=pos, K=6, max_iter=2, shares="v257")
    X, pos = blobs(1000, 64, 20, np.float32, codebook=64)
    cases["default"] = dict(X=X, verts=pos, K=20, max_iter=100)
    X, pos = blobs(120, 8, 3, np.float32)
    base = rng.uniform(-1, 1, (5, 3))                                          # 5 distinct positions, 6 seeds: two coincide
    pos = base[np.concatenate([np.arange(5), rng.integers(0, 5, 115)])]
    cases["coincident"] = dict(X=X, verts=pos, K=6, max_iter=100)
    X, pos = blobs(70, 8, 7, np.float32)
    cases["dropped"] = dict(X=X, verts=pos, K=8, max_iter=100)
    X, pos = blobs(100, 8, 4, np.float64)
    cases["f64"] = dict(X=X, verts=pos, K=5, max_iter=100)
    return cases


def run_kmeans(KMeans, seed):
    import piecewise_oracle as po
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    metas, arrs = [], {}
    margins = dict(row_margin=np.inf, fit_margin=np.inf)
    ok = True
    for ci, (name, c) in enumerate(kmeans_inputs(rng).items()):
        km = KMeans(n_clusters=c["K"], max_iter=c["max_iter"])
        mats, calc = [], km.calc_dist

        def wrapped(*a, calc=calc, mats=mats):
            out = calc(*a)
            mats.append(np.array(out, dtype=np.float64))
            return out

        km.calc_dist = wrapped
        with Recorder() as rec:
            labels = km.fit_predict(c["X"], c["verts"])
        assert len(rec.randints) == 1
        # mats: the seed matrix, one per iteration, the pruned one
        n_iter = len(mats) - 2
        fits = [m.min(axis=1).sum() for m in mats[:-1]]
        for m in mats:
            margins["row_margin"] = min(margins["row_margin"], po.row_margin(m))
        for a, b in zip(fits[:-1], fits[1:]):
            margins["fit_margin"] = min(margins["fit_margin"], float(abs(abs(a - b) - km.tol)))
        members = np.bincount(np.argmin(mats[-2], axis=1), minlength=c["K"])
        reseeds = sum(int(np.sum(np.bincount(np.argmin(m, axis=1), minlength=c["K"]) == 0)) for m in mats[:max(n_iter, 0)])
        meta = dict(name=name, V=len(c["X"]), D=c["X"].shape[1], K=c["K"], max_iter=c["max_iter"], first=rec.randints[0], n_iter=n_iter,
                    n_kept=int(len(km.centers_emb)), reseeds=reseeds, dtype=str(c["X"].dtype), shares=c.get("shares"), fit=float(fits[-1]),
                    converged=bool(n_iter < c["max_iter"]))
        seeds = km.fps_euc.__func__                                            # the seeds again, from the recorded first draw
        np_randint = np.random.randint
        np.random.randint = lambda *a, **k: rec.randints[0]
        try:
            seed_idx = np.array(seeds(km, c["verts"]), dtype=np.int64)
        finally:
            np.random.randint = np_randint
        if c.get("shares") is None:
            arrs.update({f"c{ci}_X": c["X"], f"c{ci}_verts": c["verts"]})
        arrs.update({f"c{ci}_labels": np.asarray(labels, dtype=np.int64), f"c{ci}_seeds": seed_idx, f"c{ci}_members": members.astype(np.int64),
                     f"c{ci}_centres_emb": np.asarray(km.centers_emb), f"c{ci}_centres_euc": np.asarray(km.centers_euc),
                     f"c{ci}_last_labels": np.argmin(mats[-2], axis=1).astype(np.int64)})
        metas.append(meta)
        if name == "coincident":
            ok &= reseeds > 0 and len(np.unique(c["verts"][seed_idx], axis=0)) < c["K"]
        if name == "dropped":
            ok &= meta["n_kept"] < c["K"] and bool(np.any(members <= 8))
        if name == "cut":                                                      # the same start without the cut needs more iterations
            full = KMeans(n_clusters=c["K"], max_iter=100)
            count, calc_full = [], full.calc_dist
            full.calc_dist = lambda *a: (count.append(0), calc_full(*a))[1]
            np.random.randint = lambda *a, **k: rec.randints[0]
            try:
                full.fit_predict(c["X"], c["verts"])
            finally:
                np.random.randint = np_randint
            meta["n_iter_uncut"] = len(count) - 2
            ok &= n_iter == 2 and meta["n_iter_uncut"] > 2
        if name in ("v257", "default", "f64"):
            ok &= meta["converged"]
    ok &= margins["row_margin"] >= ROW_MARGIN and margins["fit_margin"] >= FIT_MARGIN
    meta = dict(cases=metas, seed=seed, w_euc=0.2, tol=1e-4, conditions=dict(row_margin=ROW_MARGIN, fit_margin=FIT_MARGIN), margins=margins)
    return ok, meta, arrs


def main():
    Ransac, KMeans = reference()
    for name, run, cls in (("piecewise_ransac", run_ransac, Ransac), ("piecewise_kmeans", run_kmeans, KMeans)):
        for seed in range(20261018, 20261018 + 200):
            ok, meta, arrs = run(cls, seed)
            if ok:
                break
            print(f"  {name}: seed {seed} misses a condition: {meta['margins']}")
        else:
            raise SystemExit(f"{name}: no admissible seed")
        print(f"  {name}: seed {seed}, margins {meta['margins']}")
        msg.save(name, meta, **arrs)


if __name__ == "__main__":
    main()
