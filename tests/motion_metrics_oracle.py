"""The numpy statement of morig_amd/motion_metrics.py, written as per-mesh loops so that it reads like the reference's
scripts (evaluate/eval_corr.py:17-22, eval_attn.py:21, 31-36, eval_deform.py:18-19), with every dtype and cast explicit so that it does not
depend on the numpy that runs it:

  1. the correspondence distance is float32: d = a - b per component, (d0^2 + d1^2) + d2^2, np.sqrt in float32 (correctly rounded); a hit is
     dist < np.float32(tol);
  2. the attention values are normalised per mesh in float32, (x - mn) / (mx - mn) with np.min's NaN rule; a predicted positive is
     x' > np.float32(t) -- the comparison of the reference's numpy 1.21, where numpy 2 would compare an np.float64 threshold in float64;
  3. counts are integers;
  4. ratios and means are float64, from the counts.
"""
import numpy as np

TOLERANCES = [0.02, 0.04, 0.06, 0.08, 0.10, 0.12, 0.14, 0.16, 0.18, 0.20]
THRESHOLDS = np.arange(0.0, 1.0, 0.1)


def f32(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32)


def corr_distance(pts, nnind, corr):
    """float32 [n]: |pts[nnind[v]] - pts[p_gt]| per correspondence row, in the order numpy adds the three squares"""
    pts = np.asarray(pts)
    assert pts.dtype == np.float32
    pred_pos = pts[np.asarray(nnind)[corr[:, 0]]]
    gt_pos = pts[corr[:, 1]]
    d = (pred_pos - gt_pos).astype(np.float32)
    sq = (d * d).astype(np.float32)
    s = ((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32)
    return np.sqrt(s).astype(np.float32)


def corr_hits(pts, nnind, corr, tolerances=TOLERANCES):
    """one pair -> int64 [n_tol]"""
    dist = corr_distance(pts, nnind, np.asarray(corr, dtype=np.int64).reshape(-1, 2))
    return np.array([int((dist < t).sum()) for t in f32(tolerances)], dtype=np.int64)


def corr_accuracy(pairs, tolerances=TOLERANCES):
    """pairs: list of (pts float32 [P, 3], nnind [V], corr [n, 2]) -> the dict of motion_metrics.corr_accuracy"""
    n_tol = len(tolerances)
    hits = np.zeros((len(pairs), n_tol), dtype=np.int64)
    count = np.zeros(len(pairs), dtype=np.int64)
    acc = np.zeros((len(pairs), n_tol), dtype=np.float64)
    curve, n_valid = np.zeros(n_tol), 0
    for b, (pts, nnind, corr) in enumerate(pairs):
        hits[b], count[b] = corr_hits(pts, nnind, corr, tolerances), len(corr)
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(n_tol):
                acc[b, i] = np.float64(hits[b, i]) / np.float64(count[b]) * 100.0
        if count[b] > 0:
            curve += acc[b]
            n_valid += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        curve = curve / np.float64(n_valid)
    return dict(hits=hits, count=count, acc=acc, curve=curve, n_valid=n_valid)


def normalised(pred):
    pred = np.asarray(pred)
    assert pred.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        mn, mx = np.min(pred), np.max(pred)                      # NaN as soon as one value is NaN
        return ((pred - mn).astype(np.float32) / np.float32(mx - mn)).astype(np.float32)


def pr_counts(pred, gt, thresholds=THRESHOLDS, normalize=True):
    """one mesh -> (tp int64 [n_thr], pp int64 [n_thr], gp int)"""
    pred = np.asarray(pred).reshape(-1)
    x = normalised(pred) if normalize else pred.astype(np.float32)
    g = np.asarray(gt).reshape(-1) != 0
    tp, pp = [], []
    for t in f32(thresholds):
        with np.errstate(invalid="ignore"):
            above = x > t                                        # float32 against float32
        pp.append(int(above.sum()))
        tp.append(int((above & g).sum()))
    return np.array(tp, dtype=np.int64), np.array(pp, dtype=np.int64), int(g.sum())


def pr_curve(meshes, thresholds=THRESHOLDS, normalize=True):
    """meshes: list of (pred float32 [V], gt [V]) -> the dict of motion_metrics.pr_curve"""
    n_thr, B = len(thresholds), len(meshes)
    tp, pp, gp = np.zeros((B, n_thr), dtype=np.int64), np.zeros((B, n_thr), dtype=np.int64), np.zeros(B, dtype=np.int64)
    precision, recall = np.zeros((B, n_thr)), np.zeros((B, n_thr))
    mean_precision, mean_recall = np.zeros(n_thr), np.zeros(n_thr)
    for b, (pred, gt) in enumerate(meshes):
        tp[b], pp[b], gp[b] = pr_counts(pred, gt, thresholds, normalize)
        for i in range(n_thr):
            precision[b, i] = tp[b, i] / (pp[b, i] + 1e-6)
            recall[b, i] = tp[b, i] / (gp[b] + 1e-6)
        mean_precision += precision[b]
        mean_recall += recall[b]
    return dict(tp=tp, pp=pp, gp=gp, precision=precision, recall=recall, mean_precision=mean_precision / B, mean_recall=mean_recall / B)


def keyframe_flow_errors(meshes):
    """meshes: list of (pred_flow [V, 3 K], gt_flow [V, 3 K]) -> (float64 [B, K], float64 [B]) in float64"""
    K = meshes[0][0].shape[1] // 3
    per_frame = np.zeros((len(meshes), K))
    for b, (pred, gt) in enumerate(meshes):
        p, g = np.asarray(pred, dtype=np.float64).reshape(-1, K, 3), np.asarray(gt, dtype=np.float64).reshape(-1, K, 3)
        d = g - p
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        with np.errstate(invalid="ignore"):
            per_frame[b] = dist.sum(axis=0) / np.float64(len(p))
    total = per_frame[:, 0].copy()
    for t in range(1, K):
        total += per_frame[:, t]
    return per_frame, total / np.float64(K)


# ------------------------------------------------------------------------------------------------------------------ generated cases
def float32_at_distance(rng, target):
    """two float32 points whose rule-1 distance is exactly np.float32(target): along one axis, from the origin"""
    t = np.float32(target)
    a = np.zeros(3, dtype=np.float32)
    b = np.zeros(3, dtype=np.float32)
    b[int(rng.integers(0, 3))] = t                                # sqrt(float32(t * t)) == t for the t in use (asserted by corr_pair)
    return a, b


def corr_pair(seed, n_pts, n_vtx, n_corr, exact=()):
    """one pair: points in the unit box, nnind random, correspondences random with predicted points near their ground truth (so that all
    tolerances see hits and misses). ``exact``: tolerances whose value some row's distance equals exactly (two extra points each)."""
    rng = np.random.default_rng([0x6D6F7469, seed])
    pts = rng.random((n_pts, 3)).astype(np.float32)
    nnind = rng.integers(0, n_pts, n_vtx)
    corr = np.stack([rng.integers(0, n_vtx, n_corr), rng.integers(0, n_pts, n_corr)], 1).astype(np.int64)
    # half the rows: move the predicted point of the row's vertex close to the ground truth, at a distance spread over the tolerances
    for r in range(0, n_corr, 2):
        v, p = corr[r]
        q = int(nnind[v])
        if q != p:
            step = rng.normal(size=3)
            pts[q] = (pts[p] + (step / np.linalg.norm(step) * rng.uniform(0.0, 0.25)).astype(np.float32)).astype(np.float32)
    for k, t in enumerate(exact):
        if n_pts >= 2 * (k + 1) and n_vtx > k and n_corr > k:
            a, b = float32_at_distance(rng, t)
            ia, ib = n_pts - 1 - 2 * k, n_pts - 2 - 2 * k
            pts[ia], pts[ib] = a, b
            nnind[k] = ia
            corr[k] = (k, ib)
            assert corr_distance(pts, nnind, corr[k:k + 1])[0] == np.float32(t)
    return pts, nnind.astype(np.int64), corr


def contraction_pair(n_rows=32, seed=0):
    """One pair that tells rule 1 from a fused multiply-add: n_rows point pairs (origin, q) for which (d0^2 + d1^2) + d2^2 with every
    product rounded gives another float32 distance than fma(d2, d2, fma(d1, d1, d0^2)), and per row one tolerance, the larger of the two
    distances: exactly one of the two arithmetics is below it. -> (pts, nnind, corr, tolerances float32 [n_rows])"""
    rng = np.random.default_rng([0x666D6163, seed])
    rows, tol = [], []
    while len(rows) < n_rows:
        q = rng.uniform(0.01, 0.2, 3).astype(np.float32)
        sq = (q * q).astype(np.float32)
        plain = np.sqrt(((sq[0] + sq[1]).astype(np.float32) + sq[2]).astype(np.float32))
        inner = np.float32(np.float64(q[1]) * np.float64(q[1]) + np.float64(sq[0]))
        fused = np.sqrt(np.float32(np.float64(q[2]) * np.float64(q[2]) + np.float64(inner)))
        if plain != fused:
            rows.append(q)
            tol.append(max(plain, fused))
    pts = np.concatenate([np.zeros((1, 3), dtype=np.float32), np.array(rows, dtype=np.float32)])
    nnind = np.zeros(n_rows, dtype=np.int64)                                     # every vertex predicts the origin
    corr = np.stack([np.arange(n_rows), np.arange(1, n_rows + 1)], 1).astype(np.int64)
    return pts, nnind, corr, np.array(tol, dtype=np.float32)


def attn_mesh(seed, n, kind="random", thresholds=THRESHOLDS):
    """one mesh of pr_curve: (pred float32 [n], gt float64 [n] of 0 / 1). kinds: random; at_threshold (values 0, 1 and every float32(t), so
    that normalising leaves them as they are and x' == float32(t) occurs); constant; nan (one NaN); all_false / all_true (the labels)"""
    rng = np.random.default_rng([0x6174746E, seed])
    pred = rng.random(n).astype(np.float32)
    gt = (rng.random(n) < 0.4).astype(np.float64)
    if kind == "at_threshold":
        vals = np.concatenate([[0.0, 1.0], f32(thresholds)]).astype(np.float32)
        pred[:min(n, len(vals))] = vals[:min(n, len(vals))]
    elif kind == "constant":
        pred[:] = np.float32(0.37)
    elif kind == "nan":
        pred[n // 2] = np.nan
    elif kind == "all_false":
        gt[:] = 0.0
    elif kind == "all_true":
        gt[:] = 2.0                                               # non-zero reads as True
    return pred, gt


def feature_pair(seed, n_vtx, n_pts, gap=1e-3):
    """unit float32 rows [n_vtx, 64] and [n_pts, 64] such that for EVERY vertex the best similarity exceeds the second best by at least
    ``gap`` in float64 (checked; rows are re-drawn until it holds) -> (vtx_f, pts_f, the float64 arg-max int64 [n_vtx])"""
    rng = np.random.default_rng([0x66656174, seed])
    pts_f = rng.normal(size=(n_pts, 64))
    pts_f = (pts_f / np.linalg.norm(pts_f, axis=1, keepdims=True)).astype(np.float32)
    vtx_f = np.zeros((n_vtx, 64), dtype=np.float32)
    best = np.zeros(n_vtx, dtype=np.int64)
    for v in range(n_vtx):
        while True:
            target = int(rng.integers(0, n_pts))
            row = pts_f[target].astype(np.float64) + 0.35 * rng.normal(size=64) / 8.0
            row = (row / np.linalg.norm(row)).astype(np.float32)
            sim = pts_f.astype(np.float64) @ row.astype(np.float64)
            order = np.argsort(-sim)
            if n_pts == 1 or sim[order[0]] - sim[order[1]] >= gap:
                vtx_f[v], best[v] = row, order[0]
                break
    return vtx_f, pts_f, best


def similarity_gaps(vtx_f, pts_f):
    """float64 [n_vtx]: best minus second-best similarity (inf with one point)"""
    sim = np.asarray(vtx_f, dtype=np.float64) @ np.asarray(pts_f, dtype=np.float64).T
    if sim.shape[1] < 2:
        return np.full(len(sim), np.inf)
    top = -np.sort(-sim, axis=1)[:, :2]
    return top[:, 0] - top[:, 1]


def pack(parts, dtype=None):
    """list of per-segment arrays -> (concatenated rows, int64 batch vector)"""
    rows = np.concatenate([np.asarray(p) for p in parts], axis=0)
    batch = np.concatenate([np.full(len(p), b, dtype=np.int64) for b, p in enumerate(parts)])
    return (rows.astype(dtype) if dtype is not None else rows), batch
