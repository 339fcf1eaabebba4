"""NumPy float64 restatement of the rig-free tracker (morig_amd/piecewise.py, csrc/piecewise.hip), written from the description in
DESIGN.md section 17: the piecewise RANSAC and the kernel k-means. No code of the reference, nothing of morig_amd, no GPU, and no library
SVD: the rigid fit is Horn's quaternion form with this file's own cyclic Jacobi sweeps. Besides the results it returns the intermediate
values the fixture conditions are stated on (tests/test_piecewise_oracle.py re-checks them).

Every function that computes takes ``dtype`` (float64 by default): the same text runs in ``np.longdouble`` (a 64-bit mantissa on x86-64),
which is the yardstick of tests/piecewise_cases.py. The sums whose ORDER the device documents are spelled out here and do not rest on
how numpy reduces: a cluster's centre adds its members' rows in ascending vertex order, the embedding product adds its D terms from left
to right."""
import numpy as np

MIN_HANDLES = 4


# ---------------------------------------------------------------------------------------------------------------------- the rigid fit
def jacobi_eigh(A, sweeps=32, dtype=np.float64):
    """symmetric [n, n] -> (eigenvalues, eigenvectors in columns), cyclic Jacobi rotations in the order (0,1), (0,2), ... (n-2,n-1)"""
    A = np.array(A, dtype=dtype)
    n = len(A)
    V = np.eye(n, dtype=dtype)
    for _ in range(sweeps):
        if np.sum(np.abs(A[np.triu_indices(n, 1)])) == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if A[p, q] == 0.0:
                    continue
                g = 100.0 * abs(A[p, q])
                if abs(A[p, p]) + g == abs(A[p, p]) and abs(A[q, q]) + g == abs(A[q, q]):
                    A[p, q] = A[q, p] = 0.0
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(n, dtype=dtype)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                V = V @ J
    return np.diag(A).copy(), V


def horn(M, dtype=np.float64):
    """M = tar_c^T src_c [3, 3] -> (the proper rotation R with tar ~ R src, singular values (s1, s2, d * s3) of M read off the spectrum)"""
    S = np.asarray(M, dtype=dtype).T                       # S[a, b] = sum src_a tar_b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]], dtype=dtype)
    lam, vec = jacobi_eigh(N, dtype=dtype)
    w, x, y, z = vec[:, int(np.argmax(lam))] / np.linalg.norm(vec[:, int(np.argmax(lam))])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=dtype)
    l = np.sort(lam)[::-1]                                       # s1+s2+ds3, s1-s2-ds3, -s1+s2-ds3, -s1-s2+ds3
    return R, np.array([(l[0] + l[1]) / 2, (l[0] + l[2]) / 2, (l[0] + l[3]) / 2], dtype=dtype)


def covariance(src, tar):
    return (tar - tar.mean(axis=0)).T @ (src - src.mean(axis=0))


def rigid_fit(src, tar, dtype=np.float64):
    """-> (R, t, singular values): tar ~ src R^T + t; t is the mean of tar - src R^T over the fitted points"""
    src, tar = np.asarray(src, dtype=dtype), np.asarray(tar, dtype=dtype)
    R, sv = horn(covariance(src, tar), dtype)
    return R, (tar - src @ R.T).mean(axis=0), sv


# ---------------------------------------------------------------------------------------------------------------------- RANSAC
def renumber(seg):
    """labels -> ranks among the labels present"""
    return np.unique(np.asarray(seg), return_inverse=True)[1].reshape(-1)


def segment_handles(vismask, seg, threshold):
    """-> (rank labels, [handle indices of every rank, ascending])"""
    rank = renumber(seg)
    kept = np.asarray(vismask, dtype=np.float64) >= threshold                  # the mask is promoted before it is compared
    return rank, [np.nonzero(kept & (rank == l))[0] for l in range(int(rank.max()) + 1 if len(rank) else 0)]


def select(counts, sums):
    """the two running selections -> (by_count or -1, by_sum or -1, best count)"""
    best, by_count, err, by_sum = 0, -1, 1e10, -1
    for i in range(len(counts)):
        if counts[i] > best:
            best, by_count = int(counts[i]), i
        if sums[i] < err:
            err, by_sum = sums[i], i
    return by_count, by_sum, best


def ransac_segment(src, tar, samples, inlier_dist=5e-2, refit_share=0.35, dtype=np.float64):
    """one problem: src, tar [H, 3] handle positions, samples [n_iter, 3] -> dict with every decision and the margins. ``inliers``: the
    positions in the handle list that the hypothesis with the largest count holds below the inlier distance (empty without one)."""
    src, tar = np.asarray(src, dtype=dtype), np.asarray(tar, dtype=dtype)
    n_iter = len(samples)
    counts, sums = np.zeros(n_iter, dtype=np.int64), np.zeros(n_iter, dtype=dtype)
    fits, dists, ratios = [], [], []
    for i, s in enumerate(samples):
        R, t, sv = rigid_fit(src[s], tar[s], dtype)
        d = np.sqrt(np.sum((src @ R.T + t - tar) ** 2, axis=1))
        counts[i], sums[i] = int(np.sum(d < inlier_dist)), d.sum()
        fits.append((R, t))
        dists.append(d)
        ratios.append(sv[1] / sv[0] if sv[0] > 0 else 0.0)
    by_count, by_sum, best = select(counts, sums)
    refit = by_count >= 0 and best > refit_share * len(src)
    inl = np.nonzero(dists[by_count] < inlier_dist)[0] if by_count >= 0 else np.zeros(0, dtype=np.int64)
    if refit:
        R, t, sv = rigid_fit(src[inl], tar[inl], dtype)
        used = min(sv[1] / sv[0], (sv[1] + sv[2]) / sv[0])
    elif by_sum >= 0:
        R, t = fits[by_sum]
        used = ratios[by_sum]
    else:
        R, t, used = None, None, 0.0
    two = np.sort(sums)[:2]
    return dict(counts=counts, sums=sums, by_count=by_count, by_sum=by_sum, best_count=best, refit=bool(refit), R=R, t=t,
                sigma_ratio=float(used), sigma_ratio_vote=float(min(ratios)), dist_margin=float(np.min(np.abs(np.array(dists) - inlier_dist))),
                sum_gap=float((two[1] - two[0]) / two[1]) if len(two) == 2 and two[1] > 0 else np.inf, inliers=inl,
                hyp_R=np.array([f[0] for f in fits]), hyp_t=np.array([f[1] for f in fits]))


def piecewise_ransac(vert_src, vert_dst, vismask, seg, samples, threshold=0.3, inlier_dist=5e-2, refit_share=0.35, dtype=np.float64,
                     unfitted="raise"):
    """one mesh; samples: one [n_iter, 3] array per segment with >= 4 handles, ranks ascending -> (moved vertices, details per problem).
    ``unfitted="keep"``: a problem without a hypothesis stays in the details (R None) and its vertices stay, where the default raises."""
    src, dst = np.asarray(vert_src, dtype=dtype), np.asarray(vert_dst, dtype=dtype)
    out = src.copy()
    rank, handles = segment_handles(vismask, seg, threshold)
    labels = np.unique(np.asarray(seg))
    details, p = [], 0
    for l, h in enumerate(handles):
        members = rank == l
        if len(h) < MIN_HANDLES:
            out[members] = dst[members]
            continue
        d = ransac_segment(src[h], dst[h], np.asarray(samples[p]), inlier_dist, refit_share, dtype)
        p += 1
        if d["R"] is None and unfitted != "keep":
            raise ValueError(f"label {labels[l]}: no hypothesis has a distance sum below 1e10")
        if d["R"] is not None:
            out[members] = src[members] @ d["R"].T + d["t"]
        d.update(label=int(labels[l]), handles=h)
        details.append(d)
    return out, details


# ---------------------------------------------------------------------------------------------------------------------- k-means
def fps(verts, K, first, dtype=np.float64):
    """farthest-point seeds: squared distances as (dx*dx + dy*dy) + dz*dz, the first index of the maximum"""
    v = np.asarray(verts, dtype=dtype)
    sq = lambda i: ((v[i, 0] - v[:, 0]) ** 2 + (v[i, 1] - v[:, 1]) ** 2) + (v[i, 2] - v[:, 2]) ** 2
    seeds = np.zeros(K, dtype=np.int64)
    seeds[0] = first
    d = sq(first)
    for k in range(1, K):
        seeds[k] = int(np.argmax(d))
        d = np.minimum(d, sq(seeds[k]))
    return seeds


def kdist(X64, v, cemb, ceuc, w_euc):
    """[V, K] distances; the embedding product adds its D terms from left to right, starting from 0"""
    diff = v[:, None, :] - ceuc[None, :, :]
    euc = np.sqrt((diff[..., 0] ** 2 + diff[..., 1] ** 2) + diff[..., 2] ** 2)
    dot = np.zeros((len(X64), len(cemb)), dtype=X64.dtype)
    for j in range(X64.shape[1]):
        dot += X64[:, j, None] * cemb[None, :, j]
    return euc * w_euc + np.maximum(1.0 - dot, 0.0) / 2.0


def ordered_sum(rows, ids):
    """rows[ids[0]] + rows[ids[1]] + ... from 0, one row after the other: the order of the device's centre update"""
    acc = np.zeros(rows.shape[1], dtype=rows.dtype)
    for i in ids:
        acc = acc + rows[i]
    return acc


def column_margin(col):
    """the gap between a column's minimum and its nearest value that is not bitwise equal to it (inf for a column of equal values)"""
    rest = col[col != col.min()]
    return float(rest.min() - col.min()) if len(rest) else np.inf


def row_margin(dist):
    """the smallest gap between a row's minimum and its nearest value that is not bitwise equal to it (identical centres give identical
    columns: the first wins in every implementation)"""
    low = dist.min(axis=1, keepdims=True)
    rest = np.where(dist == low, np.inf, dist)
    return float(np.min(rest.min(axis=1) - low[:, 0]))


def kernel_kmeans(X, verts, n_clusters=20, max_iter=100, w_euc=0.2, tol=1e-4, first=0, dtype=np.float64):
    """one mesh -> (labels over the kept clusters, state). All arithmetic in ``dtype``; the embedding centres are rounded to X's type. No
    cluster kept: labels of -1 and n_kept 0, as the device reports. ``reseeded``: (iteration, cluster) of every reseed; ``reseed_margin``:
    the smallest gap by which a reseed's vertex was the nearest."""
    X = np.asarray(X)
    X64, v = X.astype(dtype), np.asarray(verts, dtype=dtype)
    seeds = fps(v, n_clusters, first, dtype)
    cemb, ceuc = X64[seeds].copy(), v[seeds].copy()
    dist = kdist(X64, v, cemb, ceuc, w_euc)
    fit_last = dist.min(axis=1).sum()
    margin, fit_margin, reseeds, n_iter = row_margin(dist), np.inf, 0, 0
    reseeded, reseed_margin = [], np.inf
    for it in range(max_iter):
        label, nearest = dist.argmin(axis=1), dist.argmin(axis=0)
        for k in range(n_clusters):
            ids = np.nonzero(label == k)[0]
            if len(ids) == 0:
                cemb[k], ceuc[k] = X64[nearest[k]], v[nearest[k]]
                reseeds += 1
                reseeded.append((it, k))
                reseed_margin = min(reseed_margin, column_margin(dist[:, k]))
            else:
                cemb[k] = (ordered_sum(X64, ids) / len(ids)).astype(X.dtype).astype(dtype)
                ceuc[k] = ordered_sum(v, ids) / len(ids)
        dist = kdist(X64, v, cemb, ceuc, w_euc)
        fit_this = dist.min(axis=1).sum()
        margin = min(margin, row_margin(dist))
        delta = abs(fit_last - fit_this)
        fit_margin = min(fit_margin, abs(delta - tol))
        n_iter = it + 1
        fit_last = fit_this
        if delta < tol:
            break
    label = dist.argmin(axis=1)
    members = np.bincount(label, minlength=n_clusters)
    kept = np.nonzero(members > 8)[0]
    state = dict(seeds=seeds, n_iter=n_iter, n_kept=len(kept), members=members, centres_emb=cemb, centres_euc=ceuc, fit=float(fit_last),
                 row_margin=margin, fit_margin=float(fit_margin), reseeds=reseeds, last_labels=label, reseeded=reseeded,
                 reseed_margin=reseed_margin)
    if len(kept) == 0:
        return np.full(len(X64), -1, dtype=np.int64), state
    final = kdist(X64, v, cemb[kept], ceuc[kept], w_euc)
    state["row_margin"] = min(margin, row_margin(final))
    return final.argmin(axis=1), state
