"""Tracking a mesh that has no rig: the reference's ``Piecewise_RANSAC`` (utils/piecewise_ransac.py) -- every segment of the mesh is
fitted rigidly to DeformNet's target by RANSAC voting -- and ``KernelKMeans`` (utils/kernel_kmeans.py), its segment source when no
skeleton exists: a k-means on the motion embedding plus position, seeded by farthest-point sampling. ``eval_tracking.plot`` draws the
result as the "none" curve beside the rigged ones.

Every function takes lists with one entry per mesh (numpy arrays or tensors, on any device) and runs the batch in a fixed number of
launches of csrc/piecewise.hip; the results are device tensors. ALL arithmetic is float64: float32 inputs are promoted on entry, where
the reference would stay in float32 (its k-means then multiplies float32 embeddings; the only float32 kept here is the rounding of the
embedding centres, which the reference stores in X's type). Sums have a fixed order and nothing uses floating-point atomics, so two runs
give the same bits and a mesh alone gives the bits it gives inside a batch.

    draw_ransac_samples   the reference's sample draws, in its order, from a numpy RandomState (host)
    piecewise_ransac      Piecewise_RANSAC.run
    kernel_kmeans         KernelKMeans.fit_predict
    segments_from_skins   np.argmax(rig.skins, axis=1), the segments of a mesh that has a rig
    (tracking.track_piecewise is the frame loop over these.)

The rigid fit (csrc/kabsch_core.h) is unique while the fitted points are not collinear; collinear or coincident samples have several best
rotations and this module may return another of them than numpy's SVD does.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .ragged import as_tensor, cat_to, device_of, ptr_of
from .runtime import get_ops

N_ITER = 100                    # range(100) of ransac_voting
INLIER_DIST = 5e-2
REFIT_SHARE = 0.35
MIN_HANDLES = 4
KMEANS_MAX_CLUSTERS = 64        # MORIG_KMEANS_MAX_CLUSTERS / MORIG_KMEANS_MAX_DIM of include/morig_hip.h
KMEANS_MAX_DIM = 128


# ------------------------------------------------------------------------------------------------------------------- the sample draws
def draw_ransac_samples(handle_counts: Sequence[int], n_iter: int = N_ITER, rng=None) -> np.ndarray:
    """The draws of a reference run: ``handle_counts`` are the handle counts of all segments in the reference's order (mesh after mesh,
    renumbered labels ascending); a segment with fewer than 4 handles draws nothing, every other one ``n_iter`` times
    ``np.random.choice(range(n), 3, replace=False)`` -- for numpy's legacy generator that is ``permutation(n)[:3]``. ``rng``: an
    ``np.random.RandomState``; None: numpy's global one, so that ``np.random.seed(s)`` before the call reproduces the reference run that
    was seeded alike. -> int32 [n_problems, n_iter, 3] positions in each problem's handle list (a host array: the draws are host work)."""
    rng = np.random if rng is None else rng
    counts = [int(c) for c in np.asarray(handle_counts).reshape(-1)]
    solved = [c for c in counts if c >= MIN_HANDLES]
    out = np.zeros((len(solved), int(n_iter), 3), dtype=np.int32)
    for p, n in enumerate(solved):
        for i in range(int(n_iter)):
            out[p, i] = rng.permutation(n)[:3]
    return out


# ------------------------------------------------------------------------------------------------------------------- the plumbing
class RansacPlan:
    """The tables of one batch, all on the device but ``handle_counts`` (THE host read): per segment its mesh, label and handle count in
    the reference's order; ``problem_of`` int32 [N] the problem of every vertex (-1: its segment has < 4 handles); ``handles`` int32 rows
    of the batch in CSR form by ``hptr``; ``problem_segment`` the segment of every problem."""

    def __init__(self, vismask: torch.Tensor, seg: torch.Tensor, mesh_of: torch.Tensor, threshold: float):
        dev = seg.device
        keys, sid = torch.unique(torch.stack([mesh_of, seg], 1), dim=0, return_inverse=True)     # sorted by (mesh, label): the renumbering
        S = keys.shape[0]
        kept = vismask >= threshold
        n_handles = torch.bincount(sid[kept], minlength=S)
        self.handle_counts = n_handles.cpu().numpy()                                            # the one host read
        self.segment_mesh, self.segment_label = keys[:, 0], keys[:, 1]
        solved = n_handles >= MIN_HANDLES
        problem_of_seg = torch.where(solved, torch.cumsum(solved.long(), 0) - 1, torch.full_like(n_handles, -1))
        self.problem_of = problem_of_seg[sid].to(torch.int32).contiguous()
        rows = torch.nonzero(kept & solved[sid]).reshape(-1)
        order = torch.sort(sid[rows], stable=True).indices                                       # ascending vertex inside a segment
        self.handles = rows[order].to(torch.int32).contiguous()
        counts = self.handle_counts[self.handle_counts >= MIN_HANDLES]
        self.hptr = torch.from_numpy(ptr_of(counts).astype(np.int32)).to(dev)
        self.problem_segment = np.nonzero(self.handle_counts >= MIN_HANDLES)[0]
        self.n_problems = len(counts)


def piecewise_ransac(vert_src: Sequence, vert_dst: Sequence, vismask: Sequence, seg: Sequence, vismask_threshold: float = 0.3,
                     samples=None, rng=None, n_iter: int = N_ITER, inlier_dist: float = INLIER_DIST, refit_share: float = REFIT_SHARE,
                     details: Optional[list] = None) -> List[torch.Tensor]:
    """``Piecewise_RANSAC(vismask_threshold).run`` for a list of meshes: vert_src / vert_dst [V, 3], vismask [V], seg [V] integer labels
    (any integers, interleaved as they come; they are renumbered by rank). A segment's handles are its vertices with vismask >=
    threshold in ascending vertex order; with fewer than 4 the segment copies vert_dst; otherwise ``n_iter`` hypotheses are fitted to 3
    sampled handles each, and the segment moves by the refit to the inliers (distance < inlier_dist) of the hypothesis with the most
    inliers when those exceed refit_share of the handles, else by the hypothesis with the smallest distance sum.
    ``samples``: int32 [n_problems, n_iter, 3] as draw_ransac_samples gives; None: drawn here from ``rng``.
    -> float64 [V, 3] per mesh on the device, NEW tensors (the reference overwrites vert_src). Positions and the mask are promoted to
    float64 (the reference would fit float32 inputs in float32). ``details``: a list that receives per problem dict(mesh, label, handles,
    by_count, by_sum, best_count, refit, R, t, counts, sums). Raises ValueError where the reference would end on ``R = None`` (no
    hypothesis with a distance sum below 1e10)."""
    n = len(vert_src)
    if not (len(vert_dst) == len(vismask) == len(seg) == n):
        raise ValueError("piecewise_ransac: one entry per mesh in every list")
    if n == 0:
        return []
    dev = device_of(*vert_src, *vert_dst)
    sizes = [len(v) for v in vert_src]
    if any(len(vert_dst[m]) != sizes[m] or len(vismask[m]) != sizes[m] or len(seg[m]) != sizes[m] for m in range(n)):
        raise ValueError("piecewise_ransac: vert_dst, vismask and seg have one row per vertex of vert_src")
    src = cat_to([as_tensor(v).reshape(-1, 3) for v in vert_src], dev, torch.float64)
    dst = cat_to([as_tensor(v).reshape(-1, 3) for v in vert_dst], dev, torch.float64)
    vis = cat_to([as_tensor(v).reshape(-1) for v in vismask], dev, torch.float64)
    labels = cat_to([as_tensor(v).reshape(-1) for v in seg], dev, torch.int64)
    vptr = ptr_of(sizes)
    mesh_of = torch.repeat_interleave(torch.arange(n, device=dev), torch.as_tensor(sizes, device=dev))
    plan = RansacPlan(vis, labels, mesh_of, float(vismask_threshold))
    if samples is None:
        samples = draw_ransac_samples(plan.handle_counts, n_iter, rng)
    samples = np.ascontiguousarray(np.asarray(samples.cpu() if isinstance(samples, torch.Tensor) else samples), dtype=np.int32)
    if samples.ndim != 3 or samples.shape[0] != plan.n_problems or samples.shape[2] != 3:
        raise ValueError(f"piecewise_ransac: samples of shape {samples.shape} for {plan.n_problems} segments with at least 4 handles")
    counts = plan.handle_counts[plan.problem_segment]
    if samples.size and (samples.min() < 0 or (samples >= counts[:, None, None]).any()):
        raise ValueError("piecewise_ransac: a sample names no handle of its segment")
    d_samples = torch.from_numpy(samples).to(dev)
    ops = get_ops()
    if plan.n_problems:
        count, dsum = ops.ransac_vote(src, dst, plan.handles, plan.hptr, d_samples, inlier_dist)
        chosen, best, flag, Rt = ops.ransac_fit(src, dst, plan.handles, plan.hptr, d_samples, count, dsum, inlier_dist, refit_share)
    else:
        count = torch.zeros(0, samples.shape[1], dtype=torch.int32, device=dev)
        dsum = torch.zeros(0, samples.shape[1], dtype=torch.float64, device=dev)
        chosen, best = torch.zeros(0, 2, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        flag, Rt = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 12, dtype=torch.float64, device=dev)
    out = ops.ransac_apply(src, dst, plan.problem_of, flag, Rt)
    none = torch.nonzero(flag == ops.RANSAC_NONE).reshape(-1)
    if none.numel():
        s = plan.problem_segment[int(none[0])]
        raise ValueError(f"piecewise_ransac: mesh {int(plan.segment_mesh[s])}, label {int(plan.segment_label[s])}: no hypothesis has a "
                         "distance sum below 1e10 (the reference ends on R = None)")
    if details is not None:
        h_chosen, h_best, h_flag, h_Rt = chosen.cpu().numpy(), best.cpu().numpy(), flag.cpu().numpy(), Rt.cpu().numpy()
        h_handles, h_ptr, h_count, h_sum = plan.handles.cpu().numpy(), plan.hptr.cpu().numpy(), count.cpu().numpy(), dsum.cpu().numpy()
        seg_mesh, seg_label = plan.segment_mesh.cpu().numpy(), plan.segment_label.cpu().numpy()
        for p, s in enumerate(plan.problem_segment):
            m = int(seg_mesh[s])
            details.append(dict(mesh=m, label=int(seg_label[s]), handles=h_handles[h_ptr[p]:h_ptr[p + 1]].astype(np.int64) - vptr[m],
                                by_count=int(h_chosen[p, 0]), by_sum=int(h_chosen[p, 1]), best_count=int(h_best[p]),
                                refit=bool(h_flag[p] == ops.RANSAC_REFIT), R=h_Rt[p, :9].reshape(3, 3).copy(), t=h_Rt[p, 9:].copy(),
                                counts=h_count[p].copy(), sums=h_sum[p].copy()))
    return [out[vptr[m]:vptr[m + 1]] for m in range(n)]


# ------------------------------------------------------------------------------------------------------------------- k-means
def kernel_kmeans(X: Sequence, verts: Sequence, n_clusters: int = 20, max_iter: int = 100, w_euc: float = 0.2, tol: float = 1e-4, first=None,
                  rng=None, return_state: bool = False):
    """``KernelKMeans(n_clusters, max_iter, w_euc, tol).fit_predict(X, verts)`` for a list of meshes: X [V, D] unit embeddings (float32
    or float64, one type per batch), verts [V, 3]. Seeds: farthest-point sampling on the positions from ``first[m]`` (None: one
    ``randint(V)`` per mesh from ``rng``, an ``np.random.RandomState``, or numpy's global generator) -- bit-equal to the reference's. The
    distance is w_euc * |v - c_euc| + max(1 - x . c_emb, 0) / 2. Per iteration: row arg-min labels; an empty cluster is reseeded onto the
    vertex nearest to its centre before the update; the others move to the mean of their members; the loop stops when the fit sum changes
    by less than ``tol`` or after ``max_iter`` iterations. Clusters with at most 8 members are dropped, the labels are the arg-min over
    the kept ones. Everything is float64 (positions and the products of a float32 X are promoted, where the reference stays in float32);
    the embedding centres are rounded to X's type after every mean, as the reference's centre array has it.
    -> int64 [V] labels per mesh on the device; with ``return_state`` a second list of dict(seeds, n_iter, n_kept, members, centres_emb,
    centres_euc, fit) (host values) per mesh. Supported: n_clusters <= 64, D <= 128; beyond: ValueError."""
    n = len(X)
    if len(verts) != n:
        raise ValueError("kernel_kmeans: one entry per mesh in both lists")
    if n == 0:
        return ([], []) if return_state else []
    dev = device_of(*X, *verts)
    xs = [as_tensor(a) for a in X]
    D, sizes = int(xs[0].shape[1]), [int(x.shape[0]) for x in xs]
    if any(x.dim() != 2 or x.shape[1] != D or x.dtype != xs[0].dtype for x in xs) or xs[0].dtype not in (torch.float32, torch.float64):
        raise ValueError("kernel_kmeans: X is [V, D] float32 or float64, one width and type per batch")
    if any(len(verts[m]) != sizes[m] or sizes[m] < 1 for m in range(n)):
        raise ValueError("kernel_kmeans: verts has one row per row of X, and a mesh has at least one vertex")
    if not (1 <= int(n_clusters) <= KMEANS_MAX_CLUSTERS and 1 <= D <= KMEANS_MAX_DIM):
        raise ValueError(f"kernel_kmeans: n_clusters {n_clusters}, D {D}: supported are n_clusters <= {KMEANS_MAX_CLUSTERS} and "
                         f"D <= {KMEANS_MAX_DIM}")
    if first is None:
        rng = np.random if rng is None else rng
        first = [int(rng.randint(v)) for v in sizes]
    first = [int(f) for f in first]
    if len(first) != n or any(not 0 <= first[m] < sizes[m] for m in range(n)):
        raise ValueError("kernel_kmeans: first names one vertex per mesh")
    Xc = torch.cat([x.to(dev) for x in xs], 0).contiguous()
    pos = cat_to([as_tensor(v).reshape(-1, 3) for v in verts], dev, torch.float64)
    vptr = ptr_of(sizes)
    ops = get_ops()
    res = ops.kernel_kmeans(Xc, pos, torch.from_numpy(vptr.astype(np.int32)).to(dev), torch.tensor(first, dtype=torch.int32, device=dev),
                            int(n_clusters), int(max_iter), float(w_euc), float(tol))
    info = res["info"].cpu().numpy()                                                             # the status read
    for m in range(n):
        if info[m, 0] == ops.KMEANS_NO_CLUSTER:
            raise ValueError(f"kernel_kmeans: mesh {m}: no cluster keeps more than 8 members (the reference fails on its empty centre array)")
        if info[m, 0] != ops.KMEANS_OK:
            raise ValueError(f"kernel_kmeans: mesh {m}: status {int(info[m, 0])}")
    labels = [res["labels"][vptr[m]:vptr[m + 1]] for m in range(n)]
    if not return_state:
        return labels
    host = {k: res[k].cpu().numpy() for k in ("seeds", "members", "centres_emb", "centres_euc", "fit")}
    state = [dict(seeds=host["seeds"][m].astype(np.int64), n_iter=int(info[m, 1]), n_kept=int(info[m, 2]), members=host["members"][m],
                  centres_emb=host["centres_emb"][m], centres_euc=host["centres_euc"][m], fit=float(host["fit"][m])) for m in range(n)]
    return labels, state


# ------------------------------------------------------------------------------------------------------------------- segments of a rig
def segments_from_skins(skins: Sequence) -> List[torch.Tensor]:
    """``np.argmax(rig.skins, axis=1)`` (utils/piecewise_ransac.py:101) per mesh: the first joint on ties. An entry is a dense [V, J]
    array or tensor, or the device entries ``rigging.assemble_rigs(entries=True)`` leaves in ``Rig.skin_entries_device``: (vptr int32
    [V + 1], vertex, joint, weight). -> int64 [V] per mesh, on the device the input lives on."""
    out = []
    for s in skins:
        if isinstance(s, (tuple, list)) and len(s) == 4:
            vptr, vertex, joint, weight = (torch.as_tensor(t) for t in s)
            V = vptr.numel() - 1
            J = int(joint.max()) + 1 if joint.numel() else 1
            dense = torch.zeros(V, J, dtype=weight.dtype, device=weight.device)
            dense[vertex.long(), joint.long()] = weight
        else:
            dense = as_tensor(s)
        out.append(torch.argmax(dense, dim=1))
    return out
