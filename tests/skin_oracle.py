"""A plain float64 reference of every stage of morig_amd/geodesic.py and morig_amd/skinning.py: numpy and the standard library only
(torch on the CPU for the one float32 softmax). No GPU, no native library, nothing read from outside the repository. It is written
from the semantics the project documents (DESIGN.md sections 10 and 11, the docstrings of geodesic.py / skinning.py, the comments of
csrc/geodesic.hip and csrc/skin.hip); tests/test_skin_oracle.py pins it to the fixtures the reference's own functions made, and
tests/test_skin_geo_differential.py compares the device with it on generated inputs.

Clarity over speed. Where the kernels promise bitwise results the operation order is numpy's: a sum of three terms is spelled
``(x + y) + z`` (np.dot may go through a fused BLAS), products and sums round separately.
"""
import heapq

import numpy as np

KNN = 5
GRID = 88


def _sum3(a):
    """(x + y) + z over the last axis"""
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def _norm3(a):
    return np.sqrt(_sum3(a * a))


# ---------------------------------------------------------------------------------------------------------------- stage 1
class SampleGraph:
    """the filtered 5-NN graph of a sample set: ``nbr`` [S, 5] neighbour ids in ascending distance (the smaller index first among equal
    distances), ``keep`` [S, 5] the arcs that pass the normal filter, ``w`` [S, 5] the float32 weights, ``cos`` [S, 5];
    ``near7`` [S, 7] the distances self, 5 neighbours, the first sample left out (what the fixtures' margin is stated on);
    ``adj``: per node the list of (neighbour, weight as a Python float) of the UNDIRECTED graph, every pair once per end."""

    def __init__(self, pts, normals, block=256):
        pts, normals = np.asarray(pts, dtype=np.float64), np.asarray(normals, dtype=np.float64)
        S = len(pts)
        assert S >= KNN + 1 and normals.shape == pts.shape
        m = min(S, KNN + 3)                                       # self + 5 + the first left out (+ 1 spare)
        self.nbr = np.empty((S, KNN), dtype=np.int64)
        dn = np.empty((S, KNN))
        self.near7 = np.full((S, KNN + 2), np.inf)
        for s in range(0, S, block):
            d = np.sqrt(_sum3((pts[np.newaxis, :, :] - pts[s:s + block, np.newaxis, :]) ** 2))
            rows = np.arange(d.shape[0])
            d[rows, s + rows] = -1.0                              # self first, whatever coincides with it
            cand = np.argpartition(d, m - 1, axis=1)[:, :m] if m < S else np.tile(np.arange(S), (len(rows), 1))
            cd = np.take_along_axis(d, cand, 1)
            order = np.lexsort((cand, cd), axis=1)                # by distance, then by index
            cand, cd = np.take_along_axis(cand, order, 1), np.take_along_axis(cd, order, 1)
            assert (cand[:, 0] == s + rows).all()
            self.nbr[s:s + block] = cand[:, 1:KNN + 1]
            dn[s:s + block] = cd[:, 1:KNN + 1]
            n7 = min(m, KNN + 2)
            self.near7[s:s + block, :n7] = cd[:, :n7]
            self.near7[s:s + block, 0] = 0.0
        nq = normals[self.nbr]                                    # [S, 5, 3]
        num = _sum3(nq * normals[:, np.newaxis, :])
        self.cos = num / (_norm3(nq) * _norm3(normals)[:, np.newaxis] + 1e-10)
        self.keep = self.cos > -0.5
        self.w = dn.astype(np.float32)                            # the reference's float32 sparse matrix
        self.S = S
        pairs = {}
        for p, q, w in zip(np.repeat(np.arange(S), KNN)[self.keep.reshape(-1)].tolist(), self.nbr[self.keep].tolist(),
                           self.w[self.keep].tolist()):
            pairs[(min(p, q), max(p, q))] = w                     # both directions of a pair carry the same float32
        self.adj = [[] for _ in range(S)]
        for (p, q), w in pairs.items():
            self.adj[p].append((q, w))
            self.adj[q].append((p, w))
        self.n_entries = 2 * len(pairs)

    def margins(self):
        """(smallest gap among the 7 nearest distances of a sample, smallest |cos + 0.5|, arcs filtered)"""
        return float(np.diff(self.near7, axis=1).min()), float(np.abs(self.cos + 0.5).min()), int((~self.keep).sum())

    def components(self):
        """component label per node of the undirected graph"""
        lab = -np.ones(self.S, dtype=np.int64)
        n = 0
        for s in range(self.S):
            if lab[s] >= 0:
                continue
            lab[s] = n
            stack = [s]
            while stack:
                u = stack.pop()
                for v, _ in self.adj[u]:
                    if lab[v] < 0:
                        lab[v] = n
                        stack.append(v)
            n += 1
        return lab


def dijkstra_row(graph, src):
    """shortest float64 path lengths from ``src`` (left-to-right sums of the float32 weights), inf where unreachable"""
    dist = [float("inf")] * graph.S
    dist[src] = 0.0
    heap = [(0.0, src)]
    adj = graph.adj
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for v, w in adj[u]:
            c = d + w
            if c < dist[v]:
                dist[v] = c
                heapq.heappush(heap, (c, v))
    return np.array(dist)


def surface_geodesic_rows(pts, normals, sources, graph=None):
    """rows ``sources`` of the sample-to-sample matrix: shortest paths over the filtered 5-NN graph, an unreachable pair patched to
    8 + its Euclidean distance -> float64 [len(sources), S]"""
    pts = np.asarray(pts, dtype=np.float64)
    g = graph if graph is not None else SampleGraph(pts, normals)
    out = np.empty((len(sources), g.S))
    for i, s in enumerate(sources):
        row = dijkstra_row(g, int(s))
        unreached = np.isinf(row)
        if unreached.any():
            row[unreached] = 8.0 + np.sqrt(_sum3((pts[unreached] - pts[int(s)]) ** 2))
        out[i] = row
    return out


def nearest_sample(verts, pts, squared=False, block=512):
    """first minimum over the samples of the float64 (squared) distance -> (ids int64 [V], the minimum [V])"""
    verts, pts = np.asarray(verts, dtype=np.float64), np.asarray(pts, dtype=np.float64)
    ids = np.empty(len(verts), dtype=np.int64)
    best = np.empty(len(verts))
    for s in range(0, len(verts), block):
        d = _sum3((verts[s:s + block, np.newaxis, :] - pts[np.newaxis, :, :]) ** 2)
        if not squared:
            d = np.sqrt(d)
        ids[s:s + block] = np.argmin(d, axis=1)
        best[s:s + block] = d[np.arange(d.shape[0]), ids[s:s + block]]
    return ids, best


# ---------------------------------------------------------------------------------------------------------------- stages 2 and 3
def pts2line(pos, bones):
    """the nearest point of every bone to every vertex and its distance -> (origins [V, nb, 3], dist [V, nb]); a bone whose squared
    length is below 1e-8 is its start point"""
    pos, bones = np.asarray(pos, dtype=np.float64), np.asarray(bones, dtype=np.float64)
    V, nb = len(pos), len(bones)
    origins = np.empty((V, nb, 3))
    for c in range(nb):
        a, e = bones[c, 0:3], bones[c, 3:6] - bones[c, 0:3]
        l2 = _sum3(e * e)
        if np.abs(l2) < 1e-8:
            origins[:, c] = a
        else:
            t = np.clip(_sum3((pos - a) * e) / l2, 0.0, 1.0)
            origins[:, c] = a + t[:, np.newaxis] * e
    return origins, _norm3(origins - pos[:, np.newaxis, :])


def ray_caster(mesh, origins, ends):
    """float64 Moeller-Trumbore over all triangles (the rule of csrc/geodesic.hip) -> (visible, per-ray record of
    |min_hit - length| and the nearest hit's smallest barycentric clearance)"""
    tri_pos, faces = mesh
    tri_pos = np.asarray(tri_pos, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    A = tri_pos[faces[:, 0]]
    E1, E2 = tri_pos[faces[:, 1]] - A, tri_pos[faces[:, 2]] - A
    Nn = np.linalg.norm(np.cross(E1, E2), axis=1)
    n = len(origins)
    vis = np.zeros(n, dtype=bool)
    delta = np.zeros(n)
    bary = np.full(n, np.inf)
    length = np.linalg.norm(ends - origins, axis=1)
    if len(faces) == 0:                                            # nothing to hit: min_hit is the ray's length
        return np.ones(n, dtype=bool), dict(delta=delta, bary=bary, length=length)
    for s in range(0, n, 512):
        o = origins[s:s + 512, None, :]
        d = (ends[s:s + 512] - origins[s:s + 512] + 1e-15)[:, None, :]
        dn = np.linalg.norm(d, axis=2)
        P = np.cross(d, E2[None])
        det = np.sum(E1[None] * P, axis=2)
        ok = np.abs(det) > 1e-12 * dn * Nn[None]
        inv = 1.0 / np.where(ok, det, 1.0)
        T = o - A[None]
        u = np.sum(T * P, axis=2) * inv
        Q = np.cross(T, E1[None])
        v = np.sum(d * Q, axis=2) * inv
        t = np.sum(E2[None] * Q, axis=2) * inv
        hit = ok & (u >= -1e-12) & (u <= 1 + 1e-12) & (v >= -1e-12) & (u + v <= 1 + 1e-12) & (t > 0)
        h = np.where(hit, np.linalg.norm(t[..., None] * d, axis=2), np.inf)
        j = np.argmin(h, axis=1)
        rows = np.arange(len(j))
        mh = np.where(np.isinf(h[rows, j]), length[s:s + 512], h[rows, j])
        delta[s:s + 512] = np.abs(mh - length[s:s + 512])
        vis[s:s + 512] = delta[s:s + 512] < 1e-4
        b = np.minimum(np.minimum(u[rows, j], v[rows, j]), 1.0 - u[rows, j] - v[rows, j])
        bary[s:s + 512] = np.where(np.isinf(h[rows, j]), np.inf, np.abs(b))
    return vis, dict(delta=delta, bary=bary, length=length)


def bone_visibility(pos, bones, tri_pos, tri_faces):
    """every (vertex, bone) ray of a mesh -> (visible bool [V, nb], unsure bool [V, nb], record): ``unsure`` marks the rays whose
    outcome rests on the order of float64 operations: ||min_hit - length| - 1e-4| < 5e-5, a length below 1e-9, or an invisible ray
    whose nearest hit lies within 1e-6 of a triangle edge"""
    pos = np.asarray(pos, dtype=np.float64)
    origins, _ = pts2line(pos, bones)
    V, nb = origins.shape[:2]
    ends = np.repeat(pos[:, np.newaxis, :], nb, axis=1)
    vis, rec = ray_caster((tri_pos, tri_faces), origins.reshape(-1, 3), ends.reshape(-1, 3))
    unsure = (np.abs(rec["delta"] - 1e-4) < 5e-5) | (rec["length"] < 1e-9) | (~vis & np.isfinite(rec["bary"]) & (rec["bary"] < 1e-6))
    return vis.reshape(V, nb), unsure.reshape(V, nb), rec


def restate(dist, vis, sg, block=256):
    """the vertex-to-bone matrix given the visibility, with numpy's own percentile, keeping what the function does not return
    -> (out, visible_after, nn, percentile, the smallest |dist - 1.3 percentile|, the number of 8 + dist entries)"""
    dist, sg = np.asarray(dist, dtype=np.float64), np.asarray(sg)
    vis = np.asarray(vis).astype(bool).copy()
    V, nb = dist.shape
    pct = np.full(nb, np.nan)
    margin = np.inf
    for b in range(nb):
        ids = np.flatnonzero(vis[:, b])
        if len(ids) == 0:
            continue
        pct[b] = np.percentile(dist[ids, b], 15)
        margin = min(margin, np.abs(dist[:, b] - 1.3 * pct[b]).min())
        vis[dist[:, b] > 1.3 * pct[b], b] = False
    out = np.where(vis, dist, 0.0)
    nn = -np.ones((V, nb), dtype=np.int32)
    n_inf = 0
    for c in range(nb):
        ids = np.flatnonzero(vis[:, c])
        if len(ids) == 0:
            out[:, c] = dist[:, c]
            continue
        inv = np.flatnonzero(~vis[:, c])
        for s in range(0, len(inv), block):
            r = inv[s:s + block]
            sub = sg[np.ix_(r, ids)]
            j = np.argmin(sub, axis=1)                             # the first minimum in vertex order
            best = sub[np.arange(len(r)), j]
            nn[r, c] = ids[j]
            far = np.isinf(best)
            n_inf += int(far.sum())
            out[r, c] = np.where(far, 8.0 + dist[r, c], best + dist[ids[j], c])
    return out, vis, nn, pct, margin, n_inf


def geodesic_matrix_subsampled(pos, sub_ids, dist_sub, vis_sub, sg):
    """the sub-sampled form: the matrix on pos[ids] with sg[ids][:, ids]; every vertex takes the row of its nearest sub-sample by
    squared distance -> (out [V, nb], nn_sub [V])"""
    pos, sub_ids = np.asarray(pos, dtype=np.float64), np.asarray(sub_ids)
    out = restate(dist_sub, vis_sub, np.asarray(sg)[sub_ids][:, sub_ids])[0]
    nn_sub = nearest_sample(pos, pos[sub_ids], squared=True)[0]
    return out[nn_sub], nn_sub


def bind_joint2rig(geo, bones, is_leaf, k):
    """the bind loop at inference time: the k nearest bones by the float64 distance, equal distances by ascending bone id; per slot
    the bone (6), 1 / (D + 1e-10), the leaf flag; a slot past the bone count repeats the nearest bone with skin_nn = 0 and
    loss_mask = 0 -> (skin_input float32 [V, 8k], skin_nn int64 [V, k], loss_mask int64 [V, k])"""
    geo, bones = np.asarray(geo, dtype=np.float64), np.asarray(bones, dtype=np.float64)
    leaf = np.asarray(is_leaf).astype(np.float64).reshape(-1)
    V, nb = geo.shape
    order = np.argsort(geo, axis=1, kind="stable")
    rows = np.zeros((V, k, 8))
    nn = np.zeros((V, k), dtype=np.int64)
    mask = np.zeros((V, k), dtype=np.int64)
    ar = np.arange(V)
    for s in range(k):
        t = order[:, s] if s < nb else order[:, 0]
        rows[:, s, 0:6] = bones[t]
        rows[:, s, 6] = 1.0 / (geo[ar, t] + 1e-10)
        rows[:, s, 7] = leaf[t]
        if s < nb:
            nn[:, s], mask[:, s] = t, 1
    return rows.reshape(V, 8 * k).astype(np.float32), nn, mask


# ---------------------------------------------------------------------------------------------------------------- volumetric geodesic
def voxel_index(p, translate, scale, dims0):
    """np.round is half to even; clipped to the grid"""
    v = np.round((np.asarray(p, dtype=np.float64) - np.asarray(translate, dtype=np.float64)) / float(scale) * float(dims0))
    return np.clip(v, 0, GRID - 1).astype(np.int64)


def bone_seeds(bone):
    """the bone's start point and the points start + (end - start) / (n + 1e-30) * i, i = 1 .. n - 1, n = round(length / 0.01)"""
    p, c = np.asarray(bone[0:3], dtype=np.float64), np.asarray(bone[3:6], dtype=np.float64)
    d = p - c
    n = np.round(np.sqrt(_sum3(d * d)) / 0.01)
    unit = (c - p) / (n + 1e-30)
    i = np.arange(1, n)
    return np.concatenate([p[np.newaxis, :], p + unit[np.newaxis, :] * i[:, np.newaxis]], 0)


def _shift_or(a, axis):
    """a | a shifted by +-1 along ``axis``, nothing enters across the border"""
    out = a.copy()
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    out[tuple(hi)] |= a[tuple(lo)]
    out[tuple(lo)] |= a[tuple(hi)]
    return out


def dilate(a):
    """3 x 3 x 3 binary dilation"""
    return _shift_or(_shift_or(_shift_or(a, 0), 1), 2)


def boundary6(a):
    """the voxels of ``a`` with a 6-neighbour outside ``a`` (outside the grid counts as outside) -> int64 [n, 3] in scan order"""
    p = np.zeros((GRID + 2,) * 3, dtype=bool)
    p[1:-1, 1:-1, 1:-1] = a
    inner = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return np.argwhere(a & ~inner)


def volumetric_geodesic_bone(mask, bone, translate, scale, dims0, return_info=False):
    """the layer map of one (grid, bone): a breadth-first search by 3 x 3 x 3 dilation under the occupancy mask from the bone's seeds
    (a seed outside the mask stays reached and grows into the mask); the layer counter advances on every dilation, also one that
    reaches nothing; a dilation that reaches nothing is followed by the patch: every unreached occupied voxel at the smallest distance
    to the reached set is reached with (the smallest layer among its equally near reached voxels) + 1; the count the loop compares
    against is the one before the patch. -> (layer int64 [88, 88, 88], reached bool) (+ dict(patches, patched, steps, layer_ties):
    layer_ties counts the patched voxels whose equally near reached voxels differ in layer)"""
    mask = np.asarray(mask).astype(bool)
    assert mask.shape == (GRID,) * 3
    sv = voxel_index(bone_seeds(bone), translate, scale, dims0)
    reached = np.zeros_like(mask)
    reached[sv[:, 0], sv[:, 1], sv[:, 2]] = True
    layer = np.zeros(mask.shape, dtype=np.int64)
    counter, patches, patched, steps, layer_ties = 1, 0, 0, 0, 0
    last = int((mask & ~reached).sum())
    while last > 0:
        new = dilate(reached) & mask & ~reached
        layer[new] = counter
        counter += 1
        steps += 1
        reached |= new
        this = int((mask & ~reached).sum())
        if this == last:
            A, R = boundary6(mask & ~reached), boundary6(reached)
            chunk = max(1, (1 << 22) // max(len(R), 1))           # squared distances are integers: they compare exactly
            d2 = lambda s: np.sum((A[s:s + chunk, np.newaxis, :] - R[np.newaxis, :, :]) ** 2, axis=2)
            D = min(int(d2(s).min()) for s in range(0, len(A), chunk))
            lr = layer[R[:, 0], R[:, 1], R[:, 2]]
            for s in range(0, len(A), chunk):
                at = d2(s) == D
                hit = at.any(axis=1)
                a = A[s:s + chunk][hit]
                new_layer = np.where(at, lr[np.newaxis, :], np.iinfo(np.int64).max).min(axis=1)[hit] + 1
                layer_ties += int((np.where(at, lr[np.newaxis, :], -1).max(axis=1)[hit] + 1 != new_layer).sum())
                layer[a[:, 0], a[:, 1], a[:, 2]] = new_layer      # A and R are disjoint: ``lr`` is the state before the patch
                reached[a[:, 0], a[:, 1], a[:, 2]] = True
                patched += int(hit.sum())
            patches += 1
        last = this
    info = dict(patches=patches, patched=patched, steps=steps, layer_ties=layer_ties)
    return (layer, reached, info) if return_info else (layer, reached)


def volumetric_geodesic(pos, mask, bones, translate, scale, dims0, return_info=False):
    """the layer at every vertex's voxel for every bone; a voxel never reached reads 0 -> int64 [V, nb]"""
    vv = voxel_index(pos, translate, scale, dims0).reshape(-1, 3)
    bones = np.asarray(bones, dtype=np.float64).reshape(-1, 6)
    out = np.zeros((len(vv), len(bones)), dtype=np.int64)
    infos = []
    for b in range(len(bones)):
        layer, reached, info = volumetric_geodesic_bone(mask, bones[b], translate, scale, dims0, return_info=True)
        out[:, b] = np.where(reached[vv[:, 0], vv[:, 1], vv[:, 2]], layer[vv[:, 0], vv[:, 1], vv[:, 2]], 0)
        infos.append(info)
    return (out, infos) if return_info else out


# ---------------------------------------------------------------------------------------------------------------- bind rows, weights
def stable_rows(dist, is_leaf, k):
    """the k nearest bones by the integer distance, ties by ascending bone id -> (ids int64 [V, k], -1 past the bone count; 1/D)"""
    V, nb = dist.shape
    ids = -np.ones((V, k), dtype=np.int64)
    invd = np.zeros((V, k))
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    m = min(k, nb)
    ids[:, :m] = order[:, :m]
    invd[:, :m] = 1.0 / (np.take_along_axis(dist, order[:, :m], 1).astype(np.int64) + 1e-10)
    return ids, invd


def labels_of(ids, skins, start_jid):
    """per slot the skin weight of the bone's start joint when positive and not taken by an earlier slot of the vertex"""
    out = np.zeros(ids.shape)
    for v in range(ids.shape[0]):
        used = set()
        for s in range(ids.shape[1]):
            if ids[v, s] < 0:
                continue
            j = int(start_jid[ids[v, s]])
            w = skins[v, j]
            if w > 0 and j not in used:
                out[v, s] = w
                used.add(j)
    return out


def labels(ids, rig, bone_names):
    return labels_of(ids, np.asarray(rig.skins), [rig.names.index(n[0]) for n in bone_names])


def bind_tensors(ids, invd, bones, is_leaf, start_jid):
    """the dataset tensors of the bind rows: an invalid slot repeats slot 0 with loss_mask 0
    -> (skin_input float32 [V, 8k], skin_nn, loss_mask, skin_nnjids int64 [V, k])"""
    bones = np.asarray(bones, dtype=np.float64)
    leaf = np.asarray(is_leaf).astype(np.float64).reshape(-1)
    sj = np.asarray(start_jid, dtype=np.int64)
    V, k = ids.shape
    valid = ids >= 0
    t = np.where(valid, ids, ids[:, :1])
    tinv = np.where(valid, invd, invd[:, :1])
    rows = np.zeros((V, k, 8))
    rows[:, :, 0:6] = bones[t]
    rows[:, :, 6] = tinv
    rows[:, :, 7] = leaf[t]
    return rows.reshape(V, 8 * k).astype(np.float32), t.astype(np.int64), valid.astype(np.int64), sj[t]


def one_ring(tpl_edge_index, n):
    """per vertex the sorted unique neighbours over the edges in both directions, self excluded"""
    e = np.asarray(tpl_edge_index, dtype=np.int64)
    ring = [set() for _ in range(n)]
    for a, b in zip(e[0].tolist(), e[1].tolist()):
        if a != b:
            ring[a].add(b)
            ring[b].add(a)
    return [sorted(r) for r in ring]


def skin_weights(logits, skin_nn, loss_mask, tpl_edge_index, n_bones, mode="train_skin", ratio=None):
    """SkinNet logits of ONE mesh -> weights float64 [V, n_bones]. "train_skin": float32 softmax, then x loss_mask, ratio 0.5;
    "joint2rig": logits x loss_mask, then the softmax, ratio 0.35. The mask-1 slots are scattered at skin_nn, every vertex takes the
    mean over its unique 1-ring neighbours (a vertex without neighbours keeps its own row), entries below ratio x row maximum are
    cleared, rows are divided by their sum + 1e-10."""
    import torch
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32))
    nn, msk = np.asarray(skin_nn, dtype=np.int64), np.asarray(loss_mask, dtype=np.int64)
    k = x.shape[1]
    nn, msk = nn[:, :k], msk[:, :k]
    m = torch.from_numpy(msk).float()
    if mode == "train_skin":
        p = (torch.softmax(x, dim=1) * m).numpy().astype(np.float64)
        ratio = 0.5 if ratio is None else ratio
    elif mode == "joint2rig":
        p = torch.softmax(x * m, dim=1).numpy().astype(np.float64)
        ratio = 0.35 if ratio is None else ratio
    else:
        raise ValueError(mode)
    V = x.shape[0]
    P = np.zeros((V, n_bones))
    for v in range(V):
        for s in range(k):
            if msk[v, s] == 1 and 0 <= nn[v, s] < n_bones:
                P[v, nn[v, s]] = p[v, s]
    W = np.empty_like(P)
    for v, ring in enumerate(one_ring(tpl_edge_index, V)):
        if ring:
            acc = np.zeros(n_bones)
            for u in ring:
                acc = acc + P[u]
            W[v] = acc / float(len(ring))
        else:
            W[v] = P[v]
    W[W < W.max(axis=1, keepdims=True) * ratio] = 0.0
    return W / (W.sum(axis=1, keepdims=True) + 1e-10)
